"""Test-side restatement of the naive sequence's codon posteriors (K9) on the oracle HMM's dense matrices.

Three forms of the same [n_codons][125] table (entry 25 b1 + 5 b2 + b3 over linearham_amd.posterior.BASES), all built from
oracle.linearham_oracle.HMM's dense members through tests/posterior_oracle.py (neither is changed):
  enumerated    every state path of non-zero probability, its naive sequence, its codons;
  dense         the three-position smoothing formula  P(k, k2, k3) = pi_{t+2}(k3) B_{t+1}(k2 | k3) B_t(k | k2)  with
                B_t(k | k2) = F_t[k] T(k -> k2) / Z_t(k2)  on the oracle's forward arrays;
  from_compact  the dense form's window codons and gene posteriors expanded by linearham_amd.posterior.codon_table."""
import numpy as np

from linearham_amd import posterior as lp
from tests import posterior_oracle as po


def _forward_rows(h, forward=None):
    igh = h.locus == "igh"
    fw = forward if forward is not None else {k: getattr(h, k) for k in (
        "vgerm_forward", "vd_junction_forward", "jgerm_forward") + (("dgerm_forward", "dj_junction_forward") if igh else ())}
    return {k[:-len("_forward")]: np.asarray(v, dtype=np.float64) for k, v in fw.items()}


def chain_rows(h):
    """The chain as po._rows unrolls it, with what every state of every row writes: a list of dicts(name, row, T = the
    transition INTO the row, writes = per state a list of (site, base))."""
    ss = po.state_space(h)
    site0 = {j[0]: j[3] for j in lp._junctions(ss)}
    out = []
    for name, i, e, T in po._rows(*po._chain(h)):
        ranges, sites, bases = (ss[name + "_" + f] for f in po.REGION_FIELDS)
        if i is None:
            writes = [[(sites[k], bases[k]) for k in range(*ranges[g])] for g in sorted(ranges)]
        else:
            s = site0[name] + i
            writes = [[(s, bases[k])] if sites[k] in (-1, s) else [] for k in range(len(bases))]
        assert len(writes) == len(e)
        out.append(dict(name=name, row=i, T=T, e=e, writes=writes))
    return out


def n_codons(L, frame):
    return (L - frame) // 3 if L >= frame else 0


def enumerated(h, frame):
    """([n_codons][125] table, [(probability, naive sequence)]) from every state path with non-zero probability."""
    rows = chain_rows(h)
    L = h.msa.shape[1]
    n = len(rows)
    paths = []

    def rec(t, k, w, path):
        if t == n - 1:
            paths.append((w, path))
            return
        e1, T1 = rows[t + 1]["e"], rows[t + 1]["T"]
        for k2 in np.nonzero(T1[k] * e1)[0]:
            rec(t + 1, k2, w * T1[k, k2] * e1[k2], path + [k2])

    e0 = rows[0]["e"]
    for k in np.nonzero(e0)[0]:
        rec(0, k, e0[k], [k])
    total = sum(w for w, _ in paths)
    nc = n_codons(L, frame)
    table = np.zeros((nc, 125))
    seqs = []
    for w, path in paths:
        seq = [4] * L
        for t, k in enumerate(path):
            for s, b in rows[t]["writes"][k]:
                seq[s] = b
        for c in range(nc):
            b = seq[frame + 3 * c:frame + 3 * c + 3]
            table[c, 25 * b[0] + 5 * b[1] + b[2]] += w / total
        seqs.append((w / total, "".join(lp.BASES[b] for b in seq)))
    return table, seqs


def dense(h, frame, forward=None):
    """[n_codons][125] by the smoothing formula over at most three consecutive chain rows per codon, and the per-row
    posteriors {region: array} it used (po.smoothing)."""
    rows = chain_rows(h)
    L = h.msa.shape[1]
    post = po.smoothing(h, forward)
    F = _forward_rows(h, forward)

    def of(d, r):
        return d[r["name"]] if r["row"] is None else d[r["name"]][r["row"]]
    pis = [of(post, r) for r in rows]
    fs = [of(F, r) for r in rows]
    row_of_site = {}
    for t, r in enumerate(rows):
        for wr in r["writes"]:
            for s, _ in wr:
                assert row_of_site.setdefault(s, t) == t  # a site belongs to one chain row
    nc = n_codons(L, frame)
    table = np.zeros((nc, 125))

    def back(t, v):  # sum_k2 B_t(. | k2) v[k2]
        T = rows[t + 1]["T"]
        Z = fs[t] @ T
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(v != 0, v / np.where(v != 0, Z, 1.0), 0.0)
        return fs[t] * (T @ rho)

    for c in range(nc):
        sites = [frame + 3 * c + o for o in range(3)]
        ts = sorted({row_of_site[s] for s in sites if s in row_of_site})
        if not ts:
            table[c, 124] = 1.0
            continue
        assert ts == list(range(ts[0], ts[-1] + 1)) and len(ts) <= 3, ts
        # what each state of each touched row adds to the all-N index 124
        delta = []
        for t in ts:
            d = np.zeros(len(rows[t]["writes"]), dtype=np.int64)
            for k, wr in enumerate(rows[t]["writes"]):
                for s, b in wr:
                    if s in sites:
                        d[k] += (b - 4) * 5 ** (2 - sites.index(s))
            delta.append(d)

        def down(level, v, idx):
            """v: the joint of the rows above `level` with row ts[level], as a vector over that row's states."""
            d = delta[level]
            for val in np.unique(d[v != 0]):
                vm = np.where(d == val, v, 0.0)
                if level == 0:
                    table[c, idx + val] += vm.sum()
                else:
                    down(level - 1, back(ts[level - 1], vm), idx + val)
        down(len(ts) - 1, pis[ts[-1]], 124)
    return table, post


def window_inputs(h, table, post, frame):
    """What the device writes, from the dense form: (windows [n_window][125], genes [n_genes] V | D | J, layout)."""
    ss = po.state_space(h)
    lay = lp.codon_layout(ss, frame)
    regions = ["vgerm"] + (["dgerm"] if h.locus == "igh" else []) + ["jgerm"]
    genes = np.concatenate([post[r] for r in regions])
    return table[lay["window_codon"]], genes, lay


def from_compact(h, table, post, frame):
    windows, genes, lay = window_inputs(h, table, post, frame)
    return lp.codon_table(po.state_space(h), windows, genes, lay)


def product_of_marginals(table):
    """The table a product-of-site-marginals shortcut would give."""
    t = np.asarray(table).reshape(-1, 5, 5, 5)
    m1, m2, m3 = t.sum(axis=(2, 3)), t.sum(axis=(1, 3)), t.sum(axis=(1, 2))
    return np.einsum("ca,cb,cd->cabd", m1, m2, m3).reshape(-1, 125)
