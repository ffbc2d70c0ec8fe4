"""Helper of tests/test_gpu_lineage_cadence.py: K11 (lh_asr_marginals_batch), K12 (lh_asr_edges_batch, full and lean), K13b's
conditional tables, K14 (lh_asr_node_codons_batch) and K15 (lh_asr_codon_edges_batch) on the rows of tests/cadence_cases.py
where the upward pass needs more than one 2^256 rescaling per op (the compound family) or runs deep (cad190's lossy and
zeroed rows), against the exact lineage reference (tests/exact_lineage_oracle.py).

  python tests/lineage_cadence_worker.py --cpu DIR [--jobs N]   CPU: DIR/lineage_<row>.npz per row -- the exact tables per seed
                                                                tip on the alignment's distinct columns, and d_ref, the distance
                                                                of the double-precision oracles from them
  python tests/lineage_cadence_worker.py --gpu DIR --family F   GPU: every row of family F, three seed tips, three naive-base
                                                                distributions; one JSON line {"failures": .., "figures": ..}
  python tests/lineage_cadence_worker.py --gpu-codons DIR --family F
                                                                GPU: K15 (lh_asr_codon_edges_batch: K15b's cond_edge and the
                                                                five tables) and K14 (lh_asr_node_codons_batch, both nodes) on
                                                                the same rows, COMBOS x Q_KINDS at the codon level; for cmp180
                                                                the evaluation forms too (eval_forms); one JSON line

d_ref: tests/ancestral_marginal_oracle.marginals and tests/edge_oracle.edges restate the device's formulas in doubles (per
rate one message passed down the path, every table normalised per rate).  Here they get the exact model's P-matrices rounded
to double and an upward pass with the device's arithmetic -- after every node, 2^256 until the largest entry is back at or
above 2^-256 (upward_until) -- so that d_ref is what double precision itself costs on the row.  The device is held to
max(1e-10, 8 d_ref) per row, seed tip and table (the rule of tests/test_gpu_extreme_parameters.py; 1e-10 is the project's
bound for these tables, ancestral_cases.BOUND).

The codon level (K14, K15).  K15b's H[s][j][b][a][c] is ExactLineage.tables' cond_edge itself; its d_ref comes from
tests/codon_edge_oracle.cond_edges on the same `pre`.  K15's five tables and K14's two are contractions of H (of cond at
slot 0 and at the last slot) with a naive codon posterior Q [C][125] (codon_q_of): the reference is
codon_edge_oracle.tables / node_codon_oracle.contraction and .change fed the EXACT H and cond -- the contraction itself is
done in doubles, its operands are probabilities and a sum has at most 125 non-negative terms -- and d_ref the distance of
the same functions fed the double-precision H and cond.  The --cpu side stores the reference tables per seed tip, Q kind and
frame in the row's npz (k15_<tip number>_<kind>_<frame>_<table>, k14_..._<node>_<table>) and prints, for the two rows whose
joins need more than one rescaling, how far one rescaling per node puts H from the exact tables (one_rescale_of_row)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# family -> seed tips (tip ids: alignment row + 1).  cmp180: under the block's first ladder a tip that differs on the deep
# columns (44) and one that does not (41), and a background tip on the ladder above the block (101).  cad190: a tip of the
# mutated stretch of four deep columns (26), a tip of tree A's cherries (151), a tip near the root (181).
SEEDS = {"cmp180": (44, 41, 101), "cad190": (26, 151, 181)}
ROW_CLASSES = ("compound_control", "compound_clear", "compound_lossy", "compound_zeroed", "lossy", "zeroed")
Q_KINDS = ("one_hot", "dirichlet", "all_n")
K11_TABLES = ("marg", "rate_post")
K12_TABLES = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
LEAN_TABLES = K12_TABLES[1:]          # without "edge" lh_asr_edges_batch runs the lean kernel
K15_TABLES = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")      # codon_edges_cases.TABLES
K14_TABLES = ("codons", "change")
# (seed tip number, frame) of the codon-level cases: frame 0 for every seed tip, frames 1 and 2 for the first, so that every
# deep site (cmp180: 5, 23, 29, 44; cad190: 5, 9, 17, 23, 29, 40, 44) takes every position in a codon
COMBOS = ((0, 0), (0, 1), (0, 2), (1, 0), (2, 0))
FLOOR = 1e-10


def rows_of(family):
    from tests import cadence_cases as cc
    return [r for r in cc.ROWS if r[1] == family and r[2] in ROW_CLASSES]


def naive_rows(h):
    """The naive sequence's base per site, as the family's xMSA has it."""
    from tests import cadence_cases as cc
    site = cc.kc.column_sites(h)
    col_of = {}
    for c in range(len(site)):
        col_of.setdefault(int(site[c]), c)
    return np.array([int(h.xmsa[0, col_of[t]]) for t in range(h.msa.shape[1])])


def q_of(kind, h, n):
    """[n][L][5]: the naive sequence one-hot, benign Dirichlet rows (exact zeros, mass on N and one-hot rows among them),
    all mass on N."""
    from tests.ancestral_cases import naive_dist
    L = h.msa.shape[1]
    if kind == "one_hot":
        return np.tile(np.eye(5)[naive_rows(h)], (n, 1, 1))
    if kind == "dirichlet":
        return naive_dist(np.random.default_rng(2311), n, L)
    return np.tile(np.eye(5)[4], (n, L, 1))


def codon_q_of(kind, h, frame):
    """[C][125], C = (L - frame) // 3: Q_KINDS at the codon level -- the naive sequence's triple one-hot (entry 25 b1 + 5 b2
    + b3, an N base as 4), sparse Dirichlet rows from a fixed seed (codon_edges_cases.dirichlet_codons), all mass on NNN."""
    from tests.codon_edges_cases import dirichlet_codons
    C = (h.msa.shape[1] - frame) // 3
    if kind == "one_hot":
        b = naive_rows(h)[frame:frame + 3 * C].reshape(C, 3)
        return np.eye(125)[25 * b[:, 0] + 5 * b[:, 1] + b[:, 2]]
    if kind == "dirichlet":
        return dirichlet_codons(np.random.default_rng(2611 + frame), C)
    return np.tile(np.eye(125)[124], (C, 1))


def upward_until(children, root, T, tips, P, until=True):
    """oracle/asr_oracle.upward with the device's rescaling: after every node, times 2^256 until the largest entry is back
    at or above 2^-256 (an all-zero vector once; the device's rescale_steps wherever an op's product is a normal number,
    cadence_cases.restate_walk says where they part).  until=False: one rescaling per node, the arithmetic before the fix of
    the tree joins.  Returns clv [2T-2][L][4] and the log of the scale taken out per site."""
    L = tips.shape[1]
    onehot = np.concatenate([np.eye(4), np.ones((1, 4))], axis=0)
    clv, count = np.zeros((2 * T - 2, L, 4)), np.zeros(L)
    for t in range(T):
        clv[t] = onehot[tips[t]]
    order, stack = [], [int(root)]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(int(c) for c in children[2 * (v - T):2 * (v - T) + 2] if c >= T)
    for v in reversed(order):
        a, b = children[2 * (v - T)], children[2 * (v - T) + 1]
        x = np.einsum("ij,lj->li", P[a], clv[a]) * np.einsum("ij,lj->li", P[b], clv[b])
        need = x.max(axis=1) < 2.0 ** -256
        while need.any():
            x = np.where(need[:, None], x * 2.0 ** 256, x)
            count += need
            if not until:
                break
            need = need & (x.max(axis=1) < 2.0 ** -256) & (x.max(axis=1) > 0)
        clv[v] = x
    return clv, -256.0 * np.log(2.0) * count


def double_pre(children, root, T, msa, pi, P, until=True):
    """ancestral_marginal_oracle._per_rate on given P-matrices [2T-2][R][4][4] with upward_until."""
    from tests import ancestral_marginal_oracle as amo
    L, R = msa.shape[1], P.shape[1]
    tips = np.concatenate([np.full((1, L), 4, dtype=msa.dtype), msa], axis=0)
    clvs, logscale, w = [], np.zeros((R, L)), np.zeros((R, L, 5))
    for k in range(R):
        clv, ls = upward_until(children, root, T, tips, P[:, k], until)
        clvs.append(clv)
        logscale[k] = ls
        w[k] = (np.asarray(pi)[None, :] * clv[root]) @ (P[0, k] @ amo.ONEHOT.T)
    with np.errstate(under="ignore"):
        lik = w * np.exp(logscale - logscale.max(axis=0, keepdims=True))[:, :, None]
    return P, clvs, lik


def _row_setup(family, row):
    """What the exact side of a row starts from: the family, the row's sample and tree, the exact model and lineage, and the
    double-precision oracles' `pre` (exact P-matrices rounded to double, upward_until)."""
    import shutil
    import tempfile
    from tests import cadence_cases as cc
    from tests import exact_lineage_oracle as xl
    from tests import exact_model_oracle as ex
    work = tempfile.mkdtemp(prefix="lh_lineage_cadence_")
    try:
        h = cc.load_family(family, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    sample, R = cc.sample_of(row)
    T, children, root, brlen, ops, depth = cc.schedule(h, sample)
    rates = ex.gamma_rates_mean(sample["alpha"], R)                       # doubles: what the entry points are given
    model = ex.ExactModel(sample["er"], sample["pi"], [float(r) for r in rates])
    msa = np.asarray(h.msa)
    lin = xl.ExactLineage(model, T, children, root, brlen, msa)
    Pd = model.pmatrices_double(brlen)
    pre = double_pre(np.asarray(children).ravel(), root, T, msa, sample["pi"], Pd)
    return dict(h=h, sample=sample, T=T, children=children, root=root, brlen=brlen, rates=rates, msa=msa, lin=lin, P=Pd, pre=pre)


def _far(a, b):
    """The largest distance of two tables; not finite counts as infinitely far."""
    with np.errstate(invalid="ignore"):
        return float(np.abs(a - b).max()) if np.isfinite(a).all() and np.isfinite(b).all() else float("inf")


def exact_of_row(args):
    """One row in a pool process: the exact tables per seed tip (on the distinct columns), the exact codon-level tables of K14
    and K15 per seed tip, frame and Q kind (COMBOS, codon_q_of), and d_ref per seed, q and table."""
    import time
    from tests import ancestral_marginal_oracle as amo
    from tests import ancestral_probs_oracle as apo
    from tests import codon_edge_oracle as ceo
    from tests import edge_oracle as eo
    from tests import exact_lineage_oracle as xl
    from tests import node_codon_oracle as nco
    family, row = args
    t0 = time.perf_counter()
    s = _row_setup(family, row)
    h, sample, T, children, root, brlen, rates, msa, lin, pre = (s[k] for k in ("h", "sample", "T", "children", "root", "brlen",
                                                                               "rates", "msa", "lin", "pre"))
    first = [int(np.nonzero(lin.pattern_of == p)[0][0]) for p in range(len(lin.patterns))]
    keep = {"pattern_of": lin.pattern_of, "rates": rates}
    d_ref = {}
    for si, tip in enumerate(SEEDS[family]):
        path = amo.seed_path(children, root, T, tip)
        tab = lin.tables(path, tip)
        for k in ("cond", "cond_edge"):
            keep["%s_%d" % (k, si)] = tab[k][:, first]
        keep["rate_%d" % si] = tab["rate"][first]
        d13, G = {}, {}
        for node, slot in (("parent", 0), ("mrca", len(path) - 1)):
            with np.errstate(all="ignore"):
                G[node] = apo.cond_tables(children, root, brlen, T, msa, sample["er"], sample["pi"], rates, path,
                                          apo.PARENT if slot == 0 else apo.MRCA, pre=pre)
            d13["k13_" + node] = float(np.abs(G[node] - tab["cond"][slot]).max())
        # K15b's H: the double-precision oracle, five basis vectors through edge_oracle.edges on the same `pre`
        with np.errstate(all="ignore"):
            H = ceo.cond_edges(children, root, brlen, T, msa, sample["er"], sample["pi"], rates, path, tip, pre=pre)
        d13["k15_cond_edge"] = _far(H, tab["cond_edge"])
        d_ref["%d_cond" % si] = d13
        for kind in Q_KINDS:
            q = q_of(kind, h, 1)[0]
            want = xl.mix(tab, q)
            with np.errstate(all="ignore"):
                marg, rp = amo.marginals(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, pre=pre)
                ed = eo.edges(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, tip, pre=pre)
            d = {"k11_marg": np.abs(marg - want["marg"]).max(), "k11_rate_post": np.abs(rp - want["rate_post"]).max()}
            d.update({"k12_" + k: np.abs(ed[k] - want[k]).max() for k in K12_TABLES})
            d_ref["%d_%s" % (si, kind)] = {k: float(v) for k, v in d.items()}
        # the codon level: K15's five tables from the exact H, K14's two from the exact cond at both nodes; d_ref from the
        # same contractions (doubles: at most 125 non-negative terms of probabilities) fed the double-precision H and G
        for frame in [f for i, f in COMBOS if i == si]:
            for kind in Q_KINDS:
                Q = codon_q_of(kind, h, frame)
                tag = "%d_%s_%d" % (si, kind, frame)
                with np.errstate(all="ignore"):
                    want, dbl = ceo.tables(Q, tab["cond_edge"], frame), ceo.tables(Q, H, frame)
                d = {}
                for k in K15_TABLES:
                    keep["k15_%s_%s" % (tag, k)] = want[k]
                    d["k15_" + k] = _far(dbl[k], want[k])
                del want, dbl
                for node, slot in (("parent", 0), ("mrca", len(path) - 1)):
                    for k, f in (("codons", nco.contraction), ("change", nco.change)):
                        w14 = f(Q, tab["cond"][slot], frame)
                        keep["k14_%s_%s_%s" % (tag, node, k)] = w14
                        d["k14_%s_%s" % (node, k)] = _far(f(Q, G[node], frame), w14)
                d_ref[tag] = d
    keep["d_ref"] = json.dumps(d_ref)
    keep["seconds"] = time.perf_counter() - t0
    return row[0], keep


def one_rescale_of_row(args):
    """The mutation check of the joins at K15b's level, on the CPU: codon_edge_oracle.cond_edges fed a `pre` with ONE rescaling
    per node (upward_until(until=False): the arithmetic before lh_treepass.h rescaled until above 2^-256), for the family's
    first seed tip.  Returns (row, distance of that H from the exact cond_edge, d_ref of the rescale-until H): a row whose
    first distance is within max(FLOOR, 8 d_ref) proves nothing for K15."""
    from tests import ancestral_marginal_oracle as amo
    from tests import codon_edge_oracle as ceo
    family, row = args
    s = _row_setup(family, row)
    tip = SEEDS[family][0]
    path = amo.seed_path(s["children"], s["root"], s["T"], tip)
    exact = s["lin"].tables(path, tip)["cond_edge"]
    once = double_pre(np.asarray(s["children"]).ravel(), s["root"], s["T"], s["msa"], s["sample"]["pi"], s["P"], until=False)
    far = []
    for pre in (once, s["pre"]):
        with np.errstate(all="ignore"):
            H = ceo.cond_edges(s["children"], s["root"], s["brlen"], s["T"], s["msa"], s["sample"]["er"], s["sample"]["pi"],
                               s["rates"], path, tip, pre=pre)
        far.append(_far(H, exact))
    return row[0], far[0], far[1]


def cpu_side(out_dir, jobs=1):
    """DIR/lineage_<row>.npz for every row of both families; returns {row: (d_ref dict, seconds)}."""
    os.makedirs(out_dir, exist_ok=True)
    todo = [(family, row) for family in SEEDS for row in rows_of(family)]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            done = pool.map(exact_of_row, todo)
    else:
        done = [exact_of_row(t) for t in todo]
    out = {}
    for name, keep in done:
        np.savez(os.path.join(out_dir, "lineage_%s.npz" % name), **keep)
        out[name] = (json.loads(keep["d_ref"]), float(keep["seconds"]))
    return out


def one_rescale_rows(jobs=1):
    """one_rescale_of_row for the two rows whose joins need more than one rescaling: [(row, distance, d_ref)]."""
    todo = [(r[1], r) for r in rows_of("cmp180") if r[2] in ("compound_lossy", "compound_zeroed")]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            return pool.map(one_rescale_of_row, todo)
    return [one_rescale_of_row(t) for t in todo]


def exact_tables(x, si):
    """ExactLineage.tables of seed tip number si, spread from the distinct columns back over the sites."""
    po = x["pattern_of"]
    return dict(cond=x["cond_%d" % si][:, po], cond_edge=x["cond_edge_%d" % si][:, po], rate=x["rate_%d" % si][po])


def run_gpu(out_dir, family, workdir):
    import linearham_amd
    from linearham_amd import capi
    from tests import cadence_cases as cc
    from tests import desc_builder as db
    from tests import exact_lineage_oracle as xl
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    h = cc.load_family(family, workdir)
    rows = rows_of(family)
    R = cc.FAMILIES[family]["R"]
    samples = [cc.sample_of(r)[0] for r in rows]
    sched = [cc.schedule(h, s) for s in samples]
    T, depth = sched[0][0], max(s[5] for s in sched)
    ops, brl = np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched])
    er, pi = [s["er"] for s in samples], [s["pi"] for s in samples]
    ref = [np.load(os.path.join(out_dir, "lineage_%s.npz" % r[0])) for r in rows]
    rates = np.stack([x["rates"] for x in ref])
    d_ref = [json.loads(str(x["d_ref"])) for x in ref]
    n = len(rows)
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    failures, figures = [], []

    def note(cond, text):
        if not cond:
            failures.append(text)

    for si, tip in enumerate(SEEDS[family]):
        paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
        padded = capi.pad_paths(paths)
        tabs = [exact_tables(x, si) for x in ref]
        for kind in Q_KINDS:
            q = np.tile(q_of(kind, h, 1), (n, 1, 1))               # (the rows d_ref was measured with)
            marg, rp = fam.asr_marginals_batch(T, depth, ops, brl, er, pi, rates, q, padded)
            full = fam.asr_edges_batch(T, depth, ops, brl, er, pi, rates, q, padded, tip, want=K12_TABLES)
            lean = fam.asr_edges_batch(T, depth, ops, brl, er, pi, rates, q, padded, tip, want=LEAN_TABLES)
            if si == 0:             # every row alone: the same bits as in the batch
                for i, r in enumerate(rows):
                    m1, r1 = fam.asr_marginals_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                                     q[i:i + 1], capi.pad_paths(paths[i:i + 1]))
                    e1 = fam.asr_edges_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                             q[i:i + 1], capi.pad_paths(paths[i:i + 1]), tip, want=K12_TABLES)
                    l1 = fam.asr_edges_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                             q[i:i + 1], capi.pad_paths(paths[i:i + 1]), tip, want=LEAN_TABLES)
                    P = len(paths[i])

                    def load(v):            # a batch pads the paths to its longest: slots [0, P) and the naive edge's
                        return np.concatenate([v[:P], v[-1:]])
                    same = [np.array_equal(m1[0], marg[i, :P]), np.array_equal(r1[0], rp[i]),
                            np.array_equal(e1["edge"][0], full["edge"][i, :P])]
                    for alone, batch in ((e1, full), (l1, lean)):
                        same += [np.array_equal(alone[k][0], batch[k][i]) for k in ("naive_edge", "chain_counts", "rate_post")]
                        same.append(np.array_equal(alone["edge_load"][0], load(batch["edge_load"][i])))
                    note(all(same), "%s tip %d %s: not bit-identical alone and in the batch: %s" % (r[0], tip, kind, same))
            for i, r in enumerate(rows):
                P = len(paths[i])
                want = xl.mix(tabs[i], q[i])
                dr = d_ref[i]["%d_%s" % (si, kind)]
                where = "%s tip %d %s" % (r[0], tip, kind)
                got = {"k11_marg": marg[i, :P], "k11_rate_post": rp[i]}
                for key in K12_TABLES:
                    v = full[key][i]
                    got["k12_" + key] = v[:P] if key == "edge" else np.concatenate([v[:P], v[-1:]]) if key == "edge_load" else v
                for key in LEAN_TABLES:
                    v = lean[key][i]
                    got["k12lean_" + key] = np.concatenate([v[:P], v[-1:]]) if key == "edge_load" else v
                fig = dict(row=r[0], cls=r[2], tip=tip, q=kind, path=P)
                for key, v in got.items():
                    base = key.split("_", 1)[1]
                    ref_key = key if key in dr else "k12_" + base
                    bound = max(FLOOR, 8.0 * dr[ref_key])
                    with np.errstate(invalid="ignore"):
                        d = float(np.abs(v - want[base]).max()) if np.isfinite(v).all() else float("inf")
                    fig[key] = d
                    fig["ref_" + ref_key] = dr[ref_key]
                    note(d <= bound, "%s: %s off the exact reference by %.3g (bound %.3g, d_ref %.3g)" % (where, key, d, bound, dr[ref_key]))
                # distributions
                sums = [np.abs(marg[i, :P].sum(axis=-1) - 1).max(), np.abs(rp[i].sum(axis=-1) - 1).max(),
                        np.abs(full["rate_post"][i].sum(axis=-1) - 1).max(), np.abs(lean["rate_post"][i].sum(axis=-1) - 1).max()]
                fig["sum_to_one"] = float(np.nanmax(sums)) if np.isfinite(sums).all() else float("inf")
                note(fig["sum_to_one"] <= 1e-12, "%s: marginals or rate posteriors do not sum to 1: %s" % (where, sums))
                note(not marg[i, P:].any() and not full["edge"][i, P:].any(), "%s: the padding slots are not 0" % where)
                # K12's four margin identities against K11's device output
                e, ne, m = full["edge"][i, :P], full["naive_edge"][i], marg[i, :P]
                ident = [np.abs(e.sum(axis=-1) - m).max(), np.abs(e[1:].sum(axis=-2) - m[:-1]).max() if P > 1 else 0.0,
                         np.abs(ne.sum(axis=-1) - q[i]).max(), np.abs(ne.sum(axis=-2) - m[P - 1]).max()]
                fig["identities"] = float(max(ident)) if np.isfinite(ident).all() else float("inf")
                note(fig["identities"] <= 1e-12, "%s: K12's margins against K11: %s" % (where, ident))
                figures.append(fig)
    # ---- K13b's conditional tables: lh_eval_ancestral_candidates_batch's `cond` at both nodes, on the family as the host
    # library reads it, against the exact tables and against five one-hot calls of lh_asr_marginals_batch.  (Default mode:
    # the entry point refuses extended-range handles.  The deep columns' emissions are 0 there and the log-likelihood is
    # not finite; `cond` does not depend on either -- it is built from K1's unmixed planes and their counts.)
    from linearham_amd import host
    from tests.ancestral_cases import write_table
    yaml_path, pdir = cc.write_family_files(family, workdir, h)
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    tsv = os.path.join(workdir, "rows.tsv")
    write_table(tsv, samples[:1])
    hfam = hh.flatten_tsv(tsv, 1)["family"]
    L = h.msa.shape[1]
    hip.set_ancestral_candidates(hfam, np.full((1, L), 4, dtype=np.uint8))
    alpha = np.array([s["alpha"] for s in samples])
    cond_figures = []
    for si, tip in enumerate(SEEDS[family]):
        paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
        padded = capi.pad_paths(paths)
        tabs = [exact_tables(x, si) for x in ref]
        k11 = []
        for b in range(5):
            marg, _ = fam.asr_marginals_batch(T, depth, ops, brl, er, pi, rates, np.tile(np.eye(5)[b], (n, L, 1)), padded,
                                              want=("marg",))
            k11.append(marg)
        for node, name in ((capi.NODE_PARENT, "parent"), (capi.NODE_MRCA, "mrca")):
            res = hip.eval_ancestral_candidates_batch(hfam, T, depth, ops, brl, np.array(er), np.array(pi), alpha, R, padded, node,
                                                      want=("cond",))
            for i, r in enumerate(rows):
                slot = 0 if name == "parent" else len(paths[i]) - 1
                got = res["cond"][i]
                dr = d_ref[i]["%d_cond" % si]["k13_" + name]
                bound = max(FLOOR, 8.0 * dr)
                where = "%s tip %d %s" % (r[0], tip, name)
                ok = bool(np.isfinite(got).all())
                d = float(np.abs(got - tabs[i]["cond"][slot]).max()) if ok else float("inf")
                d11 = float(max(np.abs(got[:, b] - k11[b][i, slot]).max() for b in range(5))) if ok else float("inf")
                s1 = float(np.abs(got.sum(axis=-1) - 1).max()) if ok else float("inf")
                note(d <= bound, "%s: k13_cond off the exact reference by %.3g (bound %.3g, d_ref %.3g)" % (where, d, bound, dr))
                note(d11 <= 1e-12, "%s: K13's cond against five one-hot K11 calls: %.3g" % (where, d11))
                note(s1 <= 1e-12, "%s: K13's cond rows do not sum to 1: %.3g" % (where, s1))
                cond_figures.append(dict(row=r[0], cls=r[2], tip=tip, node=name, k13_cond=d, ref_k13=dr, k13_vs_k11=d11, sum_to_one=s1))
                if si == 0:         # the row alone: the same bits as in the batch
                    one = hip.eval_ancestral_candidates_batch(hfam, T, depth, ops[i:i + 1], brl[i:i + 1], np.array(er[i:i + 1]),
                                                              np.array(pi[i:i + 1]), alpha[i:i + 1], R,
                                                              capi.pad_paths(paths[i:i + 1]), node, want=("cond",))
                    note(np.array_equal(one["cond"][0], got), "%s: K13's cond not bit-identical alone and in the batch" % where)
    fam.close()
    print(json.dumps({"failures": failures, "figures": figures, "cond_figures": cond_figures, "rows": n}))


def run_gpu_codons(out_dir, family, workdir):
    """The codons child: K15 (lh_asr_codon_edges_batch with cond_edge: K15b's H and the five tables) and K14
    (lh_asr_node_codons_batch at both nodes) on every row of the family in one batch, COMBOS x Q_KINDS, on the family as the
    host library reads it, against the exact tables of the row's npz; for cmp180 the evaluation forms as well."""
    import linearham_amd
    from linearham_amd import capi, host
    from tests import cadence_cases as cc
    from tests import codon_edges_cases as cec
    from tests.ancestral_cases import write_table
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    h = cc.load_family(family, workdir)
    rows = rows_of(family)
    R = cc.FAMILIES[family]["R"]
    samples = [cc.sample_of(r)[0] for r in rows]
    sched = [cc.schedule(h, s) for s in samples]
    T, depth = sched[0][0], max(s[5] for s in sched)
    ops, brl = np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched])
    er, pi = np.array([s["er"] for s in samples]), np.array([s["pi"] for s in samples])
    alpha = np.array([s["alpha"] for s in samples])
    ref = [np.load(os.path.join(out_dir, "lineage_%s.npz" % r[0])) for r in rows]
    rates = np.stack([x["rates"] for x in ref])
    d_ref = [json.loads(str(x["d_ref"])) for x in ref]
    n, L = len(rows), h.msa.shape[1]
    yaml_path, pdir = cc.write_family_files(family, workdir, h)
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    tsv = os.path.join(workdir, "rows.tsv")
    write_table(tsv, samples[:1])
    hfam = hh.flatten_tsv(tsv, 1)["family"]
    fam = capi.Family.borrow(hfam, hip)
    hip.set_ancestral_candidates(hfam, np.full((1, L), 4, dtype=np.uint8))
    nodes = (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA))
    failures, figures, longest = [], [], 0

    def note(cond, text):
        if not cond:
            failures.append(text)

    def tree(i=None):
        sl = slice(None) if i is None else slice(i, i + 1)
        return T, depth, ops[sl], brl[sl], er[sl], pi[sl]

    def slots(v, P):               # a batch pads the chains to its longest: slots [0, P) and the naive edge's
        return np.concatenate([v[:P], v[-1:]])

    def k15(i, Q, padded, tip):
        sl = slice(None) if i is None else slice(i, i + 1)
        return fam.asr_codon_edges_batch(*tree(i), rates[sl], Q[sl], padded, tip, want=K15_TABLES + ("cond_edge",), n_sites=L)

    def k14(i, Q, padded, node):
        sl = slice(None) if i is None else slice(i, i + 1)
        return dict(zip(K14_TABLES, fam.asr_node_codons_batch(*tree(i), rates[sl], Q[sl], padded, node)))

    for si, frame in COMBOS:
        tip = SEEDS[family][si]
        paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
        padded = capi.pad_paths(paths)
        longest = max(longest, padded.shape[1])
        tabs = [exact_tables(x, si) for x in ref]
        lay = hip.set_codons(hfam, frame)
        assert lay["n_codons"] == (L - frame) // 3, lay["n_codons"]
        if frame == 0:
            # what the older kernels give on the same handle: K13b's cond at both nodes, K12's edge for the site-level q
            k13 = {name: hip.eval_ancestral_candidates_batch(hfam, *tree(), alpha, R, padded, node, want=("cond",))["cond"]
                   for name, node in nodes}
            q12 = np.tile(q_of("dirichlet", h, 1), (n, 1, 1))
            k12 = fam.asr_edges_batch(*tree(), rates, q12, padded, tip, want=("edge",))["edge"]
        for kind in Q_KINDS:
            tag = "%d_%s_%d" % (si, kind, frame)
            Q = np.tile(codon_q_of(kind, h, frame), (n, 1, 1))
            res = k15(None, Q, padded, tip)
            at = {name: k14(None, Q, padded, node) for name, node in nodes}
            try:
                cec.rules(res, paths)
            except AssertionError as e:
                import traceback
                note(False, "tip %d %s frame %d: K15's sum rules: %s" % (tip, kind, frame, traceback.extract_tb(e.__traceback__)[-1].line))
            for i, r in enumerate(rows):
                P = len(paths[i])
                where = "%s tip %d %s frame %d" % (r[0], tip, kind, frame)
                fig = dict(row=r[0], cls=r[2], tip=tip, q=kind, frame=frame, path=P)
                ce = res["cond_edge"][i, :P]
                got = {"k15b_cond_edge": (ce, tabs[i]["cond_edge"], d_ref[i]["%d_cond" % si]["k15_cond_edge"])}
                for k in K15_TABLES:
                    v = res[k][i]
                    got["k15_" + k] = (slots(v, P) if k in ("edge_change", "edge_load") else v, ref[i]["k15_%s_%s" % (tag, k)],
                                       d_ref[i][tag]["k15_" + k])
                for name, _ in nodes:
                    for k in K14_TABLES:
                        got["k14_%s_%s" % (name, k)] = (at[name][k][i], ref[i]["k14_%s_%s_%s" % (tag, name, k)],
                                                        d_ref[i][tag]["k14_%s_%s" % (name, k)])
                for key, (v, want, dr) in got.items():
                    d, bound = _far(v, want), max(FLOOR, 8.0 * dr)
                    fig[key], fig["ref_" + key] = d, dr
                    note(d <= bound, "%s: %s off the exact reference by %.3g (bound %.3g, d_ref %.3g)" % (where, key, d, bound, dr))
                # rules that need no oracle
                sums = [_far(at[name][k][i].sum(axis=-1), 1.0) for name, _ in nodes for k in K14_TABLES]
                fig["sum_to_one"] = max(sums)
                note(fig["sum_to_one"] <= 1e-12, "%s: K14's codons or change do not sum to 1: %s" % (where, sums))
                note(not res["edge_change"][i, P:-1].any() and not res["edge_load"][i, P:-1].any(), "%s: the padding slots are not 0" % where)
                # device identities
                ident = {"k15_vs_k14": _far(res["edge_change"][i, -1], at["mrca"]["change"][i][:, :3])}
                if frame == 0 and kind == Q_KINDS[0]:
                    ident["k15b_vs_k13"] = max(_far(ce[0].sum(axis=-1), k13["parent"][i]), _far(ce[P - 1].sum(axis=-1), k13["mrca"][i]))
                    ident["k15b_vs_k12"] = _far(np.einsum("lb,slbac->slac", q12[i], ce), k12[i, :P])
                fig.update(ident)
                note(max(ident.values()) <= 1e-12, "%s: identities against K12, K13 and K14 on the device: %s" % (where, ident))
                figures.append(fig)
                if si == 0:         # the row alone: the batch's bits on its own slots
                    own = capi.pad_paths(paths[i:i + 1])
                    one = k15(i, Q, own, tip)
                    same = [np.array_equal(one[k][0], res[k][i]) for k in K15_TABLES[:3]]
                    same += [np.array_equal(one[k][0], slots(res[k][i], P)) for k in K15_TABLES[3:]]
                    same.append(np.array_equal(one["cond_edge"][0], ce))
                    for name, node in nodes:
                        a1 = k14(i, Q, own, node)
                        same += [np.array_equal(a1[k][0], at[name][k][i]) for k in K14_TABLES]
                    note(all(same), "%s: not bit-identical alone and in the batch: %s" % (where, same))
    note(longest > 100, "the longest chain is %d: the slot loop is not stressed" % longest)
    out = {"failures": failures, "figures": figures, "rows": n, "longest_chain": int(longest)}
    if family == "cmp180":
        out["eval"] = eval_forms(hip, hh, hfam, fam, rows, sched, (T, depth, ops, brl, er, pi, alpha, R), failures)
    print(json.dumps(out))


def eval_forms(hip, hh, hfam, fam, rows, sched, args, failures):
    """The evaluation forms (lh_eval_codon_edges_batch, lh_eval_node_codons_batch) on cmp180's control row batched with its
    three deep rows, seed tip 44, frame 0, default mode: the deep rows' log-likelihoods are not finite there, so they hold NaN
    and carry no weight; the control row keeps the bits it has alone, at a chain of 113, and they are the given-rates forms'
    on the evaluation's own rates and the host-expanded K9 table."""
    from linearham_amd import capi
    from linearham_amd import posterior as lp
    T, depth, ops, brl, er, pi, alpha, R = args
    tip, n = SEEDS["cmp180"][0], len(rows)
    assert rows[0][2] == "compound_control"
    paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
    lay = hip.set_codons(hfam, 0)
    nodes = (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA))
    w15 = tuple("weighted_" + k for k in K15_TABLES[:3])
    w14 = tuple("weighted_" + k for k in K14_TABLES)

    def note(cond, text):
        if not cond:
            failures.append("evaluation forms: " + text)

    def run(sl):
        a = (T, depth, ops[sl], brl[sl], er[sl], pi[sl], alpha[sl], R)
        padded = capi.pad_paths(paths[sl])
        e = hip.eval_codon_edges_batch(hfam, *a, padded, tip, want=("loglik",) + K15_TABLES + w15 + ("weight_stats",))
        nd = {name: hip.eval_node_codons_batch(hfam, *a, padded, node, want=("loglik",) + K14_TABLES + w14 + ("weight_stats",))
              for name, node in nodes}
        return e, nd
    P = len(paths[0])
    slots = lambda v: np.concatenate([v[:P], v[-1:]])
    batch, alone = run(slice(None)), run(slice(0, 1))
    fig = dict(chain=P, loglik=[float(x) for x in batch[0]["loglik"]])
    calls = [("K15", batch[0], alone[0], K15_TABLES, w15)] + [("K14 " + name, batch[1][name], alone[1][name], K14_TABLES, w14)
                                                             for name, _ in nodes]
    worst = 0.0
    for what, b, a, tables, weighted in calls:
        note(np.isfinite(b["loglik"][0]) and not np.isfinite(b["loglik"][1:]).any(),
             "%s: the control row's log-likelihood is not finite or a deep row's is: %s" % (what, b["loglik"]))
        note(all(np.isnan(b[k][1:]).all() for k in tables), "%s: a deep row holds something other than NaN" % what)
        note(all(np.isfinite(a[k]).all() for k in tables + weighted), "%s: the control row alone is not finite" % what)
        for k in tables:
            own = slots(b[k][0]) if k in ("edge_change", "edge_load") else b[k][0]
            note(np.array_equal(own, a[k][0]), "%s: the control row's %s not bit-identical alone and in the batch" % (what, k))
        for k in weighted + ("weight_stats",):
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(b[k] - a[k]) / np.where(a[k] != 0, np.abs(a[k]), 1.0)
            d = float(rel.max()) if np.isfinite(b[k]).all() else float("inf")
            worst = max(worst, d)
            note(d <= 1e-14, "%s: %s is not the control row's alone: %.3g relative" % (what, k, d))
    fig["weighted_rel"] = worst
    # the given-rates forms on the evaluation's own rates and the host-expanded K9 table
    a1 = (T, depth, ops[:1], brl[:1], er[:1], pi[:1])
    _, ev = fam.eval_batch(*a1, alpha[:1], R, want=("rates",))
    k9 = hip.eval_codons_batch(hfam, *a1, alpha[:1], R, want=("windows", "genes"))
    Q = lp.codon_table(hh.dump(1), k9["windows"][0], k9["genes"][0], lay)[None]
    own = capi.pad_paths(paths[:1])
    given = fam.asr_codon_edges_batch(*a1, ev["rates"], Q, own, tip)
    same = {k: bool(np.array_equal(given[k], alone[0][k])) for k in K15_TABLES}
    for name, node in nodes:
        g14 = dict(zip(K14_TABLES, fam.asr_node_codons_batch(*a1, ev["rates"], Q, own, node)))
        same.update({"%s_%s" % (name, k): bool(np.array_equal(g14[k], alone[1][name][k])) for k in K14_TABLES})
    note(all(same.values()), "the given-rates forms do not have the evaluation's bits: %s" % same)
    fig["given_rates_same"] = same
    return fig


def main(argv):
    import shutil
    import tempfile

    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    if "--cpu" in argv:
        print("exact side per row, and d_ref: the largest distance of the double-precision oracles from the exact reference over the "
              "seed tips, distributions and frames, per table (K13b: k13_*, K15b: k15_cond_edge, K14: k14_*, K15: k15_*)")
        above = False
        for name, (d, sec) in cpu_side(opt("--cpu"), int(opt("--jobs", "1"))).items():
            worst = {}
            for dd in d.values():
                for k, v in dd.items():
                    worst[k] = max(worst.get(k, 0.0), v)
            print("%-16s %.1f s  d_ref %s" % (name, sec, "  ".join("%s %.2g" % kv for kv in worst.items())))
            over = sorted(k for k, v in worst.items() if v > FLOOR / 10)
            if over:
                above = True
                print("%-16s d_ref above 1e-11 (the bound is 8 d_ref wherever that exceeds the floor of 1e-10): %s" % ("", ", ".join(over)))
        if not above:
            print("no d_ref above 1e-11: every row's bound is the floor of 1e-10")
        print("one rescaling per node instead of rescaling until above 2^-256 (upward_until(until=False)), first seed tip: distance "
              "of codon_edge_oracle.cond_edges from the exact cond_edge, and the row's bound max(1e-10, 8 d_ref)")
        for name, far, ref in one_rescale_rows(int(opt("--jobs", "1"))):
            bound = max(FLOOR, 8.0 * ref)
            print("%-16s %.3g  (bound %.3g, d_ref %.2g)%s" % (name, far, bound, ref, "" if far > bound else
                                                               "  WITHIN THE BOUND: the row proves nothing for K15"))
        return 0
    if "--gpu-codons" in argv:
        work = tempfile.mkdtemp(prefix="lh_lineage_cadence_")
        try:
            run_gpu_codons(opt("--gpu-codons"), opt("--family"), work)
        finally:
            shutil.rmtree(work, ignore_errors=True)
        return 0
    work = tempfile.mkdtemp(prefix="lh_lineage_cadence_")
    try:
        run_gpu(opt("--gpu"), opt("--family"), work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
