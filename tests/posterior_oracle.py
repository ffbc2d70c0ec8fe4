"""Test-side restatement of the naive-sequence posterior (K5) on the oracle HMM's dense matrices.

Three independent forms of the same quantity, all built from oracle.linearham_oracle.HMM's dense transition,
emission and forward members (the oracle itself is imported, not changed):
  forward_backward  classical alpha * beta over the whole V | V-D rows | D | D-J rows | J chain, own scaling;
  smoothing         forward filtering / backward smoothing over the oracle's forward arrays (what K5 computes);
  brute_force       every non-zero-probability state path, enumerated;
and the state -> site / gene mapping (linearham_amd.posterior on the oracle's state space)."""
import math

import numpy as np

from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc

REGION_FIELDS = ("ggene_ranges", "site_inds", "naive_bases")


def state_space(h):
    """The oracle's state space in the host library's dump spelling (what linearham_amd.posterior reads)."""
    ss = {"locus": h.locus, "flexbounds": {k: list(v) for k, v in h.flexbounds.items()}, "msa": h.msa.tolist()}
    regions = ["vgerm", "vd_junction", "jgerm"] + (["dgerm", "dj_junction"] if h.locus == "igh" else [])
    for r in regions:
        R = getattr(h, r)
        for f in REGION_FIELDS:
            ss[r + "_" + f] = getattr(R, f)
    return ss


def _chain(h):
    """The HMM as a list of steps: ("germ", name, emission e[g]) for germline regions and ("junc", name, E[W][S]) for
    junctions, with the transitions between consecutive steps (T[from][to]).  The V region's 'emission' is its initial
    forward vector; the oracle's emissions carry their ScaleMatrix counts, returned as a total."""
    igh = h.locus == "igh"
    nv = len(h.vgerm.state_strs)
    v0 = np.zeros(nv)
    for i, gname in enumerate(sorted(h.vgerm.ggene_ranges)):
        rs, re_ = h.vgerm.ggene_ranges[gname]
        gg = h.ggenes[gname]
        gis = h.vgerm.germ_inds[rs]
        v = gg.gene_prob
        v *= h.vpadding_transition[i]
        v *= h.vpadding_emission[i]
        v *= np.prod(gg.transition[gis:gis + (re_ - rs - 1)])
        v *= h.vgerm_emission[i]
        v0[i] = v
    eJ = h.jgerm_emission * h.jpadding_transition * h.jpadding_emission
    steps = [("germ", "vgerm", v0), ("junc", "vd_junction", h.vd_junction_emission)]
    trans = [h.vgerm_vd_junction_transition, h.vd_junction_dgerm_transition]
    if igh:
        steps += [("germ", "dgerm", h.dgerm_emission.copy()), ("junc", "dj_junction", h.dj_junction_emission),
                  ("germ", "jgerm", eJ)]
        trans += [h.dgerm_dj_junction_transition, h.dj_junction_jgerm_transition]
    else:
        steps += [("germ", "jgerm", eJ)]
    return steps, trans, h.vd_junction_transition, (h.dj_junction_transition if igh else None)


def emission_count(h):
    """Sum of the regions' emission ScaleMatrix counts (read BEFORE the forward pass adds the rows' counts)."""
    return h.vgerm_scaler_count + (h.dgerm_scaler_count if h.locus == "igh" else 0) + h.jgerm_scaler_count


def _rows(steps, trans, Tvd, Tdj):
    """The chain unrolled into per-row (emission vector, transition into it) pairs, with region tags."""
    rows = []
    prevT = None
    for k, (kind, name, e) in enumerate(steps):
        if kind == "germ":
            rows.append((name, None, e, prevT))
            prevT = trans[k] if k < len(trans) else None
        else:
            Tjj = Tvd if name == "vd_junction" else Tdj
            for i in range(e.shape[0]):
                rows.append((name, i, e[i], prevT if i == 0 else Tjj))
            prevT = trans[k]
    return rows


def forward_backward(h, ec=0):
    """Dense alpha-beta with its own per-row normalisation.  Returns ({region: posterior}, loglik), the log-likelihood
    from sum_k alpha_i(k) beta_i(k) on every row (they must agree), corrected by the emissions' counts ec."""
    rows = _rows(*_chain(h))
    n = len(rows)
    alpha, ca = [None] * n, [0.0] * n
    for t, (_, _, e, T) in enumerate(rows):
        a = e.copy() if T is None else (alpha[t - 1] @ T) * e
        s = a.sum()
        alpha[t] = a / s
        ca[t] = (ca[t - 1] if t else 0.0) + math.log(s)
    beta, cb = [None] * n, [0.0] * n
    beta[-1] = np.ones_like(rows[-1][2])
    for t in range(n - 2, -1, -1):
        _, _, e1, T1 = rows[t + 1]
        b = T1 @ (e1 * beta[t + 1])
        s = b.sum()
        beta[t] = b / s
        cb[t] = cb[t + 1] + math.log(s)
    post = {}
    lls = []
    for t, (name, i, _, _) in enumerate(rows):
        ab = alpha[t] * beta[t]
        z = ab.sum()
        lls.append(math.log(z) + ca[t] + cb[t] - ec * orc.LOG_SCALE_FACTOR)
        p = ab / z
        if i is None:
            post[name] = p
        else:
            post.setdefault(name, []).append(p)
    return {k: np.array(v) for k, v in post.items()}, lls


def smoothing(h, forward=None):
    """Forward filtering / backward smoothing over forward arrays (the oracle's own, or `forward` = {vgerm_forward,
    vd_junction_forward, ...} from elsewhere, e.g. the device), with the oracle's dense transitions."""
    igh = h.locus == "igh"
    fw = forward if forward is not None else {k: getattr(h, k) for k in (
        "vgerm_forward", "vd_junction_forward", "jgerm_forward") + (("dgerm_forward", "dj_junction_forward") if igh else ())}

    def step(F, T, p_next):
        Z = F @ T
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(p_next != 0, p_next / np.where(p_next != 0, Z, 1.0), 0.0)
        return F * (T @ rho)

    def junction(F, Tjj, Tjg, p_right):
        W = F.shape[0]
        out = np.zeros_like(F)
        out[W - 1] = step(F[W - 1], Tjg, p_right)
        for i in range(W - 2, -1, -1):
            out[i] = step(F[i], Tjj, out[i + 1])
        return out

    fJ = np.asarray(fw["jgerm_forward"], dtype=np.float64)
    post = {"jgerm": fJ / fJ.sum()}
    if igh:
        post["dj_junction"] = junction(np.asarray(fw["dj_junction_forward"]), h.dj_junction_transition,
                                       h.dj_junction_jgerm_transition, post["jgerm"])
        post["dgerm"] = step(np.asarray(fw["dgerm_forward"]), h.dgerm_dj_junction_transition, post["dj_junction"][0])
        right = post["dgerm"]
    else:
        right = post["jgerm"]
    post["vd_junction"] = junction(np.asarray(fw["vd_junction_forward"]), h.vd_junction_transition,
                                   h.vd_junction_dgerm_transition, right)
    post["vgerm"] = step(np.asarray(fw["vgerm_forward"]), h.vgerm_vd_junction_transition, post["vd_junction"][0])
    return post


def brute_force(h):
    """Every state path with non-zero probability, enumerated: {region: posterior} and the number of paths."""
    rows = _rows(*_chain(h))
    n = len(rows)
    post = [np.zeros_like(r[2]) for r in rows]
    paths = []

    def rec(t, k, w, path):
        if t == n - 1:
            paths.append((w, path))
            return
        _, _, e1, T1 = rows[t + 1]
        for k2 in np.nonzero(T1[k] * e1)[0]:
            rec(t + 1, k2, w * T1[k, k2] * e1[k2], path + [k2])

    e0 = rows[0][2]
    for k in np.nonzero(e0)[0]:
        rec(0, k, e0[k], [k])
    total = sum(w for w, _ in paths)
    for w, path in paths:
        for t, k in enumerate(path):
            post[t][k] += w / total
    out = {}
    for t, (name, i, _, _) in enumerate(rows):
        if i is None:
            out[name] = post[t]
        else:
            out.setdefault(name, []).append(post[t])
    return {k: np.array(v) for k, v in out.items()}, len(paths)


def to_compact(h, dense):
    """{region: dense posterior} -> the compact vector K5 writes (linearham_amd.posterior's layout)."""
    ss = state_space(h)
    blocks, size = lp.layout(ss)
    out = np.zeros(size)
    for kind, region, off, info in blocks:
        if kind == "germ":
            out[off:off + len(info)] = dense[region]
        else:
            W, st, d = info["n_rows"], info["stride"], info["dense"]
            for i in range(W):
                ok = d[i] >= 0
                out[off + i * st:off + (i + 1) * st][ok] = dense[region][i][d[i][ok]]
    return out


def site_base(h, dense):
    ss = state_space(h)
    return lp.site_base(ss, to_compact(h, dense))


def gene_posteriors(h, dense):
    ss = state_space(h)
    return lp.gene_posteriors(ss, to_compact(h, dense))


def weighted_marginals(lh_loglik, rb_loglik, per_row, burnin_frac):
    """numpy restatement of scripts/run_bootstrap_asr_ess.R:23-31 applied to exact per-row quantities: drop the first
    floor(b N) rows (tail(n = -(b N))), weight by exp(LHLogLikelihood - RBLogLikelihood) normalised over the kept rows
    (rows with a non-finite weight dropped), return (weighted mean of per_row, Kish ESS)."""
    N = len(lh_loglik)
    first = int(math.floor(burnin_frac * N))
    lw = np.asarray(lh_loglik[first:]) - np.asarray(rb_loglik[first:])
    ok = np.isfinite(lw)
    w = np.zeros_like(lw)
    w[ok] = np.exp(lw[ok] - lw[ok].max())
    w = w / w.sum()
    x = np.asarray(per_row[first:])
    mean = np.tensordot(w[ok], x[ok], axes=1)
    return mean, 1.0 / np.sum(w ** 2)
