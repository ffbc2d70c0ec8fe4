"""TEST INFRASTRUCTURE (CPU only): the most probable state path (K8) restated on the oracle HMM's dense matrices.

Everything is built on tests/posterior_oracle._rows(*_chain(h)): the chain V | V-D rows | D | D-J rows | J unrolled into
per-row (emission vector, dense transition into it) pairs.  All arithmetic is in log space, so nothing here shares the
device's power-of-two rescaling:
  viterbi            dense max-product sweep with back-pointers: path, log P(data, path | tree), margin;
  path_log_joint     log P(data, path | tree) of a given path;
  log_path_prior     the same with every emission 1 (the path's HMM prior);
  enumerate_paths /  every state path of non-zero probability and the best of them;
  brute_force_max
  to_states /        rows order <-> K4's states layout (J gene | D-J rows | D gene | V-D rows | V gene);
  from_states
  sampler_tables     lh_sampler_junction tables of an oracle object (what the C++ host builds in HMM::BuildSamplerJunction),
                     for families that exist as oracle objects only.
`ec` is posterior_oracle.emission_count(h), read BEFORE the oracle's forward pass (which adds the rows' counts to it)."""
import math

import numpy as np

from oracle import linearham_oracle as orc
from tests import posterior_oracle as po

NEG = -math.inf


def _log(a):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(a, dtype=float))


def chain_rows(h):
    return po._rows(*po._chain(h))


def viterbi(h, ec=0):
    """Dense log-space Viterbi.  Returns dict(path = state per row, log_path, margin): margin is the smallest gap between
    the best and the runner-up at any step on the path (among the predecessors of the path's state) and at the end (among
    the last row's states); inf where there is no runner-up of positive probability."""
    rows = chain_rows(h)
    n = len(rows)
    delta, back, gaps = [None] * n, [None] * n, [None] * n
    delta[0] = _log(rows[0][2])
    logT = {}                                              # (the junction's row-to-row matrix recurs on every row)
    for t in range(1, n):
        _, _, e, T = rows[t]
        if id(T) not in logT:
            logT[id(T)] = _log(T)
        cand = delta[t - 1][:, None] + logT[id(T)]         # [from][to]
        cols = np.arange(cand.shape[1])
        back[t] = np.argmax(cand, axis=0)                  # (the lowest index among equals)
        best = cand[back[t], cols]
        if cand.shape[0] > 1:
            cand[back[t], cols] = NEG
            second = cand.max(axis=0)
            with np.errstate(invalid="ignore"):
                gaps[t] = np.where(np.isfinite(second), best - second, math.inf)
        else:
            gaps[t] = np.full(cand.shape[1], math.inf)
        delta[t] = best + _log(e)
    last = delta[-1]
    k = int(np.argmax(last))
    srt = np.sort(last)
    margin = srt[-1] - srt[-2] if len(srt) > 1 and np.isfinite(srt[-2]) else math.inf
    path = [k]
    for t in range(n - 1, 0, -1):
        margin = min(margin, float(gaps[t][k]))
        k = int(back[t][k])
        path.append(k)
    path.reverse()
    return dict(path=path, log_path=float(last[path[-1]]) - ec * orc.LOG_SCALE_FACTOR, margin=float(margin))


def path_log_joint(h, path, ec=0, rows=None):
    rows = rows if rows is not None else chain_rows(h)
    assert len(path) == len(rows)
    v = 0.0
    for t, (_, _, e, T) in enumerate(rows):
        if t:
            v += float(_log(T[path[t - 1], path[t]]))
        v += float(_log(e[path[t]]))
    return v - ec * orc.LOG_SCALE_FACTOR


def prior_rows(h):
    """chain_rows(h) with every emission 1: the germline 'emissions' keep the factors that are not emissions (gene
    probability, padding transition, in-region transitions of the V genes; the J padding transition)."""
    rows = chain_rows(h)
    nv = len(h.vgerm.state_strs)
    v0 = np.zeros(nv)
    for i, gname in enumerate(sorted(h.vgerm.ggene_ranges)):
        rs, re_ = h.vgerm.ggene_ranges[gname]
        gg = h.ggenes[gname]
        gis = h.vgerm.germ_inds[rs]
        v0[i] = gg.gene_prob * h.vpadding_transition[i] * np.prod(gg.transition[gis:gis + (re_ - rs - 1)])
    out = []
    for t, (name, i, e, T) in enumerate(rows):
        if t == 0:
            one = v0
        elif t == len(rows) - 1:
            one = np.asarray(h.jpadding_transition, dtype=float).copy()
        else:
            one = np.ones_like(np.asarray(e, dtype=float))
        out.append((name, i, one, T))
    return out


def log_path_prior(h, path):
    """log P_HMM(path): the path's weight with every emission equal to 1."""
    return path_log_joint(h, path, 0, prior_rows(h))


def is_path(h, path):
    return np.isfinite(log_path_prior(h, path))


def enumerate_paths(h, ec=0):
    """[(log P(data, path | tree), path)] of every state path of non-zero probability, in depth-first order."""
    rows = chain_rows(h)
    n = len(rows)
    out = []

    def rec(t, k, w, path):
        if t == n - 1:
            out.append((w - ec * orc.LOG_SCALE_FACTOR, path))
            return
        _, _, e1, T1 = rows[t + 1]
        for k2 in np.nonzero(T1[k] * e1)[0]:
            rec(t + 1, int(k2), w + math.log(T1[k, k2]) + math.log(e1[k2]), path + [int(k2)])

    e0 = rows[0][2]
    for k in np.nonzero(e0)[0]:
        rec(0, int(k), math.log(e0[k]), [int(k)])
    return out


def brute_force_max(h, ec=0):
    """(largest log P(data, path | tree), its path, number of paths) over all enumerated paths."""
    paths = enumerate_paths(h, ec)
    w, p = max(paths, key=lambda x: x[0])
    return w, p, len(paths)


def _widths(h):
    rows = chain_rows(h)
    w_vd = sum(1 for r in rows if r[0] == "vd_junction")
    w_dj = sum(1 for r in rows if r[0] == "dj_junction")
    return w_vd, w_dj


def to_states(h, path):
    """rows order (V gene, V-D rows, [D gene, D-J rows,] J gene) -> K4's layout."""
    w_vd, w_dj = _widths(h)
    p = list(path)
    if h.locus == "igh":
        v, vd, d, dj, j = p[0], p[1:1 + w_vd], p[1 + w_vd], p[2 + w_vd:2 + w_vd + w_dj], p[-1]
        return np.array([j] + dj + [d] + vd + [v], dtype=np.int32)
    v, vd, j = p[0], p[1:1 + w_vd], p[-1]
    return np.array([j] + vd + [v], dtype=np.int32)


def from_states(h, states):
    """K4's layout -> rows order."""
    w_vd, w_dj = _widths(h)
    s = [int(x) for x in states]
    if h.locus == "igh":
        j, dj, d, vd, v = s[0], s[1:1 + w_dj], s[1 + w_dj], s[2 + w_dj:2 + w_dj + w_vd], s[-1]
        return [v] + vd + [d] + dj + [j]
    j, vd, v = s[0], s[1:1 + w_vd], s[-1]
    return [v] + vd + [j]


def set_emissions(h, em):
    """Puts the per-column emissions `em` on an oracle object (as tests/k2_scaling_cases.oracle_eval does) and returns
    the germline regions' ScaleMatrix count `ec`."""
    h.vgerm_scaler_count = h.dgerm_scaler_count = h.jgerm_scaler_count = 0
    h.xmsa_emission = np.array(em, dtype=float)
    with np.errstate(all="ignore"):
        h._initialize_emission()
    return po.emission_count(h)


def _sampler_junction(h, J, Jx, G_left, G_right, left_fb):
    from linearham_amd.capi import SamplerJunction
    js = left_fb[0]
    W = Jx.shape[0]
    left, right = sorted(G_left.ggene_ranges), sorted(G_right.ggene_ranges)
    nL, nR = len(left), len(right)
    t = dict(left_rows=np.zeros(nL, np.int32), left_dense=np.zeros(nL, np.int32), left_lo=np.zeros((W, nL)),
             left_trans=np.zeros((W, nL)), enter_lo=np.zeros(nL), right_dense=np.zeros(nR, np.int32),
             right_first=np.full(nR, W, np.int32), gene_prob=np.zeros(nR), nti_landing_in=np.zeros((nR, 4)),
             nti_transition=np.zeros((nR, 4, 4)), nti_landing_out=np.zeros((W, nR, 4)), landing_in=np.zeros((W, nR)),
             right_trans=np.zeros((W, nR)), exit_nlo=np.zeros((nR, 4)), exit_trans=np.zeros(nR), exit_li=np.zeros(nR),
             prod=np.ones(nR))
    for l, name in enumerate(left):
        gg = h.ggenes[name]
        _, fre = G_left.ggene_ranges[name]
        p_last = G_left.germ_inds[fre - 1]
        t["enter_lo"][l] = gg.landing_out[p_last]
        rs, re_ = J.ggene_ranges[name]
        cnt = re_ - rs
        t["left_rows"][l], t["left_dense"][l] = cnt, rs
        if cnt > 0:
            t["left_trans"][0, l] = gg.transition[p_last]
        for i in range(cnt):
            p = J.germ_inds[rs + i]
            if i >= 1:
                t["left_trans"][i, l] = gg.transition[p - 1]
            t["left_lo"][i, l] = gg.landing_out[p]
    for r, name in enumerate(right):
        gg = h.ggenes[name]
        rs, re_ = J.ggene_ranges[name]
        t["right_dense"][r] = rs
        t["gene_prob"][r] = gg.gene_prob
        t["nti_landing_in"][r] = gg.nti_landing_in
        t["nti_transition"][r] = gg.nti_transition
        first, last_row = True, -1
        for k in range(rs + 4, re_):
            q = J.germ_inds[k]
            i = J.site_inds[k] - js
            if first:
                t["right_first"][r] = i
            t["nti_landing_out"][i, r] = gg.nti_landing_out[:, q]
            if not first:
                t["right_trans"][i, r] = gg.transition[q - 1]
            t["landing_in"][i, r] = gg.landing_in[q]
            first, last_row = False, i
        trs, tre = G_right.ggene_ranges[name]
        q0 = G_right.germ_inds[trs]
        prod = float(np.prod(gg.transition[q0:q0 + (tre - trs - 1)]))
        t["prod"][r] = prod
        t["exit_nlo"][r] = gg.nti_landing_out[:, q0] * prod
        if last_row == W - 1:
            t["exit_trans"][r] = gg.transition[q0 - 1] * prod
        t["exit_li"][r] = gg.landing_in[q0]
    return SamplerJunction(W, nL, nR, len(J.state_strs), **t)


def sampler_tables(h):
    """(vd, dj or None): linearham_amd.capi.SamplerJunction tables of an oracle object, for Family.set_sampler."""
    fb = h.flexbounds
    if h.locus == "igh":
        return (_sampler_junction(h, h.vd_junction, h.vd_junction_xmsa_inds, h.vgerm, h.dgerm, fb["v_r"]),
                _sampler_junction(h, h.dj_junction, h.dj_junction_xmsa_inds, h.dgerm, h.jgerm, fb["d_r"]))
    return _sampler_junction(h, h.vd_junction, h.vd_junction_xmsa_inds, h.vgerm, h.jgerm, fb["v_r"]), None


# ---------------------------------------------------------------------------------------------------------------------
# K8's structured algorithm in numpy (what lh_viterbi.hip does, on the descriptor's tables): the cross-gene term as one
# maximum and one arg-max per row, one predecessor code per (row, right gene, state), the trace-back through the sampler
# tables.  Plain products, no rescaling (small families only).  Validates the structure and the tie rule against the dense
# sweep without a GPU.
# ---------------------------------------------------------------------------------------------------------------------

def _segment_products(seg, em):
    n = len(seg.offsets) - 1
    return np.array([np.prod(em[seg.xmsa_inds[seg.offsets[g]:seg.offsets[g + 1]]]) for g in range(n)])


def _best(cands, last=False):
    """(value, code) of the first candidate that no later one exceeds: a later kind wins only when strictly larger.
    last: the opposite rule (the last of equals), which no implementation follows: it shows where ties are."""
    v, c = cands[0], 0
    for k in range(1, len(cands)):
        if cands[k] > v or (last and cands[k] == v):
            v, c = cands[k], k
    return v, c


def _argmax(v, last=False):
    return len(v) - 1 - int(np.argmax(v[::-1])) if last else int(np.argmax(v))


def _structured_junction(J, em, f_in, germ_em, pad_trans, pad_em, last=False):
    E = lambda idx: np.where(idx >= 0, em[np.maximum(idx, 0)], 0.0)
    W, nL, nR = J.n_rows, J.n_left, J.n_right
    ltr = J.left_trans.reshape(W, nL).copy()
    ltr[0] = J.enter_trans
    llo, lx = J.left_lo.reshape(W, nL), J.left_xmsa.reshape(W, nL)
    nli, ntt = J.right_gp_nli.reshape(nR, 4), J.right_ntt.reshape(nR, 4, 4)
    nlo, rtr = J.right_nlo.reshape(W, nR, 4), J.right_trans.reshape(W, nR)
    rli, rx, nx = J.right_gp_li.reshape(W, nR), J.right_xmsa.reshape(W, nR), J.nti_xmsa.reshape(W, nR, 4)
    xnlo = J.exit_nlo.reshape(nR, 4)
    argl = np.zeros(W + 1, dtype=np.int64)
    code = np.zeros((W, 5, nR), dtype=np.int64)
    cexit = np.zeros(nR, dtype=np.int64)
    fL, fN, fR = np.array(f_in, dtype=float), np.zeros((nR, 4)), np.zeros(nR)
    part = fL * J.enter_lo
    argl[0] = _argmax(part, last)
    A = part[argl[0]]
    for i in range(W):
        fL = (fL * ltr[i]) * E(lx[i])
        newN, newR = np.zeros((nR, 4)), np.zeros(nR)
        for r in range(nR):
            for b in range(4):
                v, c = _best([A * nli[r, b]] + [fN[r, a] * ntt[r, a, b] for a in range(4)], last)
                newN[r, b], code[i, b, r] = v * E(nx[i, r, b]), c
            v, c = _best([A * rli[i, r]] + [fN[r, a] * nlo[i, r, a] for a in range(4)] + [fR[r] * rtr[i, r]], last)
            newR[r], code[i, 4, r] = v * E(rx[i, r]), c
        fN, fR = newN, newR
        part = fL * llo[i]
        argl[i + 1] = _argmax(part, last)
        A = part[argl[i + 1]]
    g = np.zeros(nR)
    for r in range(nR):
        v, c = _best([A * J.exit_gp_li[r]] + [fN[r, a] * xnlo[r, a] for a in range(4)] + [fR[r] * J.exit_trans[r]], last)
        g[r], cexit[r] = v * germ_em[r], c
    if pad_trans is not None:
        g = g * pad_trans
    if pad_em is not None:
        g = g * pad_em
    return g, (argl, code, cexit)


def _trace_junction(S, bp, right_gene):
    argl, code, cexit = bp
    W, r = S.n_rows, right_gene
    out = [0] * W
    kind, i = int(cexit[r]), W - 1
    while i >= 0 and kind != 0:
        k = 4 if kind == 5 else kind - 1
        out[i] = int(S.right_dense[r]) + (4 + (i - int(S.right_first[r])) if kind == 5 else k)
        kind = int(code[i, k, r])
        i -= 1
    l = int(argl[i + 1])
    while i >= 0:
        out[i] = int(S.left_dense[l]) + i
        i -= 1
    return out, l


def emulate_viterbi(desc, sampler, em, prefer_last=False):
    """(states in K4's layout, log P(data, path)) of the per-column emissions `em` by K8's structured algorithm.
    prefer_last: break every tie the other way (see _best)."""
    last = prefer_last
    em = np.asarray(em, dtype=float)
    svd, sdj = sampler
    f = desc.vgerm_gene_prob * desc.vpadding_transition * _segment_products(desc.vpadding, em) * desc.vgerm_trans_prod * \
        _segment_products(desc.vgerm, em)
    je = _segment_products(desc.jgerm, em)
    jp = _segment_products(desc.jpadding, em)
    if desc.has_d:
        gD, bp_vd = _structured_junction(desc.vd, em, f, _segment_products(desc.dgerm, em), None, None, last)
        gJ, bp_dj = _structured_junction(desc.dj, em, gD, je, desc.jpadding_transition, jp, last)
        jg = _argmax(gJ, last)
        dj_rows, dg = _trace_junction(sdj, bp_dj, jg)
        vd_rows, vg = _trace_junction(svd, bp_vd, dg)
        states = [jg] + dj_rows + [dg] + vd_rows + [vg]
    else:
        gJ, bp_vd = _structured_junction(desc.vd, em, f, je, desc.jpadding_transition, jp, last)
        jg = _argmax(gJ, last)
        vd_rows, vg = _trace_junction(svd, bp_vd, jg)
        states = [jg] + vd_rows + [vg]
    return np.array(states, dtype=np.int32), math.log(gJ[jg])
