"""Test-side restatement of the recombination-event posteriors (K10, lh_events.hip) in three forms.

Per junction of W rows, nL left genes and nR right genes: a = the number of junction rows the left gene l occupies,
b = the first row with a germline state of the right gene r (W: none), and
  exit[nL][W+1] = P(l, a),  enter[nR][W+1] = P(r, b),  span[W+1][W+1] = P(a, b).
  enumerated  every state path of non-zero probability, classified (and checked to read left* NTI* right*);
  dense       exit / enter as differences of the smoothed posteriors, span by a backward chain through the oracle's
              dense transitions and forward rows (po.smoothing's conditional step);
  structured  what lh_events.hip computes, step for step, on the compact forward arrays, the compact posteriors and the
              sampler tables (tests/viterbi_oracle.sampler_tables): the table of reciprocal normalisers, then one
              4-vector chain per (right gene, b).
flat() lays a list of junction tables out as lh_events_layout does; columns() maps table indices to the units of the
annotation columns (V3pDel, D5pDel, ...) with the members the sampler reads."""
import numpy as np

from linearham_amd import posterior as lp
from tests import posterior_oracle as po


def junctions(h):
    """[(junction region, left region, right region)] in layout order."""
    if h.locus == "igh":
        return [("vd_junction", "vgerm", "dgerm"), ("dj_junction", "dgerm", "jgerm")]
    return [("vd_junction", "vgerm", "jgerm")]


def _info(h):
    """Per junction the compact layout's info (n_rows, stride, dense [W][stride]) plus nL and nR."""
    blocks, _ = lp.layout(po.state_space(h))
    infos = {}
    for kind, region, _, info in blocks:
        if kind == "junction":
            infos[region] = info
    out = []
    for jname, gl, gr in junctions(h):
        nL, nR = len(getattr(h, gl).state_strs), len(getattr(h, gr).state_strs)
        assert infos[jname]["stride"] == nL + 5 * nR
        out.append((jname, gl, gr, infos[jname], nL, nR))
    return out


def _classes(info, nL, nR):
    """kind[S] (0 left, 1 NTI, 2 right germline; -1: a state on no row) and gene[S] of a junction's dense states."""
    kind = np.full(info["n_states"], -1, dtype=np.int64)
    gene = np.full(info["n_states"], -1, dtype=np.int64)
    d = info["dense"]
    for i in range(info["n_rows"]):
        for c in range(info["stride"]):
            k = d[i, c]
            if k < 0:
                continue
            kind[k] = 0 if c < nL else (1 if c < nL + 4 * nR else 2)
            gene[k] = c if c < nL else ((c - nL) // 4 if c < nL + 4 * nR else c - nL - 4 * nR)
    return kind, gene


def flat(tables):
    """[(exit, enter, span)] per junction -> the flat row of lh_events_layout."""
    return np.concatenate([t.ravel() for j in tables for t in j])


def unflat(h_or_dims, row):
    """The inverse of flat(): dims = [(W, nL, nR)] or an oracle object."""
    dims = h_or_dims if isinstance(h_or_dims, list) else [(i["n_rows"], nL, nR) for _, _, _, i, nL, nR in _info(h_or_dims)]
    out, off = [], 0
    for W, nL, nR in dims:
        sizes = [(nL, W + 1), (nR, W + 1), (W + 1, W + 1)]
        j = []
        for s in sizes:
            j.append(np.asarray(row[off:off + s[0] * s[1]]).reshape(s))
            off += s[0] * s[1]
        out.append(tuple(j))
    assert off == len(row)
    return out


# ---- form 1: enumeration ----

def enumerated(h):
    """([(exit, enter, span)] per junction, number of paths).  Asserts the left* NTI* right* shape of every path."""
    rows = po._rows(*po._chain(h))
    n = len(rows)
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
    where = {}
    for t, (name, i, _, _) in enumerate(rows):
        where[(name, i)] = t
    out = []
    for jname, gl, gr, info, nL, nR in _info(h):
        W = info["n_rows"]
        kind, gene = _classes(info, nL, nR)
        ex, en, sp = np.zeros((nL, W + 1)), np.zeros((nR, W + 1)), np.zeros((W + 1, W + 1))
        for w, path in paths:
            l, r = path[where[(gl, None)]], path[where[(gr, None)]]
            ks = [path[where[(jname, i)]] for i in range(W)]
            kinds = [kind[k] for k in ks]
            assert all(x >= 0 for x in kinds) and kinds == sorted(kinds), kinds  # left* NTI* right*
            a = kinds.count(0)
            b = W - kinds.count(2)
            assert all(gene[k] == l for k in ks[:a]) and all(gene[k] == r for k in ks[a:])
            p = w / total
            ex[l, a] += p
            en[r, b] += p
            sp[a, b] += p
        out.append((ex, en, sp))
    return out, len(paths)


# ---- form 2: dense differences and backward chain ----

def _ratio(p, z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p != 0, p / np.where(p != 0, z, 1.0), 0.0)


def dense(h, post=None):
    """[(exit, enter, span)] per junction from the oracle's forward arrays (after log_likelihood()) and its dense
    transitions; post: po.smoothing(h) if already at hand."""
    post = post if post is not None else po.smoothing(h)
    trans = {"vd_junction": (h.vd_junction_transition, h.vd_junction_dgerm_transition)}
    if h.locus == "igh":
        trans["dj_junction"] = (h.dj_junction_transition, h.dj_junction_jgerm_transition)
    out = []
    for jname, gl, gr, info, nL, nR in _info(h):
        W, d = info["n_rows"], info["dense"]
        kind, _ = _classes(info, nL, nR)
        F = np.asarray(getattr(h, jname + "_forward"), dtype=np.float64)
        P, pl, pr = post[jname], post[gl], post[gr]
        Tjj, Tjg = trans[jname]
        # pi_i(left l), i = -1 .. W, and pi_i(germ r), i = -1 .. W
        left = np.zeros((W + 2, nL))
        right = np.zeros((W + 2, nR))
        left[0] = pl
        right[W + 1] = pr
        for i in range(W):
            for l in range(nL):
                if d[i, l] >= 0:
                    left[i + 1, l] = P[i, d[i, l]]
            for r in range(nR):
                k = d[i, nL + 4 * nR + r]
                if k >= 0:
                    right[i + 1, r] = P[i, k]
        ex = (left[:-1] - left[1:]).T
        en = (right[1:] - right[:-1]).T
        sp = np.zeros((W + 1, W + 1))
        for b in range(W + 1):
            if b == 0:
                sp[0, 0] = np.where(kind == 2, P[0], 0.0).sum()
                continue
            if b == W:
                v = F[W - 1] * (Tjg @ _ratio(pr, F[W - 1] @ Tjg))
            else:
                start = np.where(kind == 2, P[b], 0.0)
                v = F[b - 1] * (Tjj @ _ratio(start, F[b - 1] @ Tjj))
            i = b - 1  # v sits on row i
            while True:
                sp[i + 1, b] = v[kind == 0].sum()
                v = np.where(kind == 1, v, 0.0)
                if i == 0:
                    sp[0, b] = v.sum()  # row 0's NTI states come out of the left region, whichever gene
                    break
                v = F[i - 1] * (Tjj @ _ratio(v, F[i - 1] @ Tjj))
                i -= 1
        out.append((ex, en, sp))
    return out


# ---- form 3: the kernel's structured algorithm ----

def sampler_tables(h):
    """vo.sampler_tables for PhyloHMM and SimpleHMM objects alike, before or after a forward pass (the junctions' row
    counts come from the flexbounds)."""
    from tests import viterbi_oracle as vo
    fb = h.flexbounds
    igh = h.locus == "igh"
    rows = lambda lo, hi: np.zeros((fb[hi][1] - fb[lo][0], 1))
    vd = vo._sampler_junction(h, h.vd_junction, rows("v_r", "d_l" if igh else "j_l"), h.vgerm, h.dgerm if igh else h.jgerm,
                              fb["v_r"])
    if not igh:
        return vd, None
    return vd, vo._sampler_junction(h, h.dj_junction, rows("d_r", "j_l"), h.dgerm, h.jgerm, fb["d_r"])


def _recip(z):
    with np.errstate(divide="ignore"):
        return np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 0.0)


def structured_junction(J, F, P, pl, pg):
    """lh_events.hip's junction_events: F, P [W][nL + 5 nR] compact forward rows and posteriors, pl / pg the posteriors
    of the left and right regions' genes."""
    W, nL, nR = J.n_rows, J.n_left, J.n_right
    llo, nli, ntt = J.left_lo.reshape(W, nL), J.nti_landing_in.reshape(nR, 4), J.nti_transition.reshape(nR, 4, 4)
    nlo, li, rt = J.nti_landing_out.reshape(W, nR, 4), J.landing_in.reshape(W, nR), J.right_trans.reshape(W, nR)
    xn, gp = J.exit_nlo.reshape(nR, 4), J.gene_prob
    fL, fN, fR = F[:, :nL], F[:, nL:nL + 4 * nR].reshape(W, nR, 4), F[:, nL + 4 * nR:]
    pL, pR = P[:, :nL], P[:, nL + 4 * nR:]
    # differences
    ex, en = np.zeros((nL, W + 1)), np.zeros((nR, W + 1))
    prev = pl.copy()
    for a in range(W + 1):
        cur = np.where(a < J.left_rows, pL[a], 0.0) if a < W else np.zeros(nL)
        ex[:, a] = prev - cur
        prev = cur
    prev = np.zeros(nR)
    for b in range(W + 1):
        cur = pg if b == W else np.where(b >= J.right_first, pR[b], 0.0)
        en[:, b] = cur - prev
        prev = cur
    # tabulate
    tz, tg, ta = np.zeros((W, nR, 4)), np.zeros((W, nR)), np.zeros((W, nR))
    for i in range(W):
        here = i < J.left_rows
        a = np.sum(llo[i][here] * fL[i][here])
        fg = np.where(i >= J.right_first, fR[i], 0.0)
        if i + 1 < W:
            nxt = i + 1 >= J.right_first
            tz[i] = _recip((gp[:, None] * nli) * a + np.einsum("rab,ra->rb", ntt, fN[i]))
            l1, r1 = np.where(nxt, li[i + 1], 0.0), np.where(nxt, rt[i + 1], 0.0)
            tg[i] = np.where(nxt, _recip((gp * l1) * a + (nlo[i + 1] * fN[i]).sum(axis=1) + r1 * fg), 0.0)
            ta[i] = gp * a
        else:
            c = (gp * J.exit_li) * J.prod
            tg[i] = _recip(c * a + (xn * fN[i]).sum(axis=1) + J.exit_trans * fg)
            ta[i] = c * a
    # chains, all right genes at once ([nR][4] vectors)
    sp = np.zeros((W + 1, W + 1))
    for b in range(W + 1):
        m = pg if b == W else np.where(b >= J.right_first, pR[b], 0.0)
        if b == 0:
            sp[0, 0] = m.sum()
            continue
        rho = m * tg[b - 1]
        if b == W:
            sp[b, b] = np.sum(ta[b - 1] * rho)
            v = fN[b - 1] * (xn * rho[:, None])
        else:
            lb = np.where(b >= J.right_first, li[b], 0.0)
            sp[b, b] = np.sum((ta[b - 1] * lb) * rho)
            v = fN[b - 1] * (nlo[b] * rho[:, None])
        for i in range(b - 2, -1, -1):
            q = v * tz[i]
            sp[i + 1, b] = np.sum(ta[i] * (nli * q).sum(axis=1))
            v = fN[i] * np.einsum("rab,rb->ra", ntt, q)
        sp[0, b] = v.sum()
    return ex, en, sp


def structured(h, svd, sdj, F=None, P=None):
    """[(exit, enter, span)] per junction by the kernel's algorithm, from compact vectors F (forward) and P (K5's
    posteriors; default: the oracle's own, laid out compactly)."""
    igh = h.locus == "igh"
    if F is None:
        fwd = {k: getattr(h, k + "_forward") for k in ["vgerm", "vd_junction", "jgerm"] + (["dgerm", "dj_junction"] if igh else [])}
        F = po.to_compact(h, fwd)
    if P is None:
        P = po.to_compact(h, po.smoothing(h))
    nV, nD, nJ = len(h.vgerm.state_strs), (len(h.dgerm.state_strs) if igh else 0), len(h.jgerm.state_strs)
    st_vd = svd.n_left + 5 * svd.n_right
    o_vd, o_d = nV, nV + svd.n_rows * st_vd
    o_dj = o_d + nD
    st_dj = sdj.n_left + 5 * sdj.n_right if igh else 0
    o_j = o_dj + (sdj.n_rows * st_dj if igh else 0)
    rows = lambda v, off, J, st: v[off:off + J.n_rows * st].reshape(J.n_rows, st)
    if not igh:
        return [structured_junction(svd, rows(F, o_vd, svd, st_vd), rows(P, o_vd, svd, st_vd), P[:nV], P[o_j:o_j + nJ])]
    return [structured_junction(svd, rows(F, o_vd, svd, st_vd), rows(P, o_vd, svd, st_vd), P[:nV], P[o_d:o_d + nD]),
            structured_junction(sdj, rows(F, o_dj, sdj, st_dj), rows(P, o_dj, sdj, st_dj), P[o_d:o_d + nD], P[o_j:o_j + nJ])]


# ---- the annotation columns ----

def columns(h, tables):
    """{column: {(gene, deletion length): p}} for V3pDel, D5pDel, D3pDel, J5pDel (light chains: V3pDel, J5pDel) and
    {"VDInsertion" | "VJInsertion" | "DJInsertion": [P(length = k)]}, the units read from the members the sampler reads
    (sample_junction_states / sample_germline_state): the junction state's dels on row a - 1 or row b, the germline
    region's right_del for a = 0 and left_del for b = W."""
    igh = h.locus == "igh"
    names = [("V3pDel", "D5pDel", "VDInsertion"), ("D3pDel", "J5pDel", "DJInsertion")] if igh else \
        [("V3pDel", "J5pDel", "VJInsertion")]
    out = {}
    for (jname, gl, gr, info, nL, nR), (ex, en, sp), (cl, cr, ci) in zip(_info(h), tables, names):
        J, GL, GR = getattr(h, jname), getattr(h, gl), getattr(h, gr)
        W, d = info["n_rows"], info["dense"]
        left, right = {}, {}
        for l in range(nL):
            for a in range(W + 1):
                if a > 0 and d[a - 1, l] < 0:
                    if ex[l, a] != 0.0:
                        raise ValueError("weight on a junction row the left gene has no state on")
                    continue
                dl = GL.right_del[l] if a == 0 else J.dels[d[a - 1, l]]
                key = (GL.state_strs[l], int(dl))
                left[key] = left.get(key, 0.0) + ex[l, a]
        for r in range(nR):
            for b in range(W + 1):
                c = nL + 4 * nR + r
                if b < W and d[b, c] < 0:
                    if en[r, b] != 0.0:
                        raise ValueError("weight on a junction row the right gene has no state on")
                    continue
                dl = GR.left_del[r] if b == W else J.dels[d[b, c]]
                key = (GR.state_strs[r], int(dl))
                right[key] = right.get(key, 0.0) + en[r, b]
        out[cl], out[cr] = left, right
        out[ci] = [float(np.trace(sp, k)) for k in range(W + 1)]
    return out
