"""K9's structured algorithm in numpy: what lh_family_set_codons builds from the family descriptor and what lh_codon.hip
computes from the compact forward arrays and the sampler tables, step for step (tagged smoothing steps, skip of tags
without mass, binning by local code).  tests/test_codon_oracle.py compares it with tests/codon_oracle.py's dense form."""
import numpy as np


def tables(desc, frame):
    """lh_family_set_codons: dict(n_pos, n_codons, window_codon, windows = [dict(top, out, mult, ncodes, codes)])."""
    L = desc.msa.shape[1]
    site, base = desc.xmsa_site, desc.xmsa_naive_base
    has_d = bool(desc.has_d)

    def junc(j):
        W, nL, nR = j.n_rows, j.n_left, j.n_right
        lx, rx = np.asarray(j.left_xmsa).reshape(W, nL), np.asarray(j.right_xmsa).reshape(W, nR)
        nx = np.asarray(j.nti_xmsa).reshape(W, nR, 4)
        s0 = int(site[nx[0, 0, 0]])
        assert all(site[nx[i, 0, 0]] == s0 + i for i in range(W))
        rows = []
        for i in range(W):
            c = [base[x] if x >= 0 else 4 for x in lx[i]] + [a for _ in range(nR) for a in range(4)] + \
                [base[x] if x >= 0 else 4 for x in rx[i]]
            rows.append(np.array(c, dtype=np.int64))
        return s0, W, rows
    vs0, Wvd, rows_vd = junc(desc.vd)
    ds0, Wdj, rows_dj = junc(desc.dj) if has_d else (0, 0, [])
    assert not has_d or ds0 > vs0 + Wvd
    n_pos = Wvd + Wdj + 3 if has_d else Wvd + 2
    q_d, q_j = Wvd + 1, n_pos - 1

    def pos(s):
        if s < vs0:
            return 0
        if s < vs0 + Wvd:
            return 1 + s - vs0
        if not has_d:
            return q_j
        if s < ds0:
            return q_d
        if s < ds0 + Wdj:
            return q_d + 1 + s - ds0
        return q_j

    def gene_bases(seg, q):
        off, inds = np.asarray(seg.offsets), np.asarray(seg.xmsa_inds)
        gb = np.full((len(off) - 1, L), 4, dtype=np.int64)
        for g in range(len(off) - 1):
            for x in inds[off[g]:off[g + 1]]:
                assert pos(site[x]) == q  # a germline gene writes inside its region only
                gb[g, site[x]] = base[x]
        return gb
    gb = {0: gene_bases(desc.vgerm, 0), q_j: gene_bases(desc.jgerm, q_j)}
    if has_d:
        gb[q_d] = gene_bases(desc.dgerm, q_d)

    def is_row(q):
        return 1 <= q <= Wvd or (has_d and q_d < q < q_j)
    n_codons = (L - frame) // 3 if L >= frame else 0
    wins, window_codon = [], []
    for c in range(n_codons):
        s0 = frame + 3 * c
        qs = [pos(s0 + o) for o in range(3)]
        if not any(is_row(q) for q in qs):
            continue
        w = dict(mult=[], ncodes=[], codes=[], out=len(window_codon))
        o = 0
        while o < 3:
            q, last = qs[o], o
            while last + 1 < 3 and qs[last + 1] == q:
                last += 1
            k = last - o + 1
            w["mult"].append(5 ** (2 - last))
            w["ncodes"].append(5 ** k)
            if is_row(q):
                w["codes"].append(rows_vd[q - 1] if q <= Wvd else rows_dj[q - q_d - 1])
            else:
                b = gb[q][:, s0 + o:s0 + last + 1]
                w["codes"].append(b[:, 0] if k == 1 else 5 * b[:, 0] + b[:, 1])
            w["top"] = q
            o = last + 1
        window_codon.append(c)
        wins.append(w)
    return dict(n_pos=n_pos, n_codons=n_codons, window_codon=window_codon, windows=wins[::-1], Wvd=Wvd, Wdj=Wdj,
                has_d=has_d)


def _ratio(p, z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p != 0, p / np.where(p != 0, z, 1.0), 0.0)


def _split(J, v):
    nL, nR = J.n_left, J.n_right
    return v[:nL], v[nL:nL + 4 * nR].reshape(nR, 4), v[nL + 4 * nR:]


def _shaped(J):
    W, nL, nR = J.n_rows, J.n_left, J.n_right
    return dict(left_lo=J.left_lo.reshape(W, nL), nli=J.nti_landing_in.reshape(nR, 4), ntt=J.nti_transition.reshape(nR, 4, 4),
                nlo=J.nti_landing_out.reshape(W, nR, 4), li=J.landing_in.reshape(W, nR), rt=J.right_trans.reshape(W, nR),
                xn=J.exit_nlo.reshape(nR, 4))


def step_row(J, i, f, nxt):
    S = _shaped(J)
    fL, fN, fR = _split(J, f)
    pL, pN, pR = _split(J, nxt)
    here, gp = i < J.left_rows, J.gene_prob
    a = np.sum(S["left_lo"][i][here] * fL[here])
    germ_here, germ_next = i >= J.right_first, i + 1 >= J.right_first
    fg = np.where(germ_here, fR, 0.0)
    z = (gp[:, None] * S["nli"]) * a + np.einsum("rab,ra->rb", S["ntt"], fN)
    li, rt, nlo = np.where(germ_next, S["li"][i + 1], 0.0), np.where(germ_next, S["rt"][i + 1], 0.0), S["nlo"][i + 1]
    zg = (gp * li) * a + (nlo * fN).sum(axis=1) + rt * fg
    rN, rg = _ratio(pN, z), np.where(germ_next, _ratio(pR, zg), 0.0)
    oN = fN * (np.einsum("rab,rb->ra", S["ntt"], rN) + nlo * rg[:, None])
    oR = fg * (rt * rg)
    b = np.sum(gp * ((S["nli"] * rN).sum(axis=1) + li * rg))
    oL = np.where(i + 1 < J.left_rows, pL, 0.0) + np.where(here, fL * (S["left_lo"][i] * b), 0.0)
    return np.concatenate([oL, oN.ravel(), oR])


def step_last(J, f, pg):
    S = _shaped(J)
    i = J.n_rows - 1
    fL, fN, fR = _split(J, f)
    here = i < J.left_rows
    a = np.sum(S["left_lo"][i][here] * fL[here])
    fg = np.where(i >= J.right_first, fR, 0.0)
    c = (J.gene_prob * J.exit_li) * J.prod
    z = c * a + (S["xn"] * fN).sum(axis=1) + J.exit_trans * fg
    rho = _ratio(pg, z)
    oN = fN * (S["xn"] * rho[:, None])
    oR = fg * (J.exit_trans * rho)
    b = np.sum(c * rho)
    oL = np.where(here, fL * (S["left_lo"][i] * b), 0.0)
    return np.concatenate([oL, oN.ravel(), oR])


def step_left(J, f, p0):
    S = _shaped(J)
    pL, pN, pR = _split(J, p0)
    e = np.sum(J.enter_lo * f)
    gp = J.gene_prob
    w = gp[:, None] * S["nli"]
    b = np.sum(_ratio(pN, w * e) * w)
    li = np.where(J.right_first == 0, S["li"][0], 0.0)
    b += np.sum(np.where(li != 0, _ratio(pR, (gp * li) * e) * (gp * li), 0.0))
    return np.where(J.left_rows > 0, pL, 0.0) + f * (J.enter_lo * b)


def kernel(tab, svd, sdj, nV, nD, nJ, F):
    """codon_kernel on one sample's compact forward vector F: (windows [n_window][125], genes V | D | J)."""
    Wvd, Wdj, has_d = tab["Wvd"], tab["Wdj"], tab["has_d"]
    st_vd = svd.n_left + 5 * svd.n_right
    st_dj = sdj.n_left + 5 * sdj.n_right if has_d else 0

    def position(q):  # (kind, junction, row, offset, size)
        if q == 0:
            return 0, svd, 0, 0, nV
        if q <= Wvd:
            return 1, svd, q - 1, nV + (q - 1) * st_vd, st_vd
        off = nV + Wvd * st_vd
        q -= Wvd + 1
        if not has_d:
            return 0, None, 0, off, nJ
        if q == 0:
            return 0, sdj, 0, off, nD
        off += nD
        if q <= Wdj:
            return 1, sdj, q - 1, off + (q - 1) * st_dj, st_dj
        return 0, None, 0, off + Wdj * st_dj, nJ

    def step(q, nxt):
        kind, J, row, off, size = position(q)
        f = F[off:off + size]
        if kind == 0:
            return step_left(J, f, nxt)
        return step_last(J, f, nxt) if row == J.n_rows - 1 else step_row(J, row, f, nxt)

    def bins(v, codes, ncodes, mult, base, dst):
        for c in range(ncodes):
            dst[base + mult * c] = v[codes == c].sum()
    n_pos = tab["n_pos"]
    _, _, _, off, size = position(n_pos - 1)
    cur = F[off:off + size] / F[off:off + size].sum()
    genes = {n_pos - 1: cur}
    out = np.full((len(tab["window_codon"]), 125), np.nan)
    wi, wins = 0, tab["windows"]
    for q in range(n_pos - 1, 0, -1):
        while wi < len(wins) and wins[wi]["top"] == q:
            w = wins[wi]
            dst = out[w["out"]]
            npos = len(w["mult"])
            ctop = w["codes"][npos - 1]
            for c in range(w["ncodes"][npos - 1]):
                m = np.where(ctop == c, cur, 0.0)
                base2 = w["mult"][npos - 1] * c
                if npos == 2:
                    if m.sum() == 0.0:
                        bins(np.zeros(len(w["codes"][0])), w["codes"][0], w["ncodes"][0], w["mult"][0], base2, dst)
                        continue
                    bins(step(q - 1, m), w["codes"][0], w["ncodes"][0], w["mult"][0], base2, dst)
                    continue
                u = step(q - 1, m) if m.sum() != 0.0 else np.zeros(len(w["codes"][1]))
                for d in range(w["ncodes"][1]):
                    m1 = np.where(w["codes"][1] == d, u, 0.0)
                    base = base2 + w["mult"][1] * d
                    v = step(q - 2, m1) if m1.sum() != 0.0 else np.zeros(len(w["codes"][0]))
                    bins(v, w["codes"][0], w["ncodes"][0], w["mult"][0], base, dst)
            wi += 1
        cur = step(q - 1, cur)
        if position(q - 1)[0] == 0:
            genes[q - 1] = cur
    return out, np.concatenate([genes[q] for q in sorted(genes)])
