"""Host side of the posterior kernel K5: maps its compact per-sample posteriors (the layout of lh_eval_outputs.forward)
to dense state posteriors, per-site naive-base distributions and V / D / J gene posteriors, and combines batches.

The mapping needs only the state space, as the host library dumps it (PhyloHMM.dump(1)): keys
`<region>_ggene_ranges`, `<region>_site_inds`, `<region>_naive_bases` for the regions vgerm, vd_junction, dgerm,
dj_junction and jgerm, plus `locus`, `flexbounds` and `msa`.  Site marginals are linear in the state posteriors
because every state writes its naive base on sites no other region writes (HMM::SampleNaiveSequence,
src/HMM.cpp:358-431): a germline-region gene its bases on its sites, a junction state its base on site
site_start + row; sites that nothing writes stay N."""
import math

import numpy as np

BASES = "ACGTN"


def _junctions(ss):
    """(junction, left germline region, right germline region, first site, rows) in compact order."""
    fb = ss["flexbounds"]
    if ss["locus"] == "igh":
        return [("vd_junction", "vgerm", "dgerm", fb["v_r"][0], fb["d_l"][1] - fb["v_r"][0]),
                ("dj_junction", "dgerm", "jgerm", fb["d_r"][0], fb["j_l"][1] - fb["d_r"][0])]
    return [("vd_junction", "vgerm", "jgerm", fb["v_r"][0], fb["j_l"][1] - fb["v_r"][0])]


def layout(ss):
    """The compact layout: a list of ("germ", region, offset, genes) and ("junction", region, offset, info) blocks in
    memory order, where info holds n_rows, stride and, per compact entry of every row, the dense state index (-1: no
    state) and its naive base."""
    blocks = []
    off = 0
    juncs = _junctions(ss)

    def germ(region):
        nonlocal off
        genes = sorted(ss[region + "_ggene_ranges"])
        blocks.append(("germ", region, off, genes))
        off += len(genes)

    germ("vgerm")
    for j, (jname, gl, gr, site0, W) in enumerate(juncs):
        left = sorted(ss[gl + "_ggene_ranges"])
        right = sorted(ss[gr + "_ggene_ranges"])
        ranges = ss[jname + "_ggene_ranges"]
        sites = ss[jname + "_site_inds"]
        bases = ss[jname + "_naive_bases"]
        nL, nR = len(left), len(right)
        stride = nL + 5 * nR
        dense = np.full((W, stride), -1, dtype=np.int64)
        base = np.full((W, stride), 4, dtype=np.int64)
        for l, g in enumerate(left):
            if g not in ranges:
                continue
            rs, re_ = ranges[g]
            for k in range(rs, re_):
                i = sites[k] - site0
                dense[i, l] = k
                base[i, l] = bases[k]
        for r, g in enumerate(right):
            rs, re_ = ranges[g]
            for a in range(4):
                dense[:, nL + 4 * r + a] = rs + a
                base[:, nL + 4 * r + a] = a
            for k in range(rs + 4, re_):
                i = sites[k] - site0
                dense[i, nL + 4 * nR + r] = k
                base[i, nL + 4 * nR + r] = bases[k]
        blocks.append(("junction", jname, off, dict(n_rows=W, stride=stride, dense=dense, base=base, site0=site0,
                                                    n_states=len(ss[jname + "_naive_bases"]))))
        off += W * stride
        if j == 0 and len(juncs) == 2:
            germ("dgerm")
    germ("jgerm")
    return blocks, off


def dense_posteriors(ss, post, lay=None):
    """{region: array}: gene posteriors [n_genes] of vgerm / dgerm / jgerm and [W][S] state posteriors of the junctions,
    in the shapes of the forward members (vgerm_forward, vd_junction_forward, ...)."""
    blocks, size = lay or layout(ss)
    post = np.asarray(post, dtype=np.float64)
    assert post.shape[-1] == size, (post.shape, size)
    out = {}
    for kind, region, off, info in blocks:
        if kind == "germ":
            out[region] = post[off:off + len(info)].copy()
            continue
        W, st, dense = info["n_rows"], info["stride"], info["dense"]
        m = np.zeros((W, info["n_states"]))
        rows = post[off:off + W * st].reshape(W, st)
        for i in range(W):
            ok = dense[i] >= 0
            m[i, dense[i][ok]] += rows[i][ok]
        out[region] = m
    return out


def site_base(ss, post, lay=None):
    """[L][5] distribution of the naive base at every alignment site (A, C, G, T, N)."""
    blocks, size = lay or layout(ss)
    post = np.asarray(post, dtype=np.float64)
    L = len(ss["msa"][0])
    sb = np.zeros((L, 5))
    for kind, region, off, info in blocks:
        if kind == "germ":
            ranges = ss[region + "_ggene_ranges"]
            sites = ss[region + "_site_inds"]
            bases = ss[region + "_naive_bases"]
            for g, name in enumerate(info):
                rs, re_ = ranges[name]
                for k in range(rs, re_):
                    sb[sites[k], bases[k]] += post[off + g]
        else:
            W, st = info["n_rows"], info["stride"]
            rows = post[off:off + W * st].reshape(W, st)
            for i in range(W):
                ok = info["dense"][i] >= 0
                np.add.at(sb[info["site0"] + i], info["base"][i][ok], rows[i][ok])
    sb[:, 4] += 1.0 - sb.sum(axis=1)  # what no state writes stays N
    return sb


def gene_posteriors(ss, post, lay=None):
    """{"V": {gene: p}, "D": {...}, "J": {...}} (no "D" for light chains), gene names as the pipeline spells them."""
    blocks, _ = lay or layout(ss)
    post = np.asarray(post, dtype=np.float64)
    out = {}
    for kind, region, off, info in blocks:
        if kind == "germ":
            out[region[0].upper()] = {name: float(post[off + g]) for g, name in enumerate(info)}
    return out


def combine(parts):
    """Exact combination of per-batch (weighted_sum, weight_stats) pairs, in the order given: returns
    (sum_i w_i pi_i / sum_i w_i, max lw, sum w, sum w^2) with w relative to the overall max lw."""
    parts = [(np.asarray(s, dtype=np.float64), np.asarray(st, dtype=np.float64)) for s, st in parts]
    finite = [st[0] for _, st in parts if math.isfinite(st[0])]
    if not finite:
        return None, -math.inf, 0.0, 0.0
    m = max(finite)
    tot = np.zeros_like(parts[0][0])
    s1 = s2 = 0.0
    for s, st in parts:
        if not math.isfinite(st[0]):
            continue
        f = math.exp(st[0] - m)
        tot = tot + s * f
        s1 += st[1] * f
        s2 += st[2] * f * f
    return tot / s1, m, s1, s2


def kish_ess(s1, s2):
    return s1 * s1 / s2 if s2 > 0 else 0.0
