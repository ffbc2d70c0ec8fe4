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


# ---- K9: codon and amino-acid tables ----
# A codon's 125 entries are indexed 25 b1 + 5 b2 + b3 over BASES.  The device writes the codons that have a site in a
# junction row (the "window" codons) and the gene posteriors; a codon inside one germline region is a linear map of that
# region's gene posterior (each gene writes its three bases there, N where it writes none).

def _site_regions(ss):
    """Per alignment site the germline region that owns it ("vgerm" / "dgerm" / "jgerm"), or None for a junction row."""
    L = len(ss["msa"][0])
    juncs = _junctions(ss)
    out = [None] * L
    bounds = []
    for jname, gl, gr, site0, W in juncs:
        bounds.append((site0, site0 + W, gl, gr))
    for s in range(L):
        reg = bounds[0][2]
        for lo, hi, gl, gr in bounds:
            if s >= hi:
                reg = gr
            elif s >= lo:
                reg = None
                break
        out[s] = reg
    return out


def codon_layout(ss, frame):
    """The layout lh_codon_layout reports, from the state space alone: dict(frame, n_codons, window_codon, n_genes)."""
    if frame not in (0, 1, 2):
        raise ValueError("frame must be 0, 1 or 2")
    L = len(ss["msa"][0])
    reg = _site_regions(ss)
    n_codons = (L - frame) // 3 if L >= frame else 0
    window = [c for c in range(n_codons) if any(reg[frame + 3 * c + o] is None for o in range(3))]
    blocks, _ = layout(ss)
    n_genes = sum(len(info) for kind, _, _, info in blocks if kind == "germ")
    return dict(frame=frame, n_codons=n_codons, window_codon=window, n_genes=n_genes)


def _gene_site_bases(ss, region):
    """[n_genes][L] base each gene of a germline region writes on each site (4 = N where it writes none), genes in the
    compact layout's (sorted) order."""
    L = len(ss["msa"][0])
    ranges, sites, bases = (ss[region + "_" + f] for f in ("ggene_ranges", "site_inds", "naive_bases"))
    names = sorted(ranges)
    out = np.full((len(names), L), 4, dtype=np.int64)
    for g, name in enumerate(names):
        rs, re_ = ranges[name]
        for k in range(rs, re_):
            out[g, sites[k]] = bases[k]
    return out


def codon_table(ss, windows, genes, lay):
    """[n_codons][125] from the device's windows [n_window][125] and gene posteriors [n_genes] (V | D | J) under the layout
    `lay` (codon_layout, or capi's codon_layout of the handle plus its frame)."""
    windows = np.asarray(windows, dtype=np.float64).reshape(-1, 125)
    genes = np.asarray(genes, dtype=np.float64)
    frame, n_codons = lay["frame"], lay["n_codons"]
    wc = list(lay["window_codon"])
    assert windows.shape[0] == len(wc) and genes.shape[-1] == lay["n_genes"]
    table = np.zeros((n_codons, 125))
    reg = _site_regions(ss)
    regions = ["vgerm"] + (["dgerm"] if ss["locus"] == "igh" else []) + ["jgerm"]
    off, gb, goff = 0, {}, {}
    for r in regions:
        gb[r] = _gene_site_bases(ss, r)
        goff[r] = off
        off += gb[r].shape[0]
    is_window = set(wc)
    for i, c in enumerate(wc):
        table[c] = windows[i]
    for c in range(n_codons):
        if c in is_window:
            continue
        s0 = frame + 3 * c
        r = reg[s0]
        assert r is not None and reg[s0 + 1] == r and reg[s0 + 2] == r
        b = gb[r][:, s0:s0 + 3]
        np.add.at(table[c], 25 * b[:, 0] + 5 * b[:, 1] + b[:, 2], genes[goff[r]:goff[r] + b.shape[0]])
    return table


def codon_site_base(table, frame, L):
    """The [L][5] per-site marginals a codon table implies on the sites its codons cover (other sites: NaN)."""
    t = np.asarray(table).reshape(-1, 5, 5, 5)
    sb = np.full((L, 5), np.nan)
    for c in range(t.shape[0]):
        sb[frame + 3 * c] = t[c].sum(axis=(1, 2))
        sb[frame + 3 * c + 1] = t[c].sum(axis=(0, 2))
        sb[frame + 3 * c + 2] = t[c].sum(axis=(0, 1))
    return sb


def codon_amino_acids():
    """The amino acid of each of the 125 codons over BASES: the host library's TranslateDna (its N-codon rule included)."""
    from . import host
    aa = host.translate("".join(BASES[i // 25] + BASES[(i // 5) % 5] + BASES[i % 5] for i in range(125)))
    assert len(aa) == 125
    return aa


def aa_table(table, aa_of_codon=None):
    """Per codon {amino acid: probability} (entries above 0 only), folding a codon table with codon_amino_acids()."""
    aa = aa_of_codon or codon_amino_acids()
    out = []
    for row in np.asarray(table).reshape(-1, 125):
        d = {}
        for i in np.nonzero(row)[0]:
            d[aa[i]] = d.get(aa[i], 0.0) + float(row[i])
        out.append(d)
    return out


# ---- K14: codon and amino-acid tables of a node of a seed's lineage ----
# A node's 64 entries are indexed 16 x1 + 4 x2 + x3 over A, C, G, T: node bases are never N.

def node_codon_amino_acids():
    """The amino acid of each of the 64 node triples (the host library's TranslateDna; '*' for the stop codons)."""
    from . import host
    aa = host.translate("".join(BASES[i // 16] + BASES[(i // 4) % 4] + BASES[i % 4] for i in range(64)))
    assert len(aa) == 64
    return aa


def node_aa_table(table, aa_of_codon=None):
    """Per codon {amino acid: probability} (entries above 0 only), folding a node's codon table [n_codons][64]."""
    aa = aa_of_codon or node_codon_amino_acids()
    out = []
    for row in np.asarray(table).reshape(-1, 64):
        d = {}
        for i in np.nonzero(row)[0]:
            d[aa[i]] = d.get(aa[i], 0.0) + float(row[i])
        out.append(d)
    return out


def change_classes(aa_of_codon=None):
    """[125][64] uint8, the class of a (naive triple, node triple) pair: 0 the naive triple has no N and the node's equals
    it, 1 no N and another triple with the same translation, 2 no N and a different translation, 3 the naive triple holds
    an N.  The device carries the same relation as a compile-time table (capi.HipLibrary.node_codon_classes)."""
    aa = aa_of_codon or node_codon_amino_acids()
    out = np.full((125, 64), 3, dtype=np.uint8)
    for i in range(125):
        b = (i // 25, (i // 5) % 5, i % 5)
        if 4 in b:
            continue
        k = 16 * b[0] + 4 * b[1] + b[2]
        for x in range(64):
            out[i, x] = 0 if x == k else 1 if aa[x] == aa[k] else 2
    return out


# ---- K15: amino-acid replacements along the edges of a seed's lineage ----
AA_SYMBOLS = "ACDEFGHIKLMNPQRSTVWY*"  # the 21 symbols of aa_counts (capi.AA_SYMBOLS), the stop codons a symbol of their own


def aa_symbols(aa_of_codon=None):
    """[64] uint8: the symbol (index into AA_SYMBOLS) of every triple 16 x1 + 4 x2 + x3, from the host library's
    TranslateDna.  The device carries the same map as a compile-time table (capi.HipLibrary.codon_edge_symbols)."""
    aa = aa_of_codon or node_codon_amino_acids()
    return np.array([AA_SYMBOLS.index(a) for a in aa], dtype=np.uint8)


def edge_classes(aa_of_codon=None):
    """[64][64] uint8, the class of an inner edge by its (upper triple, lower triple): 0 the same triple, 1 another triple
    with the same translation, 2 a different translation."""
    sym = aa_symbols(aa_of_codon)
    out = np.where(sym[:, None] == sym[None, :], 1, 2).astype(np.uint8)
    out[np.arange(64), np.arange(64)] = 0
    return out
