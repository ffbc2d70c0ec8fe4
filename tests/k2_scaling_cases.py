"""TEST INFRASTRUCTURE (CPU only): emission vectors that drive K2 (lh_forward.hip) into each of its rescaling branches, and
a reference for them that shares nothing with ScaleMatrix.

The reference is an identity.  Every path of the V/D/J HMM emits each alignment site exactly once, so multiplying all
xMSA columns of site t by 2^-k_t multiplies every path's probability by 2^-sum(k): the log-likelihood moves by exactly
-ln 2 * sum(k), whatever the 2^256 rescalings did on the way.  A case is (em0', k): a benign base vector and one integer
per site; its emissions are ldexp(em0', -k[site of the column]) -- an exact operation -- and its expected log-likelihood
is the oracle's value at em0' (a run that rescales little or not at all) less ln 2 * sum(k).

The cases (build_cases) are chosen by the branch they reach; check_conditions asserts, on the numpy oracle, that each one
does reach it and that no case sits where two correct implementations may differ (a running product within rounding of a
2^-256 boundary, the documented subnormal corner of K2b).  tests/test_k2_scaling_cases_cpu.py runs all of this without
a GPU; tests/k2_forms_worker.py feeds the same cases to the device."""
import math
import os

import numpy as np

from oracle import linearham_oracle as orc

LN2 = math.log(2.0)
SETS = ("vpadding", "vgerm", "dgerm", "jgerm", "jpadding")
FORWARD_KEYS = ("vgerm_forward", "vd_junction_forward", "dgerm_forward", "dj_junction_forward", "jgerm_forward")
COUNT_KEYS = ("vgerm_scaler_count", "vd_junction_scaler_counts", "dgerm_scaler_count", "dj_junction_scaler_counts",
              "jgerm_scaler_count")
BOUNDARY_RTOL = 1e-6       # condition (a)
EXT_SPREAD_BITS = 900      # condition (c)
# condition (c) for delta4: the extended-range mode equalises every set to its smallest count and keeps an allele down to
# 2^-1024 below the set's best (fill_segments_ext; further down its product is a vanishing subnormal or 0).  delta4 puts
# the counts of the V germline set four apart and those of the V padding set three: the alleles with the long padding
# keep 2^-768 there and are the best of the germline set.  With BOTH sets four apart (their spreads then pass 1024 bits)
# every V allele is 2^-1024 down in one of its two factors, the first forward vector holds zeros and subnormals only and
# the mode returns -inf, as it says it does beyond that range.
EXT_DELTA4_BITS = 1024


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------

def family_specs():
    """name -> synthetic spec (None: the toy golden family).  The trees and leaves do not matter -- the emissions are
    supplied -- so every family has the fewest leaves; the allele counts pick K2's launch shape."""
    from tools import synth_family as sf
    few = dict(n_leaves=6, n_samples=1)   # (six rows: load_family writes every site's own pattern into them)
    return {
        "toy": None,                                                              # pair forms, 36 columns
        "small_igh": sf.Spec.small(**few),                                        # vd2<1>+dj
        "small_igk": sf.Spec.small(locus="igk", seed=43, **few),                  # junction<1,1>: light chain, no D
        "igh_70_33_5": sf.Spec.small(n_v=70, n_d=33, n_j=5, seed=61, **few),      # junction<2,1>: one wave per sample
        "igh_v260": sf.Spec.small(n_v=260, n_d=3, n_j=3, seed=62, **few),         # vd<8>+dj, K2a with two genes a thread
        # 24 V alleles on 296 sites: the V germline set in consensus form (test_consensus_products_equal_the_factor_walk)
        "igh_cons": sf.Spec(n_sites=400, n_v=24, n_d=6, n_j=4, seed=123, **few),
        # the wide germline sets: GA = V alleles / 64 rounded up to 1, 2, 4, 8, 16; GB likewise (1, 2, 4) of the D / J sets
        "igh_v70": sf.Spec.small(n_v=70, n_d=3, n_j=3, seed=63, **few),           # vd2<2>+dj
        "igh_v130_d30_j12": sf.Spec.small(n_v=130, n_d=30, n_j=12, seed=64, **few),  # vd2<4>+dj, the benchmark's counts
        "igh_v520": sf.Spec.small(n_v=520, n_d=3, n_j=3, seed=65, **few),         # vd<16>+dj, K2a with four genes a thread
        "igh_d65": sf.Spec.small(n_v=5, n_d=65, n_j=5, seed=66, **few),           # junction<1,2>
        "igh_j130": sf.Spec.small(n_v=5, n_d=3, n_j=130, seed=67, **few),         # junction<1,4>: GA < GB
        "igh_v130_d70": sf.Spec.small(n_v=130, n_d=70, n_j=5, seed=68, **few),    # junction<4,2>
        "igk_v70_j70": sf.Spec.small(locus="igk", n_v=70, n_j=70, seed=69, **few),   # junction<2,2>: light chain, GB > 1
        "igh_v520_j130": sf.Spec.small(n_v=520, n_d=3, n_j=130, seed=70, **few),  # junction<16,4>
    }


# seeds of (em0, k) per family, fixed so that conditions (a) to (d) hold (check_conditions)
SEEDS = {"toy": 1, "small_igh": 1, "small_igk": 1, "igh_70_33_5": 1, "igh_v260": 1, "igh_cons": 1,
         # (igh_v130_d30_j12 at seed 1 and igh_v520 at seeds 1 to 6: the k that puts two counts four apart, 504 bits on
         # either coverage site, brings one of the 130 / 520 running products within 1e-3 of a boundary; delta4's search
         # goes on to 512 a site, and every V allele is then more than 2^-1024 below the best of its padding or of its
         # germline set -- EXT_DELTA4_BITS)
         "igh_v70": 1, "igh_v130_d30_j12": 2, "igh_v520": 7, "igh_d65": 1, "igh_j130": 1, "igh_v130_d70": 1,
         "igk_v70_j70": 1, "igh_v520_j130": 1}


# cases each family must be able to express (build_cases leaves out what a layout cannot: the toy family's V alleles have
# fewer than eight germline factors and all start at the same site)
_ALL = ("chunk_fast", "chunk_step", "chunk_fast_j", "chunk_step_j", "exact", "exact_below", "zero", "delta3", "delta4", "row3")
NEED = {"toy": ("exact", "exact_below", "zero", "row3"), "small_igh": _ALL, "small_igk": _ALL, "igh_70_33_5": _ALL,
        "igh_v260": _ALL, "igh_cons": _ALL,
        "igh_v70": _ALL, "igh_v130_d30_j12": _ALL, "igh_v520": _ALL, "igh_j130": _ALL,
        # (no delta4, at any seed: its five V alleles differ in coverage on ONE site, and a single emission stays a normal
        # number only to 2^-960 -- short of the 2^-1024 that puts two counts of a set four apart)
        "igh_d65": tuple(n for n in _ALL if n != "delta4"),
        "igh_v130_d70": _ALL, "igk_v70_j70": _ALL, "igh_v520_j130": _ALL}

# the families of the wide germline sets (GA or GB above 1 in a form no other family reaches)
WIDE = ("igh_v70", "igh_v130_d30_j12", "igh_v520", "igh_d65", "igh_j130", "igh_v130_d70", "igk_v70_j70", "igh_v520_j130")


def load_family(name, workdir):
    """The oracle object of a family (generated into workdir/<name> when synthetic)."""
    spec = family_specs()[name]
    if spec is None:
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
        return orc.PhyloHMM(os.path.join(d, "phylo_hmm_input.yaml"), 0, os.path.join(d, "hmm_params"), 0)
    from tools import synth_family as sf
    out = os.path.join(str(workdir), name)
    sf.generate(spec, out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    # The device reads ONE emission per distinct (naive base, site pattern) pair: xMSA columns of sites with the same
    # pattern share theirs, as they do when K1 computes them.  The cases scale site by site, so every site gets a pattern
    # of its own -- its number in base four down the rows (the oracle, given emissions, never reads the alignment).
    n, L = h.msa.shape
    assert 4 ** n >= L
    h.msa = np.array([[(j // 4 ** i) % 4 for j in range(L)] for i in range(n)], dtype=np.int32)
    h._initialize_xmsa_structs()
    return h


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on supplied emissions, with what the conditions need recorded on the way
# ---------------------------------------------------------------------------------------------------------------------

def column_sites(h):
    site = np.zeros(len(h.xmsa_ids), dtype=np.int64)
    for (_, s), xi in h.xmsa_ids.items():
        site[xi] = s
    return site


def _boundary_distance(v):
    """smallest |v / 2^(-256 j) - 1| over j = 1..4 (v > 0)"""
    m, e = math.frexp(v)                # v = m * 2^e, 0.5 <= m < 1
    d = math.inf
    for j in range(1, 5):
        if e == 1 - 256 * j:            # just above the boundary (or on it)
            d = min(d, 2.0 * m - 1.0)
        elif e == -256 * j:             # just below
            d = min(d, 1.0 - m)
    return d if d < math.inf else 1.0   # (another binade: at least a factor of two away)


def germline_walk(h, em):
    """FillGermlinePaddingEmission's running products, restated to look inside: per set the genes' ScaleMatrix counts and
    log2 products, and over all sets the closest any running product comes to a 2^(-256 j) boundary."""
    out = {"near": math.inf}
    for name in SETS:
        R, inds = getattr(h, name), getattr(h, name + "_xmsa_inds")
        counts, log2p = [], []
        for g in sorted(R.ggene_ranges):
            rs, re_ = R.ggene_ranges[g]
            v, c, l2 = 1.0, 0, 0.0
            for j in range(rs, re_):
                e = float(em[inds[j]])
                v *= e
                l2 = l2 + math.log2(e) if e > 0 else -math.inf
                if v > 0:
                    out["near"] = min(out["near"], _boundary_distance(v))
                while 0 < v < orc.SCALE_THRESHOLD:
                    v *= orc.SCALE_FACTOR
                    c += 1
            counts.append(c)
            log2p.append(l2)
        out[name] = {"counts": counts, "log2": log2p}
    return out


def set_gap(walk, s):
    return max(walk[s]["counts"]) - min(walk[s]["counts"]) if walk[s]["counts"] else 0


def max_gap(walk):
    """the largest difference of two genes' counts inside one set: the d of the reference's 2^(256 d) equalisation"""
    return max(set_gap(walk, s) for s in SETS)


def ext_spread_bits(walk):
    """condition (c): how far, in bits, the smallest positive product of a set lies below that set's largest"""
    worst = 0.0
    for s in SETS:
        l2 = [x for x in walk[s]["log2"] if x > -math.inf]
        if l2:
            worst = max(worst, max(l2) - min(l2))
    return worst


def oracle_eval(h, em):
    """The numpy oracle on the emission vector `em`: log-likelihood, forward arrays, ScaleMatrix counts, and what every
    ScaleMatrix call of the forward sweep saw (smallest positive entry before it rescaled, and how often it did)."""
    rows = []
    plain = orc.scale_matrix

    def recording(m):
        pos = m[m > 0]
        lo = float(pos.min()) if pos.size else math.inf
        n = plain(m)
        rows.append((lo, n))
        return n
    h.vgerm_scaler_count = h.dgerm_scaler_count = h.jgerm_scaler_count = 0
    h.xmsa_emission = np.array(em, dtype=float)
    orc.scale_matrix = recording
    try:
        with np.errstate(all="ignore"):
            h._initialize_emission()
            h.cache_forward = True
            ll = h.log_likelihood()
    finally:
        orc.scale_matrix = plain
    r = {"loglik": ll, "rows": rows}
    for k in FORWARD_KEYS + COUNT_KEYS:
        if hasattr(h, k) and (h.locus == "igh" or not k.startswith(("dgerm", "dj_"))):
            v = getattr(h, k)
            r[k] = v.copy() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, list) else v)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, em0, k, site, expect="finite", base=None):
        self.name, self.em0, self.k, self.expect = name, em0, np.asarray(k, dtype=np.int64), expect
        self.base = base or name            # cases with the same em0' share one oracle run at k = 0
        self.em = np.ldexp(em0, -self.k[site].astype(np.int64))
        self.sum_k = int(self.k.sum())


def _gene_factors(h, set_name, min_len, pick="longest"):
    """(gene name, xMSA indices of its factors in walk order) of one gene of a set with at least min_len factors"""
    R, inds = getattr(h, set_name), getattr(h, set_name + "_xmsa_inds")
    best = None
    for g in sorted(R.ggene_ranges):
        rs, re_ = R.ggene_ranges[g]
        if re_ - rs >= min_len and (best is None or re_ - rs > best[2]):
            best = (g, inds[rs:re_], re_ - rs)
    return best[:2] if best else None


def _coverage_sites(h, end="v"):
    """sites where the V (or J) alleles differ in padding versus germline coverage: in some allele's padding, not in all"""
    R = h.vpadding if end == "v" else h.jpadding
    n = len(R.ggene_ranges)
    seen = {}
    for g in R.ggene_ranges:
        rs, re_ = R.ggene_ranges[g]
        for j in range(rs, re_):
            seen[R.site_inds[j]] = seen.get(R.site_inds[j], 0) + 1
    # (an allele that starts before the flexbound has no padding at all: every padding site then differs)
    return sorted(s for s, c in seen.items() if c < n)


def _junction_sites(h):
    fb = h.flexbounds
    if h.locus == "igh":
        return list(range(fb["v_r"][0], fb["d_l"][1])) + list(range(fb["d_r"][0], fb["j_l"][1]))
    return list(range(fb["v_r"][0], fb["j_l"][1]))


def _zero_candidates(h):
    """columns whose emission may be 0 with the likelihood still positive: first those only one germline allele reads (the
    factor walk then meets a zero), then those only NTI states read"""
    users = {}
    for s in SETS:
        R, inds = getattr(h, s), getattr(h, s + "_xmsa_inds")
        for gi, g in enumerate(sorted(R.ggene_ranges)):
            rs, re_ = R.ggene_ranges[g]
            for j in range(rs, re_):
                users.setdefault(int(inds[j]), set()).add((s[0], g))
    junction_germ, nti = set(), set()
    for J, Jx in ((h.vd_junction, h.vd_junction_xmsa_inds), (h.dj_junction, h.dj_junction_xmsa_inds)):
        if Jx.size == 0:
            continue
        for st in range(Jx.shape[1]):
            cols = set(int(x) for x in Jx[:, st] if x >= 0)
            (nti if J.site_inds[st] == -1 else junction_germ).update(cols)
    private = [c for c, u in sorted(users.items()) if len(u) == 1 and c not in junction_germ and c not in nti]
    return private + sorted(nti - junction_germ - set(users))


def build_cases(h, seed):
    """-> (site of every column, ordered list of Case).  Cases a family's layout cannot express (no V allele with eight
    germline factors, no coverage difference among the V alleles) are left out; check_conditions says which must exist."""
    site = column_sites(h)
    n_sites = int(site.max()) + 1
    C = len(site)
    rng = np.random.default_rng(seed)
    em0 = rng.uniform(0.05, 1.0, size=C)
    zero_k = np.zeros(n_sites, dtype=np.int64)
    cases = [Case("base", em0, zero_k, site)]
    # On the sites where alleles differ in padding versus germline coverage (the first few V sites, the last J sites) the
    # draws are kept to 600 bits per end: what one allele meets there in its padding another meets in its germline
    # product, and the two sets are equalised apart -- beyond 2^-768 the reference overflows (that is delta4's business),
    # beyond condition (c) the extended-range mode drops the allele.
    cov_v, cov_j = _coverage_sites(h, "v"), _coverage_sites(h, "j")

    def draw(hi):
        k = rng.integers(0, hi, size=n_sites)
        for cov in (cov_v, cov_j):
            if cov:
                k[cov] = rng.integers(0, min(hi, 600 // len(cov) + 1), size=len(cov))
        return k
    cases.append(Case("single", em0, draw(60), site, base="base"))
    cases.append(Case("double", em0, draw(300), site, base="base"))

    # eight consecutive factors of one V allele inside one 16-byte index chunk (chunk j = the gene's factors 8j..8j+7)
    gene = _gene_factors(h, "vgerm", 8)
    if gene:
        k = zero_k.copy()
        k[site[gene[1][:8]]] = 90          # 2^-720 and the factors themselves: >= 2^-768, the chunk's fast path
        cases.append(Case("chunk_fast", em0, k, site, base="base"))
        k = zero_k.copy()
        k[site[gene[1][:8]]] = 100         # below 2^-768: step by step
        cases.append(Case("chunk_step", em0, k, site, base="base"))
    # the same on a J allele: the small sets walk on one wave each (fill_segments_wave), a copy of the chunk logic
    gene_j = _gene_factors(h, "jgerm", 8)
    if gene_j:
        k = zero_k.copy()
        k[site[gene_j[1][:8]]] = 90
        cases.append(Case("chunk_fast_j", em0, k, site, base="base"))
        k = zero_k.copy()
        k[site[gene_j[1][:8]]] = 100
        cases.append(Case("chunk_step_j", em0, k, site, base="base"))

    # exact: every emission a power of two, one V allele's running product exactly 2^-256 after its fourth factor (no
    # rescaling: ScaleMatrix asks for < 2^-256) and one J allele's exactly 2^-512 (one rescaling, not two); the twin one
    # factor of 2 lower rescales once and twice
    gv, gj = _gene_factors(h, "vgerm", 1), _gene_factors(h, "jgerm", 1)
    if gv and gj:
        pv, pj = min(3, len(gv[1]) - 1), min(3, len(gj[1]) - 1)     # (the fourth factor, or the last of a shorter allele)
        expo = rng.integers(0, 4, size=C)
        em2 = np.ldexp(1.0, -expo)
        k = zero_k.copy()
        k[site[gv[1][pv]]] = 256 - int(expo[gv[1][:pv + 1]].sum())
        k[site[gj[1][pj]]] = 512 - int(expo[gj[1][:pj + 1]].sum())
        cases.append(Case("exact_base", em2, zero_k, site))
        cases.append(Case("exact", em2, k, site, base="exact_base"))
        k2 = k.copy()
        k2[site[gv[1][pv]]] += 1
        k2[site[gj[1][pj]]] += 1
        cases.append(Case("exact_below", em2, k2, site, base="exact_base"))

    # zero: `single` with one column at 0 that leaves the likelihood positive -- the sample takes K2a's per-sample
    # fallback (em_bad); 0 * 2^-k = 0, so the identity holds
    single_k = cases[1].k
    for col in _zero_candidates(h):
        emz = em0.copy()
        emz[col] = 0.0
        # (an allele whose product is 0 stops counting: where the others count far ahead of it the equalisation gives
        # 0 * inf -- such a column is passed over)
        if np.isfinite(oracle_eval(h, np.ldexp(emz, -single_k[site]))["loglik"]):
            cases.append(Case("zero_base", emz, zero_k, site))
            cases.append(Case("zero", emz, single_k, site, base="zero_base"))
            break

    # delta3 / delta4: k on the coverage sites alone, grown evenly until the widest gap between two alleles' counts in
    # one set is 3 (the 2^768 equalisation factor, finite) and 4 (pow(2^256, 4): inf).  delta3 waits until the V padding
    # AND the V germline set are three apart: both then multiply by 2^768 and the first forward vector passes 2^512
    cov = cov_v
    if cov:
        found, both = {}, False
        for total in range(0, 1400 * len(cov), 16):
            k = zero_k.copy()
            k[cov] = total // len(cov)
            if k.max() >= 960:           # (the emissions themselves stay normal numbers)
                break
            w = germline_walk(h, np.ldexp(em0, -k[site]))
            gap = max_gap(w)
            if gap == 3 and w["near"] > 1e-3 and (3 not in found or (not both and set_gap(w, "vpadding") == 3
                                                                    and set_gap(w, "vgerm") == 3)):
                both = set_gap(w, "vpadding") == 3 and set_gap(w, "vgerm") == 3
                found[3] = k
            # (EXT_DELTA4_BITS: where the 16-bit step that first gives 4 is near a boundary, the next one puts BOTH V sets
            # four apart and no allele is left for the extended-range mode; the family then has no delta4 at this seed)
            if gap == 4 and w["near"] > 1e-3 and ext_spread_bits(w) < EXT_DELTA4_BITS:
                found[4] = k
            if 4 in found:
                break
        if 3 in found:
            cases.append(Case("delta3", em0, found[3], site, base="base"))
        if 4 in found:
            cases.append(Case("delta4", em0, found[4], site, expect="overflow", base="base"))
            # control: the same total spread over every site stays finite
            spread = zero_k.copy()
            q, r = divmod(int(found[4].sum()), n_sites)
            spread[:] = q
            spread[:r] += 1
            cases.append(Case("delta4_spread", em0, spread, site, base="base"))

    # row3: one junction row that needs three rescalings at once (row_scale k3 = 3).  2^-700 on the first junction site
    # whose row then falls below 2^-768 at its smallest entry; a little more where no row is that small at 700
    def row3(name, sites, hit):
        for kk in (700, 720, 740, 760):
            for s in sites:
                k = zero_k.copy()
                k[s] = kk
                r = oracle_eval(h, np.ldexp(em0, -k[site]))
                if hit(r) and all(lo >= 2.0 ** -1022 for lo, _ in r["rows"]):
                    cases.append(Case(name, em0, k, site, base="base"))
                    return
    row3("row3", _junction_sites(h), lambda r: any(n == 3 for _, n in r["rows"]))
    # row3_dj: the same on a row of the D-J junction (the search above tries the V-D sites first and stops there on every
    # family whose V-D junction has a row that small): the right-gene sweep of the D-J kernels with k3 = 3
    if h.locus == "igh":
        fb = h.flexbounds
        row3("row3_dj", range(fb["d_r"][0], fb["j_l"][1]), lambda r: 3 in dj_increments(r))
    return site, cases


def dj_increments(oracle):
    """how often each D-J junction row rescaled: the steps of the cumulative count from the D germline region's on"""
    c = [int(oracle["dgerm_scaler_count"])] + [int(x) for x in oracle["dj_junction_scaler_counts"]]
    return [b - a for a, b in zip(c, c[1:])]


# ---------------------------------------------------------------------------------------------------------------------
# reference values and the builder's conditions
# ---------------------------------------------------------------------------------------------------------------------

def references(h, cases):
    """name -> dict(identity = the expected log-likelihood ll(em0') - ln2 * sum k, oracle = oracle_eval on the case's
    emissions, walk = germline_walk on them)"""
    base_ll = {}
    out = {}
    for c in cases:
        if c.sum_k == 0:
            out[c.name] = dict(oracle=oracle_eval(h, c.em), walk=germline_walk(h, c.em))
            base_ll[c.name] = out[c.name]["oracle"]["loglik"]
    for c in cases:
        if c.sum_k != 0:
            out[c.name] = dict(oracle=oracle_eval(h, c.em), walk=germline_walk(h, c.em))
        out[c.name]["identity"] = base_ll[c.base] - LN2 * c.sum_k
    return out


def row_near(rows):
    return min((_boundary_distance(lo) for lo, _ in rows if lo < math.inf), default=math.inf)


def check_conditions(h, cases, refs, need=()):
    """Conditions (a) to (d) of the case builder and the count patterns each case is there for, asserted on the oracle.
    `need`: case names this family must be able to express."""
    names = [c.name for c in cases]
    for n in ("base", "single", "double") + tuple(need):
        assert n in names, "case %s could not be built for this family" % n
    for c in cases:
        r, w = refs[c.name]["oracle"], refs[c.name]["walk"]
        # (a) no running germline product (outside the exact cases, which sit ON a boundary by design and in exact
        #     arithmetic) and no row minimum within 1e-6 relative of a 2^(-256 j) boundary
        if not c.name.startswith("exact"):
            assert w["near"] > BOUNDARY_RTOL, (c.name, "germline product near a boundary", w["near"])
        finite_rows = [x for x in r["rows"] if x[0] < math.inf]
        if c.expect == "finite":
            assert row_near(finite_rows) > BOUNDARY_RTOL, (c.name, "row minimum near a boundary", row_near(finite_rows))
            # (b) the documented subnormal corner of K2b is never entered
            assert all(lo >= 2.0 ** -1022 for lo, _ in finite_rows), (c.name, min(lo for lo, _ in finite_rows))
        # (c) for the extended-range checks: no allele's product more than 2^-900 below its set's best.  delta4 cannot
        #     meet it where an allele has no padding at all (its product is 1 and another's is below 2^-1024): its spread
        #     is reported by ext_spread_bits and the extended-range check of that case stands on its own
        if c.name != "delta4":
            assert ext_spread_bits(w) <= EXT_SPREAD_BITS, (c.name, ext_spread_bits(w))
        else:
            assert ext_spread_bits(w) < EXT_DELTA4_BITS, (c.name, ext_spread_bits(w))
        # (d) overflow exactly on delta4
        assert np.isfinite(r["loglik"]) == (c.expect == "finite"), (c.name, r["loglik"])
        assert (max_gap(w) >= 4) == (c.expect == "overflow"), (c.name, max_gap(w))
    by = {c.name: c for c in cases}
    all_counts = lambda n: [x for s in SETS for x in refs[n]["walk"][s]["counts"]]
    assert max(all_counts("double")) >= 2
    if "chunk_fast" in by:
        _check_chunk(h, by, refs, "vgerm", "chunk_fast", "chunk_step")
    if "chunk_fast_j" in by:
        _check_chunk(h, by, refs, "jgerm", "chunk_fast_j", "chunk_step_j")
    if "exact" in by:
        gv, gj = _gene_factors(h, "vgerm", 1), _gene_factors(h, "jgerm", 1)
        iv, ij = (sorted(getattr(h, s).ggene_ranges).index(g[0]) for s, g in (("vgerm", gv), ("jgerm", gj)))
        nv, nj = min(4, len(gv[1])), min(4, len(gj[1]))
        for name, below in (("exact", 0), ("exact_below", 1)):
            em = by[name].em
            pv, pj = float(np.prod(em[gv[1][:nv]])), float(np.prod(em[gj[1][:nj]]))
            # exactly 2^-256: no rescaling; exactly 2^-512: one, not two; a factor of two lower: one and two
            assert pv == math.ldexp(1.0, -256 - below) and pj == math.ldexp(1.0, -512 - below), (name, pv, pj)
            w = refs[name]["walk"]
            assert w["vgerm"]["counts"][iv] >= below and w["jgerm"]["counts"][ij] >= 1 + below
            if name == "exact":
                first = (w["vgerm"]["counts"][iv], w["jgerm"]["counts"][ij])
            else:  # the twin's alleles rescale once more at that factor (the factors behind it are the same)
                assert (w["vgerm"]["counts"][iv], w["jgerm"]["counts"][ij]) >= first
    if "zero" in by:
        assert (by["zero"].em == 0).sum() == 1 and np.isfinite(refs["zero"]["oracle"]["loglik"])
    if "delta3" in by:
        assert max_gap(refs["delta3"]["walk"]) == 3
        r = refs["delta3"]["oracle"]
        assert max(float(np.max(r[k])) for k in FORWARD_KEYS if k in r) >= 2.0 ** 512
    if "delta4" in by:
        assert max_gap(refs["delta4"]["walk"]) == 4 and not np.isfinite(refs["delta4"]["oracle"]["loglik"])
        assert np.isfinite(refs["delta4_spread"]["oracle"]["loglik"])
    if "row3" in by:
        assert any(n == 3 for _, n in refs["row3"]["oracle"]["rows"])
    if "row3_dj" in by:
        assert 3 in dj_increments(refs["row3_dj"]["oracle"])


def _check_chunk(h, by, refs, set_name, fast, step):
    """the eight scaled factors lie in the allele's first index chunk; their product (the chunk's smallest prefix, v0 = 1)
    is inside [2^-768, 2^-512) for the fast path -- two rescalings -- and below 2^-768 for the step-by-step path"""
    g = _gene_factors(h, set_name, 8)
    m_fast = float(np.prod(by[fast].em[g[1][:8]]))
    m_step = float(np.prod(by[step].em[g[1][:8]]))
    assert 2.0 ** -768 <= m_fast < 2.0 ** -512, m_fast
    assert 0 < m_step < 2.0 ** -768, m_step
    gi = sorted(getattr(h, set_name).ggene_ranges).index(g[0])
    assert refs[fast]["walk"][set_name]["counts"][gi] >= 2 and refs[step]["walk"][set_name]["counts"][gi] >= 3


def batch_order(cases, n_min=17):
    """Row order of the one device call: neighbours (2j, 2j + 1) -- the two samples of a pair-form wave -- alternate `base`
    with a deep case, in both orders, every case present; repeated to an odd n of at least n_min, so that the call spans
    more than two K2b workgroups of eight samples and its last wave holds one sample."""
    names = [c.name for c in cases]
    deep = [n for n in names if n != "base"]
    order = []
    for i, n in enumerate(deep):
        order += ["base", n] if i % 2 == 0 else [n, "base"]
    i = 0
    while len(order) < n_min or len(order) % 2 == 0:
        order.append(deep[i % len(deep)] if len(order) % 2 == 0 else "base")
        i += 1
    return order
