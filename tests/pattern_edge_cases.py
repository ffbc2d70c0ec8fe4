"""TEST INFRASTRUCTURE (CPU only): families with EXACTLY L distinct alignment columns, for the pattern- and site-count edges of
K1 (launch_prune, lh_prune.hip: two-site waves, the one-site wave, fused workgroups, tiles, register budgets), of
lh_family_create's state planes (blocks of 128 patterns, the tail clamped to pattern np - 1) and of the tree-pass kernels
(a lane per pattern over n_prune + 1, a lane per site).

The technique of k2_scaling_cases.load_family and cadence_cases.load_family: one family from tools/synth_family.py per
base layout, its alignment replaced on the oracle object, _initialize_xmsa_structs() called again, the descriptor built
from that object by desc_builder.build_family_desc.  Pattern p is the base-4 digits of (p * 2654435761) % 4**n down the
n rows (an odd multiplier: distinct p give distinct columns); the first L sites hold patterns 0 .. L-1, site j beyond
them pattern (j * 7919) % L.  The allele sets are small and nearly identical (test_gpu_shape_edges.LONG's way), so that no
two alleles' ScaleMatrix counts come four apart and the oracle's rows stay finite.

Variants (Case): mixed -- N written into one cell of every fifth pattern (two cells of every tenth), which selects the
N-aware kernels and moves those patterns behind the clean ones in the device's order, the count staying exact; all_n -- the
last site all N (alignment padding: n_prune stays L, one more pattern for the tree pass and one more u-column block).

check_premises asserts, on the oracle alone and per row, that a case is not vacuous: exactly L distinct columns, a finite
log-likelihood, every pattern read by some xMSA column, and for every naive base any two distinct patterns' emissions more
than GAP = 1e-7 relative apart -- 1 000 times the 1e-10 emission bound, so a lane that returns a neighbour's, the clamped
last pattern's or another tile's value cannot pass."""
import os

import numpy as np

from oracle import linearham_oracle as orc

MULT = 2654435761
STRIDE = 7919
GAP = 1e-7

_LONG = dict(n_v=3, n_d=2, n_j=2, divergence=0.01, brlen_mean=0.05, n_samples=2)
BASES = {
    "s1100": dict(n_leaves=10, n_sites=1100, len_v=980, seed=5, **_LONG),
    "s256": dict(n_leaves=10, n_sites=256, len_v=150, seed=5, **_LONG),     # pattern counts up to 255
    "s257": dict(n_leaves=10, n_sites=257, len_v=150, seed=5, **_LONG),
    # larger tip tables: K1's register budgets.  Every J allele reaches the end of the alignment (len_j: no J padding), so
    # that the J germline set covers the same sites for every allele.  With the generator's J alleles of 48 to 63 sites the
    # alleles end 0 to 24 sites before the alignment does; a site's emission is near 2^-170 on these trees, the J germline
    # set and the J padding set are then each some 500 to 770 bits apart IN OPPOSITE ORDER, and the extended-range mode --
    # which equalises each set to its own smallest 2^-256 count and multiplies the two plain values -- returns -inf where the
    # default mode is finite ("Pattern-count edges": found here, K2a's, not K1's, and still open).
    "t60": dict(n_leaves=60, n_sites=400, seed=5, len_j=(72, 72), **_LONG),
    "t100": dict(n_leaves=100, n_sites=400, seed=5, len_j=(72, 72), **_LONG),
}


class Case:
    def __init__(self, base, L, mixed=False, all_n=False):
        self.base, self.L, self.mixed, self.all_n = base, int(L), bool(mixed), bool(all_n)
        self.name = "%s_L%d%s%s" % (base, L, "_n" if mixed else "", "_pad" if all_n else "")

    def __repr__(self):
        return self.name


def generate_base(base, workdir):
    """Writes the base family's files into workdir/<base> (once) and returns that directory."""
    from tools import synth_family as sf
    out = os.path.join(str(workdir), base)
    if not os.path.exists(os.path.join(out, "meta.json")):
        sf.generate(sf.Spec(**BASES[base]), out)
    return out


def samples(base, workdir):
    """The base family's two tree samples as run_family takes them."""
    from tools import synth_family as sf
    return sf.read_trees_tsv(os.path.join(generate_base(base, workdir), "trees.tsv"))


def pattern_column(p, n):
    v = (p * MULT) % 4 ** n
    return [(v // 4 ** i) % 4 for i in range(n)]


def alignment(case, n, n_sites):
    """The case's alignment [n, n_sites] and the pattern number of every site (-1: the all-N site)."""
    L = case.L
    assert 1 <= L <= n_sites - (1 if case.all_n else 0) and L <= 4 ** n
    cols = np.array([pattern_column(p, n) for p in range(L)], dtype=np.int32)          # [L, n]
    if case.mixed:
        for p in range(L):
            if p % 5 == 2:
                cols[p, (3 * p) % n] = 4
            if p % 10 == 7:
                cols[p, (7 * p + 1) % n] = 4
    pat = np.array([j if j < L else (j * STRIDE) % L for j in range(n_sites)], dtype=np.int64)
    msa = np.ascontiguousarray(cols[pat].T)
    if case.all_n:
        msa[:, n_sites - 1] = 4
        pat[n_sites - 1] = -1
    return msa, pat


def load_case(case, workdir, h=None):
    """The oracle object of a case.  h: an oracle object of the same base family to reuse (its alignment is replaced)."""
    out = generate_base(case.base, workdir)
    if h is None:
        h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    n, n_sites = h.msa.shape
    assert n == BASES[case.base]["n_leaves"] and n_sites == BASES[case.base]["n_sites"]
    h.msa, h.site_pattern = alignment(case, n, n_sites)
    h._initialize_xmsa_structs()
    return h


def write_case_files(case, workdir):
    """What the host library needs of a case: a copy of the base family's cluster file with the case's alignment written in.
    Returns (the copy's path, the parameter directory)."""
    import json
    out = generate_base(case.base, workdir)
    with open(os.path.join(out, "cluster.yaml")) as f:
        d = json.load(f)
    ev = d["events"][0]
    msa, _ = alignment(case, len(ev["input_seqs"]), len(ev["naive_seq"]))
    ev["input_seqs"] = ["".join("ACGTN"[int(b)] for b in row) for row in msa]
    ev["indel_reversed_seqs"] = ["" for _ in ev["input_seqs"]]
    path = os.path.join(out, "cluster_%s.yaml" % case.name)
    with open(path, "w") as f:
        json.dump(d, f)
    return path, os.path.join(out, "hmm_params")


def expected_info(h, case):
    """What lh_family_info must report: (n_prune, distinct (naive base, pattern) pairs among the xMSA columns)."""
    pairs = {h.xmsa[:, c].tobytes() for c in range(h.xmsa.shape[1])}
    return case.L, len(pairs)


def column_sites(h):
    site = np.zeros(len(h.xmsa_ids), dtype=np.int64)
    base = np.zeros(len(h.xmsa_ids), dtype=np.int64)
    for (b, s), xi in h.xmsa_ids.items():
        site[xi], base[xi] = s, b
    return base, site


def oracle_row(h, sample, R):
    h.initialize_phylo_parameters(sample["tree"], sample["er"], sample["pi"], sample["alpha"], R, is_path=False)
    h.initialize_phylo_emission()
    return h.log_likelihood(), h.xmsa_emission.copy()


def emission_gap(h, em):
    """The smallest relative gap between the emissions of two distinct patterns under the same naive base."""
    base, site = column_sites(h)
    pat = h.site_pattern[site]
    worst = np.inf
    for b in range(5):
        sel = (base == b) & (pat >= 0)
        if sel.sum() < 2:
            continue
        _, first = np.unique(pat[sel], return_index=True)
        e = np.sort(em[sel][first])
        if len(e) >= 2:
            worst = min(worst, float(np.min(np.diff(e) / e[1:])))
    return worst


def check_premises(h, case, loglik, em):
    """The builder's conditions on one oracle row (module docstring).  Returns the figures."""
    msa = h.msa
    distinct = {msa[:, j].tobytes() for j in range(msa.shape[1])}
    all_n = np.full(msa.shape[0], 4, dtype=msa.dtype).tobytes()
    assert (all_n in distinct) == case.all_n, case
    assert len(distinct) - int(case.all_n) == case.L, (case, len(distinct))
    has_n = bool(((msa == 4).any(axis=0) & ~(msa == 4).all(axis=0)).any())
    assert has_n == (case.mixed and case.L > 2), case
    assert np.isfinite(loglik), (case, loglik)
    _, site = column_sites(h)
    read = set(int(p) for p in h.site_pattern[site])
    assert set(range(case.L)) <= read, (case, "a pattern no xMSA column reads")
    assert (em > 0).all() and np.isfinite(em).all(), case
    gap = emission_gap(h, em)
    assert gap > GAP, (case, "two patterns' emissions too close", gap)
    return dict(loglik=float(loglik), min_emission=float(em.min()), gap=gap)


# ---------------------------------------------------------------------------------------------------------------------
# the case lists of the two GPU modules
# ---------------------------------------------------------------------------------------------------------------------

K1_L = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 384, 385, 511, 512, 513, 1023, 1024, 1025)
K1_N_L = (64, 65, 129, 192, 193, 257, 513, 1025)
TREEPASS_L = (63, 64, 255, 256, 257, 511, 512, 1025)


# The tree-pass kernels loop with a lane per pattern over NP = n_prune + 1 in four waves (a second trip from NP = 257) and
# with a lane per site: (case, R).  NP 64, 65, 256, 257, 258, 512, 513, 1026, each without and with the all-N site; the
# 256- and 257-site families for the site loop (1 100 sites: the others); one N-aware case; R = 1 once.
TREEPASS = [(Case("s1100", L, all_n=pad), 4) for L in TREEPASS_L for pad in (False, True)] + \
           [(Case(base, 255, all_n=pad), 4) for base in ("s256", "s257") for pad in (False, True)] + \
           [(Case("s1100", 257, mixed=True), 4), (Case("s1100", 256), 1)]
K3_L = (256, 257)      # lh_asr_batch runs on these alone


def all_cases():
    """Every case either GPU module runs (tests/test_pattern_edge_cases_cpu.py checks the premises of each)."""
    from tests import test_gpu_k1_pattern_edges as k1
    seen, out = set(), []
    for c in [t[0] for t in k1.TABLE] + [t[0] for t in TREEPASS]:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out
