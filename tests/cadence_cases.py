"""TEST INFRASTRUCTURE (CPU only): tree samples on which a LIVE rate category goes subnormal between two rescaling tests of
K1's assembly walk, and references for them that share no rescaling with K1, K2 or oc_eval_batch_ext.

K1's assembly walk tests for the 2^256 rescaling after every fourth walk op and looks at the largest entry of the
conditional-likelihood vector; the C++ walks test after every op.  tests/test_gpu_extreme_parameters.py's rows never let a
category that reaches the mixture fall far between two tests.  Here one does: base frequencies (1e-6, 0.3, 0.3, 0.4) under
F81, alpha = 0.005 with two (three) categories -- the slow category mean is 3.5e-61 (8.6e-41), the fast one saturates every
branch --, some 130-190 leaves, and alignment columns whose background is the rare base A.  In the saturated category every
tip of such a column costs 2^-20, so after 130 tips it lies below the slow category, in which the column costs one
2^-194 (a branch of 100) to 2^-222 (a branch of 1e-6) per mutated tip: the slow category is the live one, the column's
emission is below 2^-1100 -- 0 in the default mode --, and a stretch of mutated tips takes the vector down by that much per
op.  The largest entry stays clear of the subnormals; the entry of the state the NEXT mutated tip needs, some 2^-240 below
it, does not (tests/exact_model_oracle.entry_window_drop).

Families (load_family): tools/synth_family.py's small heavy-chain layout (62 sites, 4 V / 3 D / 3 J alleles) with the
alignment replaced: every site constant at the naive sequence's base except the DEEP sites, placed in the V germline, both
junctions and J.  Trees (tree_newick): ladders written here as Newick over elements of one tip or a cherry of two;
tree "A" joins the tips in order (a ladder stretch, then cherries and tips alternating, then a ladder again), tree "B" joins
them with a stride, so that no two mutated tips of any column are neighbours.

Rows (ROWS: data; classes asserted by check_row on the CPU, on the references alone):
  control  tree and family of the other rows at alpha = 1, every branch 1e-4 of theirs (at the rows' own lengths the
           saturated categories of alpha = 1 put every column of 190 tips below 1e-308: no finite default-mode value to pass
           test_gpu_parity.compare with, which is what a control is for)
  deep     deep columns below 2^-1100; the double-precision restatement of the walk (restate_walk) with the test after every
           op AND after every fourth agrees with the exact per-rate values to 1e-12 in every live category
  lossy    as deep, but with the test after every fourth op a live category is more than 1e-3 off (every op: 1e-12)
  zeroed   with the test after every fourth op a live category's whole vector reaches 0
and for every row: the every-op restatement is unchanged when every entry below 2^-1022 is flushed to 0 on the way (no entry
that matters goes subnormal in a correct every-op walk), and no allele lies more than 2^-900 below its set's best (the
extended-range mode's documented reach).

Joins (family cmp180, rows compound_*).  One 2^256 rescaling per op is enough on a ladder: a tip joining the accumulator falls
by one mismatch.  The product of two subtrees that sit d_a and d_b binades down, with m more for a state mismatch, lies
d_a + d_b + m down, and after ONE rescaling still d_a + d_b + m - 256: more than 256, and the next join doubles it.  The
compound family's tree (compound_newick) is cad190's ladder of background tips, every branch 100, with one balanced block
spliced in as an element: eight four-tip ladders joined pairwise, every branch of the block 1e-6.  On its four deep columns
(V, both junctions, J) every tip holds the rare base A except the block's, whose ladders alternate between (A, A, A, Y) and
(Z, Z, Z, W).  In the live slow category a ladder then sits one mismatch down (2^-222), a pair of ladders three (2^-666;
2^-410 after one rescaling), four ladders 2^-820 (2^-564), and the eight multiply to 2^-1128: 0 in double, where the exact
vector is 2^-2655 at state A with 12 substitutions.  Rescaling UNTIL the largest entry is back at or above 2^-256, each
rescaling counted, keeps every stored vector within [2^-256, 1] and is exact as long as one op's own product stays above
2^-1022 (d_a + d_b + m with both d <= 256: check_row asserts it through the flushed restatement).  Classes:
  compound_control  the tree at alpha = 1 with every branch 1e-4 of its length, as `control`
  compound_clear    tree "D": the same shape with the like ladders joined first, so that the unlike halves meet at the block's
                    last join alone: no vector lies more than 256 down after its rescaling, and both restatements are exact
  compound_lossy    block branches of 1.8e-5 (a mismatch costs 2^-218): with one rescaling per op the last join's product lands in
                    (2^-1074, 2^-1022) and the live category is more than 1e-3 off, finitely; rescale-until is exact
  compound_zeroed   block branches of 1e-6: with one rescaling per op the live category's whole vector is 0; rescale-until is exact

The log-likelihood reference (reference_loglik): every path emits each site once.  The exact emissions E (ExactModel.prune's
log2_emission per (naive base, site)) are brought to benign doubles by one integer k_t per site, the numpy oracle runs its
forward sweep on E 2^k_t, and ln 2 * sum k_t is taken off again.  (The issue's window [2^-200, 1] for a site's five emissions
cannot hold on a deep column: a naive base other than the background costs P_naive(A -> b) pi_A / pi_b = 2^-214 by the model
itself; the window used is [2^-256, 1], still above every rescaling threshold.)  mp_loglik is the same sweep in mpmath with
no scaling at all."""
import json
import math
import os

import numpy as np

from oracle import linearham_oracle as orc
from tests import desc_builder as db
from tests import exact_model_oracle as ex
from tests import k2_scaling_cases as kc

LN2 = math.log(2.0)
ER = [1.0] * 6
PI = [1e-6, 0.3, 0.3, 0.4 - 1e-6]
LONG, SHORT = 100.0, 1e-6
LIVE_BITS = 60
DEEP_LOG2 = -1100.0
EXT_SPREAD_BITS = 900
SITE_WINDOW_BITS = 256
LOSSY_BLOCK = 1.8e-5          # block branches of the compound_lossy row: a mismatch costs 2^-218 instead of SHORT's 2^-222

# name -> (leaves, R, synth seed, elements of tree "A" as (first tip, tips) runs: 1 = ladder tips, 2 = cherry then tip
# alternating, deep columns as (site, first mutated tip, mutated tips))
FAMILIES = {
    "cad190": dict(n_leaves=190, R=2, seed=71, cherries=(120, 160),
                   deep=[(5, 20, 12), (9, 21, 12), (17, 22, 12), (23, 23, 12), (29, 120, 12), (40, 123, 12), (44, 61, 12)]),
    # the compound family (module docstring, "Joins"): block = (first tip, four-tip ladders) of the balanced block; deep
    # columns as (site, which of BLOCK_BASES the block's tips take)
    "cmp180": dict(n_leaves=180, R=2, seed=72, block=(40, 8), deep=[(5, 0), (23, 1), (29, 2), (44, 3)]),
}
# (Y, Z, W) of a deep column of the compound family: ladder j of the block holds (A, A, A, Y) for even j, (Z, Z, Z, W) for odd
BLOCK_BASES = [(1, 2, 3), (2, 3, 1), (3, 1, 2), (1, 3, 2)]
# the block's ladders in the order the balanced tree joins them pairwise: tree "C" as they lie in the alignment (every join
# pairs an (A, A, A, Y) subtree with a (Z, Z, Z, W) one or two like halves), tree "D" the even ladders first (unlike halves
# meet at the block's last join alone)
BLOCK_ORDER = {"C": (0, 1, 2, 3, 4, 5, 6, 7), "D": (0, 2, 4, 6, 1, 3, 5, 7)}

# (name, family, class, tree, alpha, first and last tip of the stretch on short branches or None, length of those branches,
#  factor on every branch)
ROWS = [
    ("control_a", "cad190", "control", "A", 1.0, None, SHORT, 1e-4),
    ("control_b", "cad190", "control", "B", 1.0, None, SHORT, 1e-4),
    ("deep_b", "cad190", "deep", "B", 0.005, None, SHORT, 1.0),
    ("lossy_ladder", "cad190", "lossy", "A", 0.005, (18, 36), SHORT, 1.0),
    ("lossy_long", "cad190", "lossy", "A", 0.005, None, SHORT, 1.0),
    ("lossy_scaled", "cad190", "lossy", "A", 0.005, (59, 75), 1e-4, 1.0),
    ("zeroed_cherries", "cad190", "zeroed", "A", 0.005, (118, 137), SHORT, 1.0),
    # the compound family: trees "C" and "D" (compound_newick); the stretch is unused, the length is the block's branches'
    ("compound_control", "cmp180", "compound_control", "C", 1.0, None, SHORT, 1e-4),
    ("compound_clear", "cmp180", "compound_clear", "D", 0.005, None, SHORT, 1.0),
    ("compound_lossy", "cmp180", "compound_lossy", "C", 0.005, None, LOSSY_BLOCK, 1.0),
    ("compound_zeroed", "cmp180", "compound_zeroed", "C", 0.005, None, SHORT, 1.0),
]
COMPOUND = ("compound_control", "compound_clear", "compound_lossy", "compound_zeroed")


# ---------------------------------------------------------------------------------------------------------------------
# families and trees
# ---------------------------------------------------------------------------------------------------------------------

def family_spec(name):
    from tools import synth_family as sf
    f = FAMILIES[name]
    return sf.Spec.small(n_leaves=f["n_leaves"], n_samples=1, seed=f["seed"], divergence=0.03, v_ancestors=1,
                         d_ancestors=1, j_ancestors=1)


def deep_sites(name):
    return [d[0] for d in FAMILIES[name]["deep"]]


def load_family(name, workdir):
    """The oracle object of a family with the alignment described in the module docstring."""
    from tools import synth_family as sf
    out = os.path.join(str(workdir), name)
    sf.generate(family_spec(name), out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    with open(os.path.join(out, "cluster.yaml")) as f:
        naive = json.load(f)["events"][0]["naive_seq"]
    n, L = h.msa.shape
    assert n == FAMILIES[name]["n_leaves"] and len(naive) == L
    base = np.array(["ACGTN".index(c) for c in naive], dtype=np.int32)
    msa = np.tile(base, (n, 1))
    if "block" in FAMILIES[name]:
        first, ladders = FAMILIES[name]["block"]
        for site, which in FAMILIES[name]["deep"]:
            y, z, w = BLOCK_BASES[which]
            msa[:, site] = 0
            for j in range(ladders):
                msa[first + 4 * j:first + 4 * j + 4, site] = (0, 0, 0, y) if j % 2 == 0 else (z, z, z, w)
    else:
        for site, first, count in FAMILIES[name]["deep"]:
            msa[:, site] = 0
            msa[first:first + count, site] = 1 + np.arange(count) % 3        # C, G, T, C, ...
    h.msa = msa
    h._initialize_xmsa_structs()
    return h


def write_family_files(name, workdir, h):
    """What the host library needs of a family that load_family(name, workdir) returned as `h`: a copy of its cluster file with
    the replaced alignment written in, next to the generated one.  Returns (the copy's path, the parameter directory)."""
    out = os.path.join(str(workdir), name)
    with open(os.path.join(out, "cluster.yaml")) as f:
        d = json.load(f)
    ev = d["events"][0]
    assert ev["unique_ids"] == list(h.xmsa_labels)[1:]
    ev["input_seqs"] = ["".join("ACGTN"[int(b)] for b in row) for row in h.msa]
    ev["indel_reversed_seqs"] = ["" for _ in ev["input_seqs"]]
    path = os.path.join(out, "cluster_replaced.yaml")
    with open(path, "w") as f:
        json.dump(d, f)
    again = orc.PhyloHMM(path, 0, os.path.join(out, "hmm_params"), 0)
    assert np.array_equal(again.msa, h.msa) and np.array_equal(again.xmsa, h.xmsa) and list(again.xmsa_labels) == list(h.xmsa_labels)
    return path, os.path.join(out, "hmm_params")


def elements(name, tree):
    """The ladder's elements, bottom first: tuples of one tip or two (a cherry)."""
    n = FAMILIES[name]["n_leaves"]
    if tree == "B":            # a stride through the tips: neighbours in the alignment are 37 elements apart on the ladder
        assert math.gcd(37, n) == 1
        return [((37 * i) % n,) for i in range(n)]
    lo, hi = FAMILIES[name]["cherries"]
    out, t = [], 0
    while t < n:
        if lo <= t < hi and (t - lo) % 3 == 0 and t + 1 < hi:
            out.append((t, t + 1))
            t += 2
        else:
            out.append((t,))
            t += 1
    return out


def tree_newick(name, tree, short=None, short_len=SHORT, scale=1.0):
    """Newick of the ladder over elements(): ((((e0, e1), e2), e3) ..., naive, e_last).  short = (first tip, last tip): the
    tip branches of those tips, the cherry branches of their cherries and the backbone branches between their elements are
    short_len; every other branch is LONG; all times `scale`."""
    el = elements(name, tree)
    is_short = lambda e: short is not None and all(short[0] <= t <= short[1] for t in e)
    fmt = lambda x: "%.12g" % max(x * scale, 1e-6)

    def text(e):
        b = fmt(short_len if is_short(e) else LONG)
        if len(e) == 1:
            return "s%d:%s" % (e[0], b)
        return "(s%d:%s,s%d:%s):%s" % (e[0], b, e[1], b, b)
    assert len(el[0]) == 1 and len(el[1]) == 1
    node = "(%s,%s)" % (text(el[0]), text(el[1]))
    for k in range(2, len(el) - 1):
        node = "(%s:%s,%s)" % (node, fmt(short_len if is_short(el[k - 1]) and is_short(el[k]) else LONG), text(el[k]))
    return "(%s:%s,naive:%s,%s);" % (node, fmt(LONG), fmt(LONG), text(el[-1]))


def compound_newick(name, tree, block_len=SHORT, scale=1.0):
    """Newick of the compound family's tree: the ladder of tree_newick over the background tips, every branch LONG, with one
    element that is the balanced block -- its four-tip ladders (((t0, t1), t2), t3), the tip that differs last, joined
    pairwise in BLOCK_ORDER[tree]'s order; every branch inside the block and the one above it is block_len; all times
    `scale`."""
    n = FAMILIES[name]["n_leaves"]
    first, ladders = FAMILIES[name]["block"]
    fmt = lambda x: "%.12g" % max(x * scale, 1e-6)
    b, long_ = fmt(block_len), fmt(LONG)
    nodes = []
    for j in BLOCK_ORDER[tree]:
        t = first + 4 * j
        nodes.append("(((s%d:%s,s%d:%s):%s,s%d:%s):%s,s%d:%s)" % (t, b, t + 1, b, b, t + 2, b, b, t + 3, b))
    while len(nodes) > 1:
        nodes = ["(%s:%s,%s:%s)" % (nodes[i], b, nodes[i + 1], b) for i in range(0, len(nodes), 2)]
    el = ["s%d:%s" % (t, long_) for t in range(first)] + ["%s:%s" % (nodes[0], b)] + \
         ["s%d:%s" % (t, long_) for t in range(first + 4 * ladders, n)]
    node = "(%s,%s)" % (el[0], el[1])
    for k in range(2, len(el) - 1):
        node = "(%s:%s,%s)" % (node, long_, el[k])
    return "(%s:%s,naive:%s,%s);" % (node, long_, long_, el[-1])


def sample_of(row):
    name, fam, cls, tree, alpha, short, short_len, scale = row
    if tree in BLOCK_ORDER:
        newick = compound_newick(fam, tree, short_len, scale)
    else:
        newick = tree_newick(fam, tree, short, short_len, scale)
    return dict(tree=newick, er=ER, pi=PI, alpha=float(alpha)), FAMILIES[fam]["R"]


def schedule(h, sample):
    """(T, children, root, brlen, ops, depth) of a sample, the schedule from lh_schedule_tree."""
    import linearham_amd
    T = h.msa.shape[0] + 1
    children, root, brlen = db.tree_arrays(orc.parse_newick(sample["tree"]), h.xmsa_labels)
    ops, depth = linearham_amd.load_library().schedule_tree(T, children, root)
    return T, children, root, brlen, ops, depth


# ---------------------------------------------------------------------------------------------------------------------
# the walk in double precision, with the rescaling test after every w-th walk op
# ---------------------------------------------------------------------------------------------------------------------

def walk_groups(ops, use_tables=True):
    """The schedule ops each WALK op of the cherry-table form executes (K0c's fold rule, lh_prune.hip
    schedule_rewrite_kernel): a cherry that pushes, followed by the pop of its slot, is one op (table into accumulator); a
    cherry followed by a tip-into-accumulator op is one op (table times tip column).  The assembly walk counts walk ops."""
    groups, k, n = [], 0, len(ops)
    while k < n:
        kind, push = int(ops[k][0]) & 15, int(ops[k][0]) & 16
        if use_tables and kind == 0 and k + 1 < n:
            nk = int(ops[k + 1][0]) & 15
            if (push and nk == 2 and ops[k + 1][3] == ops[k][3]) or nk == 1:
                groups.append((k, k + 1))
                k += 2
                continue
        groups.append((k,))
        k += 1
    return groups


def restate_walk(T, ops, pats, P, pi, w, use_tables=True, flush=False, until=False):
    """K1's walk in numpy doubles over the schedule `ops`, all patterns at once.  pats [T-1, n] tip states (4 = N), P
    [2T-2, R, 4, 4] the P-matrix above every node.  The 2^256 test looks at the LARGEST entry, after every w-th walk op
    and after the last: w = 1 rescales once per test (the C++ walks), w > 1 until the largest entry is back above 2^-256
    or has a zero high word (the assembly walk); w = 1 with until: after every op, rescaled until the largest entry is back
    at or above 2^-256, each rescale counted (what a join of two subtrees needs -- module docstring, "Joins").  This is the
    device's arithmetic (lh_device.h rescale_steps) wherever the largest entry an op leaves is a normal number; where it is
    subnormal -- bits are lost already: outside the mode's reach, and check_row asserts through `flush` that no row gets
    there -- the device reads the count off the exponent field alone: three for [2^-1042, 2^-1022), where this loop makes
    four below 2^-1024, and one for a zero high word, where this loop goes on unless the vector is 0.
    flush: every entry below 2^-1022 is set to 0 after each op.
    Returns log2 [R, 5, n] of the per-rate site likelihood by naive state (counts taken off), zeroed [R, n]: the whole
    vector was 0 after some op, low [R, n]: log2 of the smallest positive entry any op left, top_low [R, n]: log2 of the
    smallest positive LARGEST entry any op left (before its rescaling)."""
    R, n = P.shape[1], pats.shape[1]
    groups = walk_groups(ops, use_tables)
    onehot = np.concatenate([np.eye(4), np.ones((1, 4))], axis=0)
    out, zeroed, low = np.zeros((R, 5, n)), np.zeros((R, n), bool), np.full((R, n), np.inf)
    top_low = np.full((R, n), np.inf)
    thr, fac = 2.0 ** -256, 2.0 ** 256
    with np.errstate(all="ignore"):
        for r in range(R):
            tip = lambda t: P[t, r] @ onehot[pats[t - 1]].T          # [4, n]
            acc, stack, count = None, {}, np.zeros(n, dtype=np.int64)
            for wi, g in enumerate(groups):
                for k in g:
                    op = [int(x) for x in ops[k]]
                    kind = op[0] & 15
                    if op[0] & 16:
                        stack[op[3]] = acc
                    if kind == 0:
                        acc = tip(op[1]) * tip(op[2])
                    elif kind == 1:
                        acc = tip(op[1]) * (P[op[2], r] @ acc)
                    else:
                        acc = (P[op[1], r] @ stack[op[3]]) * (P[op[2], r] @ acc)
                if flush:
                    acc = np.where(acc < 2.0 ** -1022, 0.0, acc)
                pos = np.where(acc > 0, acc, np.inf).min(axis=0)
                low[r] = np.minimum(low[r], pos)
                zeroed[r] |= acc.max(axis=0) == 0
                top_low[r] = np.minimum(top_low[r], np.where(acc.max(axis=0) > 0, acc.max(axis=0), np.inf))
                if wi % w == w - 1 or wi == len(groups) - 1:
                    need = acc.max(axis=0) < thr                     # (an all-zero vector is rescaled once and left)
                    while need.any():
                        acc = np.where(need, acc * fac, acc)
                        count += need
                        if w == 1 and not until:
                            break
                        mx = acc.max(axis=0)
                        need = (mx < thr) & (mx >= 2.0 ** -1042)    # a zero high word counts as nothing left
            wgt = np.asarray(pi)[:, None] * acc
            for b in range(5):
                lik = (wgt * (P[0, r] @ onehot[b])[:, None]).sum(axis=0)
                out[r, b] = np.log2(lik) - 256.0 * count
    return {"log2": out, "zeroed": zeroed, "low": np.log2(low), "top_low": np.log2(top_low)}


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def exact_row(h, sample, R, entries=True):
    """The exact side of a row: ExactModel.prune over every xMSA column, with the schedule and the P-matrices in double."""
    T, children, root, brlen, ops, depth = schedule(h, sample)
    rates = ex.gamma_rates_mean(sample["alpha"], R, as_double=False)
    model = ex.ExactModel(sample["er"], sample["pi"], rates)
    cols = np.arange(h.xmsa.shape[1])
    pr = model.prune(T, children, root, brlen, h.xmsa, cols, entries=entries)
    pr.update(T=T, children=children, root=root, brlen=brlen, ops=ops, depth=depth, P=model.pmatrices_double(brlen),
              rates=np.array([float(x) for x in rates]))
    return pr


def site_shifts(h, log2e):
    """One integer k_t per site with max over the site's columns of E 2^k_t in (1/2, 1]."""
    site = kc.column_sites(h)
    k = np.zeros(int(site.max()) + 1, dtype=np.int64)
    for t in range(len(k)):
        k[t] = -int(math.ceil(log2e[site == t].max()))
    shifted = log2e + k[site]
    assert shifted.max() <= 0 and shifted.min() >= -SITE_WINDOW_BITS, (shifted.min(), shifted.max())
    return site, k, shifted


def reference_loglik(h, log2e):
    """The column-scaling identity on the exact emissions (module docstring)."""
    site, k, shifted = site_shifts(h, log2e)
    ll = kc.oracle_eval(h, np.exp2(shifted))["loglik"]
    return ll - LN2 * float(k.sum())


def mp_loglik(h, log2e, dps=50):
    """The dense forward sweep of the numpy oracle in mpmath on the emissions 2^log2e themselves: no scaling anywhere."""
    import mpmath as mp
    with mp.workdps(dps):
        E = np.array([mp.power(2, mp.mpf(float(x))) for x in log2e], dtype=object)
        obj = lambda a: np.vectorize(mp.mpf, otypes=[object])(np.asarray(a, dtype=float))

        def fill_gp(R, inds):
            out = []
            for g in sorted(R.ggene_ranges):
                rs, re_ = R.ggene_ranges[g]
                v = mp.mpf(1)
                for j in range(rs, re_):
                    v *= E[inds[j]]
                out.append(v)
            return np.array(out, dtype=object)

        def fill_junction(inds):
            M = np.full(inds.shape, mp.mpf(0), dtype=object)
            M[inds != -1] = E[inds[inds != -1]]
            return M

        def junction(gf, T_gj, T_jj, Em):
            row = (gf @ obj(T_gj)) * Em[0]
            Tj = obj(T_jj)
            for i in range(1, Em.shape[0]):
                row = (row @ Tj) * Em[i]
            return row
        vp, vg = fill_gp(h.vpadding, h.vpadding_xmsa_inds), fill_gp(h.vgerm, h.vgerm_xmsa_inds)
        f = []
        for i, g in enumerate(sorted(h.vgerm.ggene_ranges)):
            rs, re_ = h.vgerm.ggene_ranges[g]
            gg = h.ggenes[g]
            gis = h.vgerm.germ_inds[rs]
            f.append(mp.mpf(float(gg.gene_prob)) * mp.mpf(float(h.vpadding_transition[i])) * vp[i] *
                     mp.mpf(float(np.prod(gg.transition[gis:gis + (re_ - rs - 1)]))) * vg[i])
        f = np.array(f, dtype=object)
        assert h.locus == "igh"
        row = junction(f, h.vgerm_vd_junction_transition, h.vd_junction_transition, fill_junction(h.vd_junction_xmsa_inds))
        d = (row @ obj(h.vd_junction_dgerm_transition)) * fill_gp(h.dgerm, h.dgerm_xmsa_inds)
        row = junction(d, h.dgerm_dj_junction_transition, h.dj_junction_transition, fill_junction(h.dj_junction_xmsa_inds))
        j = (row @ obj(h.dj_junction_jgerm_transition)) * fill_gp(h.jgerm, h.jgerm_xmsa_inds) * obj(h.jpadding_transition) * \
            fill_gp(h.jpadding, h.jpadding_xmsa_inds)
        return float(mp.log(sum(j)))


def ext_spread_bits(h, log2e):
    """How far, in bits, the smallest product of a germline or padding set lies below that set's largest."""
    worst = 0.0
    for name in kc.SETS:
        R, inds = getattr(h, name), getattr(h, name + "_xmsa_inds")
        tot = []
        for g in sorted(R.ggene_ranges):
            rs, re_ = R.ggene_ranges[g]
            tot.append(float(sum(log2e[inds[j]] for j in range(rs, re_))))
        if tot:
            worst = max(worst, max(tot) - min(tot))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------------------------------------------------

def relative_deviation(log2_a, log2_b):
    """|a / b - 1| from the two base-2 logarithms (inf where a is 0 or not a number and b is not)."""
    with np.errstate(all="ignore"):
        d = np.abs(np.expm1((np.asarray(log2_a) - np.asarray(log2_b)) * LN2))
    return np.where(np.isnan(d), np.inf, d)


def analyse_row(h, row, exact=None):
    """Everything check_row asserts on and the profile file prints, from the references alone."""
    sample, R = sample_of(row)
    x = exact if exact is not None else exact_row(h, sample, R)
    T, ops = x["T"], x["ops"]
    site = kc.column_sites(h)
    deep_cols = np.nonzero(np.isin(site, deep_sites(row[1])))[0]
    naive = h.xmsa[0]
    per_rate = x["per_rate_log2"]                                        # [R, C]
    live = per_rate >= per_rate.max(axis=0, keepdims=True) - LIVE_BITS
    pats = np.zeros((T - 1, int(x["pattern_of"].max()) + 1), dtype=np.int64)
    pats[:, x["pattern_of"]] = h.xmsa[1:]
    dev, zeroed, walks = {}, {}, {}
    for tag, w, tables, flush, until in (("w1", 1, True, False, False), ("w4", 4, True, False, False),
                                         ("w4_no_tables", 4, False, False, False), ("w1_flush", 1, True, True, False),
                                         ("u1", 1, True, False, True), ("u1_no_tables", 1, False, False, True),
                                         ("u1_flush", 1, True, True, True)):
        rs = restate_walk(T, ops, pats, x["P"], sample["pi"], w, use_tables=tables, flush=flush, until=until)
        got = rs["log2"][:, naive, x["pattern_of"]]                     # [R, C]
        d = np.where(live, relative_deviation(got, per_rate), 0.0)
        dev[tag] = d
        zeroed[tag] = bool((rs["zeroed"][:, x["pattern_of"]] & live).any())
        walks[tag] = rs
    top = ex.four_op_drop(T, x["children"], ops, x["node_log2max"], window=4, live_within=LIVE_BITS)
    ent = ex.entry_window_drop(T, x["children"], ops, x["node_log2"], window=4, matters_within=LIVE_BITS)
    ent = ent[:, :, x["pattern_of"]]                                     # [ops, R, C, 4]
    ent = np.where(live[None, :, :, None], ent, np.nan)
    out = dict(name=row[0], cls=row[2], R=R, depth=int(x["depth"]), deep_cols=deep_cols,
               log2_emission=x["log2_emission"], deepest=float(x["log2_emission"][deep_cols].max()),
               live_slow=bool(live[0][deep_cols].all() and not live[1:][:, deep_cols].any()),
               dev={k: float(v.max()) for k, v in dev.items()}, dev_cols=dev, zeroed=zeroed,
               low_w1=float(np.where(live, walks["w1"]["low"][:, x["pattern_of"]], np.inf).min()),
               join_low_w1=float(np.where(live, walks["w1"]["top_low"][:, x["pattern_of"]], np.inf).min()),
               join_low_u1=float(np.where(live, walks["u1"]["top_low"][:, x["pattern_of"]], np.inf).min()),
               four_op_fall=float(top), entry_fall=float(np.nanmin(ent)) if np.isfinite(ent).any() else 0.0,
               spread=ext_spread_bits(h, x["log2_emission"]), walk_ops=len(walk_groups(ops)), live=live, exact=x)
    return out


def check_row(a):
    """The conditions of the row's class (module docstring)."""
    name, cls, dev = a["name"], a["cls"], a["dev"]
    assert a["depth"] <= 4, (name, "the default form must be the fused cherry-table kernel of depth <= 4", a["depth"])
    assert a["spread"] <= EXT_SPREAD_BITS, (name, "an allele beyond the extended-range mode's reach", a["spread"])
    # rescale-until is the arithmetic the device has: exact on every row, with and without cherry tables, and no entry that
    # matters goes subnormal on the way (the residual reach: one op's own product stays above 2^-1022)
    assert dev["u1"] <= 1e-12 and dev["u1_no_tables"] <= 1e-12, (name, "the rescale-until restatement is not the exact value", dev["u1"])
    assert dev["u1_flush"] <= 1e-12 and not a["zeroed"]["u1"], (name, "an op's product goes subnormal in the rescale-until walk", dev["u1_flush"])
    if cls in ("compound_lossy", "compound_zeroed"):
        assert a["deepest"] < DEEP_LOG2, (name, "a deep column above 2^-1100", a["deepest"])
        assert a["live_slow"], (name, "the slow category alone must be live on the deep columns")
        if cls == "compound_zeroed":
            assert a["zeroed"]["w1"], (name, "no live category's vector reaches 0 with one rescale per op")
        else:
            assert not a["zeroed"]["w1"] and 1e-3 < dev["w1"] < np.inf, (name, "one rescale per op is not finitely off", dev["w1"])
            assert -1074 < a["join_low_w1"] < -1022, (name, "no join's product in (2^-1074, 2^-1022)", a["join_low_w1"])
        return
    assert dev["w1"] <= 1e-12, (name, "the every-op restatement is not the exact value", dev["w1"])
    assert dev["w1_flush"] <= 1e-12 and not a["zeroed"]["w1"], (name, "an entry that matters goes subnormal in the every-op walk", dev["w1_flush"])
    if cls == "compound_clear":                 # the tree's shape alone is harmless: one rescale per op is exact as well
        assert a["deepest"] < DEEP_LOG2 and a["live_slow"], (name, a["deepest"])
        assert a["join_low_w1"] > -1022, (name, a["join_low_w1"])
        return
    if cls in ("control", "compound_control"):
        assert dev["w4"] <= 1e-12 and a["log2_emission"].min() > -900, (name, dev["w4"], a["log2_emission"].min())
        return
    assert a["deepest"] < DEEP_LOG2, (name, "a deep column above 2^-1100", a["deepest"])
    assert a["live_slow"], (name, "the slow category alone must be live on the deep columns")
    if cls == "deep":
        assert dev["w4"] <= 1e-12 and dev["w4_no_tables"] <= 1e-12, (name, dev)
    elif cls == "lossy":
        assert dev["w4"] > 1e-3, (name, "the every-fourth-op restatement is not off", dev["w4"])
    else:
        assert a["zeroed"]["w4"], (name, "no live category's vector reaches 0 with the test after every fourth op")


def _analyse(args):
    """One row in a pool process: the family is generated again there (deterministic, half a second).  Returns the analysis
    and the seconds it took (the exact side -- mpmath pruning -- and the restatements)."""
    import shutil
    import tempfile
    import time
    name, row = args
    work = tempfile.mkdtemp(prefix="lh_cadence_")
    try:
        h = load_family(name, work)
        t0 = time.perf_counter()
        a = analyse_row(h, row)
        return a, time.perf_counter() - t0
    finally:
        shutil.rmtree(work, ignore_errors=True)


def build_families(names, workdir, jobs=1):
    """{name: (h, [(row, analysis)], seconds)} of the families, every row checked; jobs > 1: the rows of all families on one
    pool of processes.  seconds: the family's rows' analyses, summed."""
    import time
    hs = {name: load_family(name, workdir) for name in names}
    todo = [(row[1], row) for row in ROWS if row[1] in names]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            done = pool.map(_analyse, todo)
    else:
        done = []
        for name, row in todo:
            t0 = time.perf_counter()
            done.append((analyse_row(hs[name], row), time.perf_counter() - t0))
    out = {name: (hs[name], [], 0.0) for name in names}
    for (name, row), (a, sec) in zip(todo, done):
        check_row(a)
        h, rows, total = out[name]
        out[name] = (h, rows + [(row, a)], total + sec)
    return out


def build_family(name, workdir, jobs=1):
    """(h, [(row, analysis)]) of one family, every row checked."""
    h, rows, _ = build_families([name], workdir, jobs)[name]
    return h, rows
