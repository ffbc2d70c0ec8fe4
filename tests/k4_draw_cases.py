"""TEST INFRASTRUCTURE (CPU only): rows that put unlike work into one wave of K4 (lh_sample.hip: four samples per wave,
sixteen lanes each, a chunk mask and two early exits shared by the wave), and their references.

Rows.  The emission vectors are the cases of tests/k2_scaling_cases.py (zero columns, rows three rescalings deep, the
reference's overflowed equalisation `delta4`); the engine words are eight patterns (PATTERNS: a uniform of exactly 0, the
largest below 1 by two routes, the smallest above 0, a random mix of the extremes, three random streams).  With |C| cases,
row c + |C| j carries case c and pattern (c + j) mod 8 for j = 0..7 and one more row (case 0, pattern 0) follows: every
case meets every pattern, the four rows of a wave differ in emissions AND in words, n = 8 |C| + 1 and the last wave holds
one row.

References.  Tier 1 (every row, exact): the oracle's own dense draw functions -- discrete_distribution_draw,
sample_junction_states, sample_germline_state over the oracle object's dense transition matrices -- on GIVEN forward
arrays (the device's, expanded to the dense shapes): draws_on_forward.  The weights are then bit-identical by construction
(K4 rebuilds every transition value with fill_transition's association) and the states must be equal on every row.
Tier 2 (independent of K2): the oracle end to end on its own forward arrays (draws_end_to_end), on the rows with a random
stream and a finite case.  Those arrays agree with the device's to the 1e-9 the suite asserts, so a row qualifies only if,
in every draw, the uniform is further than MARGIN_RTOL = 1e-7 relative (a hundred times that bound) from every partial sum
at which the answer changes (the partial sums in front of a positive weight, and the last one); STREAM_SEEDS are chosen so
that every such row qualifies (tests/test_k4_draw_cases_cpu.py asserts it: a seed that fails is replaced, never exempted).

classes() counts, on recorded draws, what the rows are there for -- (a) to (f) of the CPU test's docstring."""
import math

import numpy as np

from oracle import linearham_oracle as orc
from tests import k2_scaling_cases as kc
from tests import viterbi_oracle as vo

FAMILIES = ("toy", "small_igh", "small_igk", "igh_70_33_5", "igh_v130_d30_j12", "igh_v260", "igh_d65", "igk_v70_j70")
PATTERNS = ("zeros", "ones", "lo1", "hi1", "mix", "random0", "random1", "random2")
RANDOM_PATTERNS = (5, 6, 7)
MARGIN_RTOL = 1e-7
kG = 16                     # lanes per sample in K4: genes per chunk
SAVE_LIMIT = 256            # launch_sample keeps a draw's weights in LDS up to this many genes (rounded up to kG)
# seeds of (mix, random0, random1, random2) per family: every tier-2 row keeps MARGIN_RTOL (check_margins)
STREAM_SEEDS = {name: 100 + 10 * i for i, name in enumerate(FAMILIES)}


# ---------------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------------

def draw_sizes(h):
    """dense vector length of every draw of a sample, in the order the draws are made: J genes | D-J rows W-1..0 | D genes
    | V-D rows W-1..0 | V genes (light chains: J genes | V-J rows | V genes)"""
    sizes = [len(h.jgerm.state_strs)]
    if h.locus == "igh":
        sizes += [len(h.dj_junction.state_strs)] * _rows(h, "d_r", "j_l") + [len(h.dgerm.state_strs)]
        sizes += [len(h.vd_junction.state_strs)] * _rows(h, "v_r", "d_l")
    else:
        sizes += [len(h.vd_junction.state_strs)] * _rows(h, "v_r", "j_l")
    return sizes + [len(h.vgerm.state_strs)]


def _rows(h, left, right):
    return h.flexbounds[right][1] - h.flexbounds[left][0]


def words_per_sample(h):
    """lh_sample_words from the structure: two engine outputs per region or junction row with more than one state"""
    return 2 * sum(1 for s in draw_sizes(h) if s > 1)


def widest_draw(h):
    """the widest block of genes K4 spreads over its lanes, rounded up to whole chunks (launch_sample's `widest`)"""
    w = [len(h.vgerm.state_strs), len(h.jgerm.state_strs)]
    if h.locus == "igh":
        w.append(len(h.dgerm.state_strs))
    return (max(w) + kG - 1) // kG * kG


def saves_weights(h):
    """launch_sample's rule for save_cap: the saved form up to SAVE_LIMIT genes, the recompute form beyond"""
    return widest_draw(h) <= SAVE_LIMIT


def blocks(h):
    """per draw (draw_sizes' order): the dense indices of the genes K4 spreads over its lanes, in lane order (-1: the gene
    has no state on that junction row) -- the whole vector for a germline region, the left genes' states for a junction row"""
    def junction(J, G_left, W):
        left = sorted(G_left.ggene_ranges)
        out = []
        for i in range(W - 1, -1, -1):
            out.append(np.array([J.ggene_ranges[g][0] + i if i < J.ggene_ranges[g][1] - J.ggene_ranges[g][0] else -1
                                 for g in left], dtype=np.int64))
        return out
    out = [np.arange(len(h.jgerm.state_strs))]
    if h.locus == "igh":
        out += junction(h.dj_junction, h.dgerm, _rows(h, "d_r", "j_l")) + [np.arange(len(h.dgerm.state_strs))]
        out += junction(h.vd_junction, h.vgerm, _rows(h, "v_r", "d_l"))
    else:
        out += junction(h.vd_junction, h.vgerm, _rows(h, "v_r", "j_l"))
    return out + [np.arange(len(h.vgerm.state_strs))]


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------

def patterns(n_words, seed):
    """[8][n_words] uint32: PATTERNS"""
    rng = np.random.default_rng(seed)
    lo1 = np.zeros(n_words, np.uint32)
    lo1[0::2] = 1                                  # the smallest positive uniform
    hi1 = np.full(n_words, 0xFFFFFFFF, np.uint32)
    hi1[0::2] = 0xFFFFF800                         # rounds to just below 1
    mix = np.where(rng.integers(0, 2, n_words) == 1, 0xFFFFFFFF, 0).astype(np.uint32)
    rand = [rng.integers(0, 2 ** 32, n_words, dtype=np.uint64).astype(np.uint32) for _ in RANDOM_PATTERNS]
    return np.stack([np.zeros(n_words, np.uint32), np.full(n_words, 0xFFFFFFFF, np.uint32), lo1, hi1, mix] + rand)


def layout(n_cases):
    """[(case index, pattern index)] of the n = 8 |C| + 1 rows"""
    rows = [(c, (c + j) % 8) for j in range(8) for c in range(n_cases)]
    return rows + [(0, 0)]


class Rows:
    """The rows of one family: cases, em [n][C], words [n][NW], (case, pattern) per row."""

    def __init__(self, name, h, cases, seed=None):
        self.name, self.cases = name, cases
        self.n_words = words_per_sample(h)
        self.patterns = patterns(self.n_words, STREAM_SEEDS[name] if seed is None else seed)
        self.layout = layout(len(cases))
        self.em = np.stack([cases[c].em for c, _ in self.layout])
        self.words = np.stack([self.patterns[p] for _, p in self.layout])
        self.n = len(self.layout)
        assert self.n == 8 * len(cases) + 1 and self.n % 4 == 1

    def tier2_rows(self):
        return [r for r, (c, p) in enumerate(self.layout) if p in RANDOM_PATTERNS and self.cases[c].expect == "finite"]


def build_rows(name, workdir, seed=None):
    h = kc.load_family(name, workdir)
    _, cases = kc.build_cases(h, kc.SEEDS[name])
    return h, Rows(name, h, cases, seed)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

class _Engine:
    """the row's words in order, as the callable the oracle's draws take"""

    def __init__(self, words):
        self.words, self.used = [int(w) for w in words], 0

    def __call__(self):
        self.used += 1
        return self.words[self.used - 1]


def _sample(h, words, record):
    """h.sample_naive_sequence() with the engine replaced -> (states in K4's layout, words consumed, recorded draws).
    A recorded draw is dict(w = the dense weight vector, p = the uniform or None, k = the element drawn)."""
    eng = _Engine(words)
    draws = []
    plain = orc.discrete_distribution_draw

    def recording(weights, rng):
        before = eng.used
        k = plain(weights, rng)
        p = None
        if eng.used > before:
            pair = iter(eng.words[before:eng.used])
            p = orc.generate_canonical(lambda: next(pair))
        draws.append(dict(w=np.array(weights, dtype=float), p=p, k=int(k)))
        return k
    old_rng = h.rng
    h.rng = eng
    if record:
        orc.discrete_distribution_draw = recording
    try:
        with np.errstate(all="ignore"):
            h.sample_naive_sequence()
    finally:
        orc.discrete_distribution_draw = plain
        h.rng = old_rng
    s = h.sample
    if h.locus == "igh":
        st = [s["jgerm_state_ind_samp"]] + list(s["dj_junction_state_ind_samps"]) + [s["dgerm_state_ind_samp"]] + \
            list(s["vd_junction_state_ind_samps"]) + [s["vgerm_state_ind_samp"]]
    else:
        st = [s["jgerm_state_ind_samp"]] + list(s["vd_junction_state_ind_samps"]) + [s["vgerm_state_ind_samp"]]
    return np.array(st, dtype=np.int32), eng.used, draws


def draws_on_forward(h, forward, words, record=False):
    """Tier 1: the oracle's dense draws on the forward arrays `forward` (a dict with the *_forward members of
    k2_scaling_cases.FORWARD_KEYS, dense shapes)."""
    for k in kc.FORWARD_KEYS:
        if k in forward:
            setattr(h, k, np.asarray(forward[k], dtype=float))
    h.cache_forward = False
    return _sample(h, words, record)


def draws_end_to_end(h, em, words, record=False):
    """Tier 2: emissions -> the oracle's own forward sweep -> its draws."""
    vo.set_emissions(h, em)
    h.cache_forward = True
    return _sample(h, words, record)


def margin(draw):
    """the smallest relative distance of the draw's uniform from a partial sum at which the answer changes: the (positive)
    partial sums in front of a positive weight, and the last one before libstdc++ sets it to 1; inf for a draw that takes
    no words.  A partial sum of exactly 0 (leading structural zeros) is the same on both sides and is left out."""
    w, p = draw["w"], draw["p"]
    if p is None:
        return math.inf
    total = 0.0
    for x in w:
        total += float(x)
    acc, cp = 0.0, []
    for x in w:
        acc += orc._ieee_div(float(x), total)
        cp.append(acc)
    cp = np.array(cp)
    edge = np.concatenate([cp[:-1][w[1:] > 0], cp[-1:]])
    edge = edge[edge > 0]
    if not np.all(np.isfinite(edge)):
        return 0.0
    return float(np.min(np.abs(p - edge) / edge)) if edge.size else math.inf


def check_margins(h, rows):
    """-> (worst margin over the tier-2 rows, {row: states}); raises if a tier-2 row does not keep MARGIN_RTOL"""
    worst, states = math.inf, {}
    for r in rows.tier2_rows():
        st, used, draws = draws_end_to_end(h, rows.em[r], rows.words[r], record=True)
        assert used == rows.n_words
        m = min(margin(d) for d in draws)
        c, p = rows.layout[r]
        assert m > MARGIN_RTOL, ("%s: row %d (case %s, pattern %s) has a uniform %.3e relative from a partial sum: replace "
                                 "the family's seed in STREAM_SEEDS" % (rows.name, r, rows.cases[c].name, PATTERNS[p], m))
        worst = min(worst, m)
        states[r] = st
    return worst, states


# ---------------------------------------------------------------------------------------------------------------------
# what the rows are for
# ---------------------------------------------------------------------------------------------------------------------

def classes(h, rows, recorded):
    """recorded: per row the draws of a reference run (tier 1 or the oracle's own).  Counts
      a  draws (of more than one element) with no positive weight                         [a_finite: in a finite row]
      b  draws beyond the last partial sum that return the dense vector's last element   [b_zero: which has zero weight]
      c  drawn states of zero weight that a later draw of the row follows
      d  (wave, draw) pairs whose rows find their answers in different 16-gene chunks    [d_max: most chunks in one pair]
      e  (wave, draw) pairs with a chunk all zero in one row and not in another          [e_zero: one of the two a `zero` row]
      f  waves that hold a non-finite row (delta4) beside finite rows"""
    out = dict(a=0, a_finite=0, b=0, b_zero=0, c=0, d=0, d_max=0, e=0, e_zero=0, f=0)
    blk = blocks(h)
    case_of = [rows.cases[c] for c, _ in rows.layout]
    for r, draws in enumerate(recorded):
        assert len(draws) == len(blk)
        for i, d in enumerate(draws):
            w, p, k = d["w"], d["p"], d["k"]
            if p is None:
                continue
            positive = w > 0
            if not positive.any():
                out["a"] += 1
                out["a_finite"] += bool(np.all(np.isfinite(w)))
            else:
                total = 0.0
                for x in w:
                    total += float(x)
                acc = 0.0
                for x in w:
                    acc += orc._ieee_div(float(x), total)
                if np.isfinite(total) and acc < p and k == len(w) - 1:   # (partial sums never fall: the last is the largest)
                    out["b"] += 1
                    out["b_zero"] += bool(w[-1] == 0)
            if not w[k] > 0 and i + 1 < len(draws):
                out["c"] += 1
    for w0 in range(0, rows.n, 4):
        wave = list(range(w0, min(w0 + 4, rows.n)))
        finite = [case_of[r].expect == "finite" for r in wave]
        out["f"] += bool(any(finite) and not all(finite))
        for i, idx in enumerate(blk):
            chunks, masks = set(), []
            valid = idx >= 0
            for r in wave:
                d = recorded[r][i]
                if d["p"] is None:
                    continue
                at = np.nonzero(idx == d["k"])[0]
                if at.size:
                    chunks.add(int(at[0]) // kG)
                wb = np.where(valid, d["w"][np.where(valid, idx, 0)], 0.0)
                pad = (-len(wb)) % kG
                nz = (np.concatenate([wb, np.zeros(pad)]) != 0).reshape(-1, kG).any(axis=1)   # (NaN != 0: a weight)
                masks.append((nz, case_of[r].name == "zero"))
            if len(chunks) > 1:
                out["d"] += 1
            out["d_max"] = max(out["d_max"], len(chunks))
            hit = hit_zero = False
            for a, (na, za) in enumerate(masks):
                for nb, zb in masks[a + 1:]:
                    if np.any(na != nb):
                        hit = True
                        hit_zero = hit_zero or za or zb
            out["e"] += hit
            out["e_zero"] += hit_zero
    return out
