"""K2, K5 and K6 at the shapes where their launch code chooses differently, against the oracle.

  * A long alignment (1 733 distinct columns): n_ucol = 5 n_prune + 5 is above 8 190, so K2's index chunks hold
    plain indices instead of byte offsets (kByteOff = false, lh_device.h) and K2a's emission vector takes more than
    64 KB of LDS.
  * K6b's three score_kernel launches (n_vlem = 1 024 | 1 025, 8 192 | 8 193), its grid edges (K = 1, 256, 257, 513, n
    not a multiple of 8, two slabs of rows) and K6a's groups of 4 096 candidates.
  * K5 past its first 16-row workgroup, and K5 / K6 on the junction shapes of unequal 64-gene chunk counts and a seeded
    sweep of allele counts across the chunk edges.
Candidates are drawn from the HMM's prior (naive_probs_oracle.prior_draws), so they are spread out and have finite
priors; every one is checked in two parts: its prior against constrained_log_prior, and log_cand - prior + loglik
against the oracle's sum of log emissions, which isolates K6b's gather."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from linearham_amd import host
from linearham_amd.capi import load_library
from oracle import linearham_oracle as orc
from tests import naive_probs_oracle as npo
from tests import posterior_oracle as po
from tests import test_gpu_parity as tp
from tests.test_gpu_naive_probs import _impossible, _tol

pytestmark = pytest.mark.gpu

# 1 733 distinct alignment columns (n_prune > 1 637); the allele sets stay nearly identical, since more divergence or
# more alleles make the oracle's own rows overflow
LONG = dict(n_leaves=48, n_sites=1900, len_v=1780, n_v=3, n_d=2, n_j=2, divergence=0.01, brlen_mean=0.15, n_samples=4)
BYTE_OFF_LIMIT = 1637           # the largest n_prune whose u-columns fit 16-bit byte offsets
UNEQUAL = [dict(n_v=289, n_d=65, n_j=30, n_leaves=7, ragged=10, ambiguous=0.05, divergence=0.3, seed=13358),
           dict(n_v=70, n_d=65, n_j=30, seed=61), dict(n_v=70, n_d=20, n_j=70, seed=62),
           dict(n_v=130, n_d=140, n_j=10, seed=63), dict(n_v=40, n_d=3, n_j=200, seed=64)]
UNEQUAL_IDS = ["sweep13358", "d65_j30", "d20_j70", "d140_j10", "d3_j200"]   # test_gpu_parity's unequal-chunk shapes


@pytest.fixture(scope="module")
def hip():
    lib = load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


class Fam:
    """A generated family: oracle, host handle, its flattened rows (the family handle K5 and K6 run on)."""

    def __init__(self, out, spec, n=None, seed=0):
        from tools import synth_family as sf
        sf.generate(spec, out)
        self.yaml, self.pdir, self.tsv = (os.path.join(out, x) for x in ("cluster.yaml", "hmm_params", "trees.tsv"))
        self.rows = sf.read_trees_tsv(self.tsv)
        self.o = orc.PhyloHMM(self.yaml, 0, self.pdir, seed)
        self.h = host.PhyloHMM(self.yaml, 0, self.pdir, seed)
        self.n = len(self.rows) if n is None else n
        self.fl = self.h.flatten_tsv(self.tsv, self.n)
        self.row(0, 4)   # (prior_draws and constrained_log_prior read the oracle's tables, filled by a first row)

    def row(self, i, R):
        """Sets the oracle to row i (cyclic, as flatten_tsv takes them) and returns its log-likelihood."""
        r = self.rows[i % len(self.rows)]
        self.o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        self.o.initialize_phylo_emission()
        return self.o.log_likelihood()

    def args(self, R, sl=slice(None)):
        fl = self.fl
        return (fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"][sl], fl["brlen"][sl], fl["er"][sl], fl["pi"][sl],
                fl["alpha"][sl], R)

    def set_extended_range(self, hip, on):
        hip.check(hip.lib.lh_family_set_extended_range(C.c_void_p(self.fl["family"]), int(on)))


@pytest.fixture(scope="module")
def long_fam(tmp_path_factory):
    from tools import synth_family as sf
    fam = Fam(str(tmp_path_factory.mktemp("long") / "fam"), sf.Spec(**LONG))
    assert len({fam.o.msa[:, i].tobytes() for i in range(fam.o.msa.shape[1])}) >= BYTE_OFF_LIMIT + 2
    return fam


@pytest.fixture(scope="module")
def small_fam(tmp_path_factory):
    from tools import synth_family as sf
    return Fam(str(tmp_path_factory.mktemp("small") / "fam"), sf.Spec.small(n_samples=257), n=257)


def _distinct_draws(o, n, seed, at_least=None):
    """n distinct prior draws (at least `at_least` where the prior has fewer), in the order they were first drawn."""
    rng = np.random.default_rng(seed)
    d = npo.prior_draws(o, 4 * n + 64, rng)
    _, first = np.unique(d, axis=0, return_index=True)
    d = d[np.sort(first)]
    assert len(d) >= (n if at_least is None else at_least), "the prior gave %d distinct sequences" % len(d)
    return d[:n]


def check_candidates(hip, fam, cands, R=4, sl=slice(None), want_layout=None, want_prior=None):
    """Registers cands, checks the layout against the host restatement, every distinct candidate's prior against the
    oracle (or, want_prior given, against those bits), then evaluates the rows sl and checks log_cand of every (row,
    candidate): impossible candidates exactly -inf, the others log_cand - prior + loglik against the oracle's
    log-emission sum.  Rows the oracle overflows must be non-finite on the device too.  Returns (prior, result)."""
    cands = np.ascontiguousarray(cands, dtype=np.uint8)
    o = fam.o
    K = len(cands)
    prior = hip.set_candidates(fam.fl["family"], cands)
    layout = hip.candidates_layout(fam.fl["family"])
    assert layout == npo.candidate_layout(o.msa, cands), layout
    if want_layout is not None:
        assert layout[2] == want_layout, layout
    assert not np.isnan(prior).any()
    _, first, inv = np.unique(cands, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    for k in (first if want_prior is None else ()):
        want = npo.constrained_log_prior(o, cands[k])
        if want == -math.inf:
            assert prior[k] == -math.inf, (k, prior[k])
        else:
            assert abs(prior[k] - want) < 1e-12 * max(1.0, abs(want)), (k, prior[k], want)
    if want_prior is not None:
        assert np.array_equal(prior, want_prior)
    assert np.array_equal(prior, prior[first][inv])   # duplicated candidates: the same bits
    res = hip.eval_candidates_batch(*fam.args(R, sl), K)
    lc_all = res["log_cand"]
    assert np.array_equal(lc_all, lc_all[:, first][:, inv], equal_nan=True)
    fin = np.isfinite(prior)
    start = 0 if sl.start is None else sl.start
    for i in range(lc_all.shape[0]):
        ll = fam.row(start + i, R)
        lc = lc_all[i]
        if not np.isfinite(ll):   # the reference's 2^(256 d) overflow: non-finite on both sides
            assert not np.isfinite(res["loglik"][i]) and np.isnan(lc).all(), i
            continue
        assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll), (i, res["loglik"][i], ll)
        assert not np.isnan(lc).any(), i
        assert np.all(lc[~fin] == -math.inf), i
        les = npo.log_emission_sums(o, cands[fin])
        got = lc[fin] - prior[fin] + res["loglik"][i]
        assert np.array_equal(np.isfinite(got), np.isfinite(les)), i
        ok = np.isfinite(les)
        err = np.abs(got[ok] - les[ok])
        assert err.size == 0 or err.max() < _tol(ll), (i, int(np.argmax(err)), err.max(), _tol(ll))
    return prior, res


def check_posterior_rows(hip, fam, R, rows, sl=slice(None)):
    """K5: the posterior of every row in `rows` (of the batch sl) against po.smoothing, one by one."""
    res = hip.eval_posterior_batch(*fam.args(R, sl), want=("loglik", "posterior"))
    start = 0 if sl.start is None else sl.start
    checked = 0
    for i in rows:
        ll = fam.row(start + i, R)
        if not np.isfinite(ll):
            assert not np.isfinite(res["loglik"][i]) and np.isnan(res["posterior"][i]).all(), i
            continue
        assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll), (i, res["loglik"][i], ll)
        err = np.max(np.abs(res["posterior"][i] - po.to_compact(fam.o, po.smoothing(fam.o))))
        assert err < 1e-10, (i, err)
        checked += 1
    return checked


# ---- 1. the long family: K2 with plain indices (kByteOff = false), K5 and K6 on it, RunPipeline ----

@pytest.mark.parametrize("extended", [False, True], ids=["default", "extended"])
def test_long_family_forward_matches_oracle(hip, long_fam, extended):
    desc, ll, res, ref = tp.run_family(hip, long_fam.o, long_fam.rows, 4, extended=extended)
    n_pat, form = tp.LAST_RUN["n_patterns"], tp.LAST_RUN["form"]
    assert n_pat >= BYTE_OFF_LIMIT + 2, (n_pat, form)
    assert all(np.isfinite(r["loglik"]) for r in ref)
    msg = "n_patterns %d, prune form %s" % (n_pat, form)
    if not extended:
        try:
            tp.compare(long_fam.o, desc, ll, res, ref)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (msg, e))
        return
    # extended-range mode scales its forward arrays by its own 2^-256 counts (test_gpu_parity's convention)
    for i, r in enumerate(ref):
        assert abs(ll[i] - r["loglik"]) <= 1e-10 * abs(r["loglik"]), (msg, i, ll[i], r["loglik"])
        np.testing.assert_allclose(res["xmsa_emission"][i], r["xmsa_emission"], rtol=1e-10, err_msg=msg)
        ex = tp.expand_forward(long_fam.o, desc, res["forward"][i], res["scaler_counts"][i])
        got = np.log(ex["jgerm_forward"].sum()) - ex["jgerm_scaler_count"] * np.log(2.0 ** 256)
        assert abs(got - r["loglik"]) <= 1e-10 * abs(r["loglik"]), (msg, i)
        big = r["jgerm_forward"] > r["jgerm_forward"].max() * 1e-100
        d = (ex["jgerm_scaler_count"] - r["jgerm_scaler_count"]) * 256
        np.testing.assert_allclose(ex["jgerm_forward"][big], np.ldexp(r["jgerm_forward"][big], d), rtol=1e-9,
                                   err_msg=msg)


def test_long_family_posterior(hip, long_fam):
    """K5 on the long family: every row against smoothing, and the host's site / gene marginals of one row."""
    from tests.test_gpu_posterior import _check, _pair
    assert check_posterior_rows(hip, long_fam, 4, range(long_fam.n)) == long_fam.n
    r = long_fam.rows[0]
    h, o = _pair(long_fam.yaml, long_fam.pdir, r["tree"], r["er"], r["pi"], r["alpha"], 4, False)
    _check(h, o)


def _boundary_candidates(o, target, rng):
    """Candidate 0 = one prior draw s0, then a few more prior draws, then fillers -- s0 with one site set to another
    base -- until the variable sites hold exactly `target` distinct (pattern, base) pairs.  A filler on a fresh pattern
    adds two pairs (s0's base and its own), one on an already variable site's pattern adds one."""
    d = _distinct_draws(o, 9, int(rng.integers(1 << 30)))
    s0 = d[0]
    cands = [c for c in d]
    msa = o.msa
    pats = {}
    pat = np.array([pats.setdefault(msa[:, i].tobytes(), len(pats)) for i in range(msa.shape[1])])
    var = np.nonzero((d != d[:1]).any(axis=0))[0]
    have = {(int(pat[i]), int(b)) for i in var for b in np.unique(d[:, i])}
    var_pats = {int(pat[i]) for i in var}
    assert len(have) < target
    # one site per pattern no variable site has, from the far end of the alignment (the last LDS slots)
    fresh = {}
    for i in range(msa.shape[1] - 1, -1, -1):
        if int(pat[i]) not in var_pats:
            fresh.setdefault(int(pat[i]), i)
    fresh_sites = list(fresh.values())
    pat_site = {int(pat[i]): int(i) for i in var}
    while len(have) < target:
        if target - len(have) >= 2 and fresh_sites:
            i = fresh_sites.pop(0)
            b = (int(s0[i]) + 1) % 4
            have |= {(int(pat[i]), int(s0[i])), (int(pat[i]), b)}
            pat_site[int(pat[i])] = i
        else:
            p, i, b = next((p, i, b) for p, i in pat_site.items() for b in range(5) if (p, b) not in have)
            have.add((p, b))
        c = s0.copy()
        c[i] = b
        cands.append(c)
    return np.array(cands, dtype=np.uint8)


@pytest.mark.parametrize("n_vlem", [1024, 1025, 8192, 8193])
def test_long_family_score_kernel_paths(hip, long_fam, n_vlem):
    """n_vlem 1 024 (score_kernel<8>, 64 KB), 1 025 (score_kernel<1>), 8 192 (<1>, 64 KB) and 8 193 (<1> past 64 KB of
    dynamic LDS), asserted on the device's own layout; all 4 rows, default and extended-range mode."""
    cands = _boundary_candidates(long_fam.o, n_vlem, np.random.default_rng(n_vlem))
    prior, _ = check_candidates(hip, long_fam, cands, want_layout=n_vlem)
    assert np.isfinite(prior[:9]).all()
    long_fam.set_extended_range(hip, True)
    try:
        check_candidates(hip, long_fam, cands, want_layout=n_vlem, want_prior=prior)
    finally:
        long_fam.set_extended_range(hip, False)


def test_long_family_run_pipeline(hip, long_fam, tmp_path):
    """RunPipeline on the long family: log-likelihood and NaiveSequence (K4) row by row against the oracle."""
    h = host.PhyloHMM(long_fam.yaml, 0, long_fam.pdir, 3)
    res = str(tmp_path / "lh.tsv")
    h.run_pipeline(long_fam.tsv, res, 4)
    lines = [ln.rstrip("\n").split("\t") for ln in open(res)]
    col = {name: i for i, name in enumerate(lines[0])}
    body = lines[1:]
    o = orc.PhyloHMM(long_fam.yaml, 0, long_fam.pdir, 3)
    assert len(body) == len(long_fam.rows)
    for r, got in zip(long_fam.rows, body):
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        ll = o.log_likelihood()
        assert abs(float(got[col["LHLogLikelihood"]]) - ll) <= 5e-6 * abs(ll)
        assert got[col["NaiveSequence"]] == o.sample_naive_sequence()
        assert got[col["VGene"]] == o.sample["vgerm_state_str_samp"]


# ---- 2. K6 at its launch edges (Spec.small) ----

@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 513])
def test_candidate_counts(hip, small_fam, K):
    """K = 1 and 2 identical candidates (V = 0: no gather, zero dynamic LDS), one block exactly (256), one candidate
    short and over, and a third partial block; 9 rows."""
    d = _distinct_draws(small_fam.o, K, K)
    cands = d[[0, 0]] if K == 2 else d
    _, res = check_candidates(hip, small_fam, cands, sl=slice(0, 9))
    if K <= 2:
        assert hip.candidates_layout(small_fam.fl["family"])[::2] == (0, 0)
    if K == 2:
        assert np.array_equal(res["log_cand"][:, 0], res["log_cand"][:, 1])


@pytest.mark.parametrize("n", [1, 7, 9, 257])
def test_row_counts(hip, small_fam, n):
    """K = 257 over 1 row, a partial 8-row group (7, 9) and two 256-row slabs (257); at 257 the weighted sums and weight
    statistics against numpy over the oracle-checked log_cand."""
    d = _distinct_draws(small_fam.o, 257, 7)
    cands = np.concatenate([d[:256], [_impossible(small_fam.o, d[256])]])
    _, res = check_candidates(hip, small_fam, cands, sl=slice(0, n))
    assert res["log_cand"].shape == (n, 257)
    if n == 257:
        from tools import synth_family as sf
        rb = np.array([r["likelihood"] for r in sf.read_trees_tsv(small_fam.tsv)][:n])
        again = hip.eval_candidates_batch(*small_fam.args(4, slice(0, n)), 257, log_offset=rb)
        assert np.array_equal(again["log_cand"], res["log_cand"])
        lw = again["loglik"] - rb
        m = lw.max()
        w = np.exp(lw - m)
        st = again["weight_stats"]
        assert st[0] == m and abs(st[1] - w.sum()) < 1e-12 * w.sum()
        assert abs(st[2] - (w * w).sum()) < 1e-12 * (w * w).sum()
        ref = w @ np.exp(res["log_cand"])
        assert np.allclose(again["weighted_sum"], ref, rtol=1e-12, atol=1e-300)
        assert again["weighted_sum"][-1] == 0.0


def test_two_prior_groups(hip, small_fam):
    """K = 4 097: K6a's second group of candidates starts at 4 096.  Candidates 4 095 and 4 096 are distinct draws;
    the draws repeat, and repeated candidates give the same bits."""
    o = small_fam.o
    d = npo.prior_draws(o, 4097, np.random.default_rng(4097))
    if np.array_equal(d[4095], d[4096]):
        j = next(j for j in range(4095) if not np.array_equal(d[j], d[4096]))
        d[[4095, j]] = d[[j, 4095]]
    assert not np.array_equal(d[4095], d[4096])
    assert len(np.unique(d, axis=0)) < 4097
    prior, _ = check_candidates(hip, small_fam, d, sl=slice(0, 3))
    assert np.isfinite(prior).all()


def test_too_many_candidates_refused(hip, small_fam):
    """K = 65 537 is refused before the sequences are read (a small array suffices)."""
    seqs = np.zeros((2, small_fam.o.msa.shape[1]), dtype=np.uint8)
    rc = hip.lib.lh_family_set_candidates(C.c_void_p(small_fam.fl["family"]), 65537,
                                          seqs.ctypes.data_as(C.POINTER(C.c_uint8)), None)
    assert rc != 0 and "K must be 1 .. 65536" in hip.error()


# ---- 3. K5 past the first workgroup, K5 / K6 on the unequal-chunk junction shapes, a seeded sweep ----

@pytest.mark.parametrize("kw", [{}, UNEQUAL[1]], ids=["small", "d65_j30"])
def test_posterior_rows_past_the_first_workgroup(hip, tmp_path, kw):
    """n = 37 = 16 + 16 + 5 rows: every row of the three K5 workgroups against smoothing, one by one."""
    from tools import synth_family as sf
    fam = Fam(str(tmp_path / "fam"), sf.Spec.small(**dict(dict(n_samples=37), **kw)))
    assert fam.n == 37
    assert check_posterior_rows(hip, fam, 4, range(37)) == 37


@pytest.mark.parametrize("kw", UNEQUAL, ids=UNEQUAL_IDS)
def test_unequal_chunk_shapes(hip, tmp_path, kw):
    from tools import synth_family as sf
    fam = Fam(str(tmp_path / "fam"), sf.Spec.small(n_samples=3, **kw))
    assert check_posterior_rows(hip, fam, 3, range(3)) == 3
    d = _distinct_draws(fam.o, 32, 5, at_least=8)
    check_candidates(hip, fam, np.concatenate([d, [_impossible(fam.o, d[0])]]), R=3)


def _sweep_kw(seed):
    rng = np.random.default_rng(seed)
    pick = lambda *ranges: int(rng.choice(np.concatenate([np.arange(a, b + 1) for a, b in ranges])))
    locus = ["igh", "igk", "igl"][seed % 3]
    kw = dict(locus=locus, seed=seed, n_samples=3, n_v=pick((1, 8), (60, 70), (125, 135)), n_j=pick((1, 6), (62, 70)))
    if locus == "igh":
        kw["n_d"] = pick((1, 6), (62, 70))
    if seed % 2:
        kw.update(ragged=int(rng.integers(1, 6)), ambiguous=0.03)
    return kw, int(rng.choice([1, 3, 4]))


@pytest.mark.parametrize("seed", range(201, 209))
def test_chunk_edge_sweep(hip, tmp_path, seed):
    """Allele counts drawn across the 64-gene chunk edges: K2 against the oracle, K5 row by row, K6 on prior draws."""
    from tools import synth_family as sf
    kw, R = _sweep_kw(seed)
    fam = Fam(str(tmp_path / "fam"), sf.Spec.small(**kw))
    desc, ll, res, ref = tp.run_family(hip, fam.o, fam.rows, R)
    fin = [i for i, r in enumerate(ref) if np.isfinite(r["loglik"])]
    assert [bool(np.isfinite(x)) for x in ll] == [bool(np.isfinite(r["loglik"])) for r in ref], kw
    sub = {k: v[fin] for k, v in res.items()}
    tp.compare(fam.o, desc, ll[fin], sub, [ref[i] for i in fin])
    check_posterior_rows(hip, fam, R, range(3))
    d = _distinct_draws(fam.o, 24, seed, at_least=8)
    check_candidates(hip, fam, np.concatenate([d, [_impossible(fam.o, d[0])]]), R=R)
