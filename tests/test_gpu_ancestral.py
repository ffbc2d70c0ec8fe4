"""K11 (exact ancestral-state marginals along a seed's lineage: lh_asr_marginals_batch, lh_eval_ancestral_batch) on the
device against tests/ancestral_marginal_oracle.py, against K3's own draws and against K5's device output.

Bounds: tables against the oracle 1e-10 absolute (the project's bound for the K5 / K9 / K10 tables); site_base against
posterior.site_base of lh_eval_posterior_batch's posterior of the same rows 1e-12; sums to 1 within 1e-12."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import capi
from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests.ancestral_cases import BOUND, Case, EvalCase, naive_dist, toy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


# ---- lh_asr_marginals_batch: trees, rates and a distribution of the naive base in, tables out ----

def _synth(tmp_path, spec):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(spec, out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    return h, sf.read_trees_tsv(os.path.join(out, "trees.tsv"))


def test_toy_family(hip, data_dir):
    """T = 4, two inner nodes: one tip's parent is the root (a chain of one), another's chain has two nodes."""
    h, rows = toy(data_dir)
    c = Case(hip, h, rows, 4)
    pairs = [(i, t) for i in range(2) for t in range(1, c.T)]
    _, _, paths = c.check(pairs, naive_dist(np.random.default_rng(1), 2, c.L))
    assert {len(p) for p in paths} == {1, 2}
    c.fam.close()


@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_every_tip_as_the_seed(hip, tmp_path, locus):
    """Spec.small (8 leaves x 62 sites), three tree samples, every tip in turn as the seed in ONE batch: chains of different
    lengths (so -1 padding), a seed whose sibling is a tip (a cherry: K3's tables do not store cherries) and one whose
    sibling is an inner node."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(locus=locus, n_samples=3, seed=5 if locus == "igk" else 7))
    c = Case(hip, h, rows, 4)
    pairs = [(i, t) for i in range(3) for t in range(1, c.T)]
    _, _, paths = c.check(pairs, naive_dist(np.random.default_rng(2), 3, c.L))
    assert len({len(p) for p in paths}) > 1
    sibs = [c.sibling(*p) for p in pairs]
    assert any(s < c.T for s in sibs) and any(s >= c.T for s in sibs)
    c.fam.close()


@pytest.mark.parametrize("R", [1, 8])
def test_rate_counts_at_both_ends(hip, tmp_path, R):
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_samples=2, n_leaves=17, seed=8 if R == 1 else 9))
    c = Case(hip, h, rows, R)
    c.check([(i, t) for i in range(2) for t in (1, 6, 11, 17)], naive_dist(np.random.default_rng(3), 2, c.L))
    c.fam.close()


@pytest.mark.parametrize("preset", ["mixed_n", "mixed_n_deep"])
def test_n_inside_columns(hip, tmp_path, preset):
    """N inside columns and all-N columns; the balanced 64-leaf tree has a schedule stack of depth >= 5."""
    from tools import synth_family as sf
    spec = {"mixed_n": sf.Spec.small(n_leaves=20, n_samples=3, seed=42, ragged=6, ambiguous=0.02),
            "mixed_n_deep": sf.Spec.small(n_leaves=64, n_samples=2, seed=49, tree_shape="balanced", n_nni=0, ragged=6,
                                          ambiguous=0.01)}[preset]
    h, rows = _synth(tmp_path, spec)
    n_n = (h.msa == 4).sum(axis=0)
    assert ((n_n > 0) & (n_n < h.msa.shape[0])).sum() > 10 and (n_n == h.msa.shape[0]).any()
    c = Case(hip, h, rows, 4)
    if preset == "mixed_n_deep":
        assert c.depth >= 5
    tips = range(1, c.T, 5)
    c.check([(i, t) for i in range(len(rows)) for t in tips], naive_dist(np.random.default_rng(4), len(rows), c.L))
    c.fam.close()


def test_ladder_of_forty(hip, tmp_path):
    """A ladder-shaped 40-leaf tree with the deepest tip as the seed: the longest chain a test can afford."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_leaves=40, n_samples=1, seed=11))
    rng = np.random.default_rng(6)
    leaves = [lab for lab in h.xmsa_labels if lab != "naive"]
    bl = lambda: "%.6f" % max(rng.exponential(0.02), 1e-4)
    sub = "(%s:%s,%s:%s)" % (leaves[-2], bl(), leaves[-1], bl())
    for lab in reversed(leaves[1:-2]):
        sub = "(%s:%s,%s:%s)" % (lab, bl(), sub, bl())
    rows = [dict(rows[0], tree="(naive:%s,%s:%s,%s:%s);" % (bl(), leaves[0], bl(), sub, bl()))]
    c = Case(hip, h, rows, 4)
    deepest = max(range(1, c.T), key=lambda t: len(c.path(0, t)))
    _, _, paths = c.check([(0, deepest), (0, 1)], naive_dist(rng, 1, c.L))
    assert len(paths[0]) >= 30
    c.fam.close()


def test_at_the_alpha_floor(hip, tmp_path):
    """The alpha = 0.05, R = 8, 1e-6-branch family of test_asr_at_the_alpha_floor: categories whose likelihood of a column
    is (all but) zero contribute 0, not NaN, and a column that varies leaves nothing on the slowest category."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_leaves=14, n_samples=3, seed=9005, locus="igk", ambiguous=0.05,
                                             tree_shape="balanced"))
    rows = [dict(r, alpha=0.05) for r in rows]
    c = Case(hip, h, rows, 8)
    marg, rp, _ = c.check([(i, t) for i in range(3) for t in (1, 5, 14)], naive_dist(np.random.default_rng(5), 3, c.L))
    assert np.isfinite(marg).all() and np.isfinite(rp).all()
    varies = np.array([len(set(h.msa[:, j][h.msa[:, j] < 4])) > 1 for j in range(c.L)])
    assert varies.sum() >= 3 and rp[:, varies, 0].max() < BOUND
    c.fam.close()


def test_one_hot_equals_k3s_draws(hip, tmp_path):
    """The K4-against-K5 test of this pair: with a one-hot naive_prob the tables are the distributions K3 draws from.
    lh_asr_batch over 20 000 sample numbers of one tree of Spec.small; every cell within 5 sigma + 1/N."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_samples=1))
    c = Case(hip, h, rows, 4)
    N = 20000
    naive = np.random.default_rng(7).integers(0, 5, size=c.L).astype(np.uint8)
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a)[None], N, axis=0))
    anc, choice = c.fam.asr_batch(c.T, c.depth, rep(c.ops[0]), rep(c.trees[0][2]), rep(rows[0]["er"]), rep(rows[0]["pi"]),
                                  rep(c.rates[0]), rep(naive), 20261019, 0)
    freq = np.stack([(anc == s).mean(axis=0) for s in range(4)], axis=-1)          # [T-2][L][4]
    rate_freq = np.stack([(choice == k).mean(axis=0) for k in range(4)], axis=-1)  # [L][R]
    q = [np.eye(5)[naive]]
    pairs = [(0, t) for t in range(1, c.T)]
    marg, rp, paths = c.batch(pairs, q)
    band = lambda p: 5 * np.sqrt(np.clip(p * (1 - p), 0, None) / N) + 1.0 / N
    for i, path in enumerate(paths):
        for s, v in enumerate(path):
            assert (np.abs(freq[v - c.T] - marg[i, s]) <= band(marg[i, s])).all(), (i, s)
        assert (np.abs(rate_freq - rp[i]) <= band(rp[i])).all()
    c.fam.close()


def test_rows_do_not_depend_on_their_batch(hip, tmp_path):
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_samples=3, seed=21))
    c = Case(hip, h, rows, 4)
    q = naive_dist(np.random.default_rng(8), 3, c.L)
    pairs = [(i, t) for i in range(3) for t in (1, 4, 8)]
    full, full_rp, _ = c.batch(pairs, q)
    P = full.shape[1]
    for i, p in enumerate(pairs):
        alone, alone_rp, path = c.batch([p], q)
        second, second_rp, _ = c.batch([pairs[(i + 1) % len(pairs)], p], q)
        k = len(path[0])
        assert np.array_equal(alone[0, :k], full[i, :k]) and np.array_equal(alone_rp[0], full_rp[i])
        assert np.array_equal(second[1, :k], full[i, :k]) and np.array_equal(second_rp[1], full_rp[i])
        assert k <= P
    c.fam.close()


def test_refusals(hip, data_dir):
    h, rows = toy(data_dir)
    c = Case(hip, h, rows[:1], 4)
    q = naive_dist(np.random.default_rng(9), 1, c.L)
    args = lambda path, rates=None: (c.T, c.depth, c.ops[0][None], c.trees[0][2][None], [rows[0]["er"]], [rows[0]["pi"]],
                                     c.rates[:1] if rates is None else rates, q, path)
    root = c.trees[0][1]
    other = [v for v in (c.T, c.T + 1) if v != root][0]
    c.fam.asr_marginals_batch(*args([[other, root]]))
    with pytest.raises(RuntimeError, match="path length must be in 1 .. n_tips - 2"):
        c.fam.asr_marginals_batch(*args(np.zeros((1, 0), dtype=np.int32)))
    with pytest.raises(RuntimeError, match="path length must be in 1 .. n_tips - 2"):
        c.fam.asr_marginals_batch(*args([[other, root, -1]]))
    with pytest.raises(RuntimeError, match="num_rates out of range"):
        c.fam.asr_marginals_batch(*args([[root]], rates=np.ones((1, 65))))
    # paths that are not the chain of a tip: the wrong order, a last entry that is not the root, padding in front, no entry
    for bad in ([[root, other]], [[other, -1]], [[-1, root]], [[-1, -1]], [[other, other]]):
        with pytest.raises(RuntimeError, match="is not a chain"):
            c.fam.asr_marginals_batch(*args(bad))
    bad_ops = c.ops[0].copy()
    bad_ops[0, 1] = 99
    with pytest.raises(RuntimeError, match="malformed schedule op"):
        c.fam.asr_marginals_batch(c.T, c.depth, bad_ops[None], *args([[root]])[3:])
    # the evaluation form needs sampler tables
    with pytest.raises(RuntimeError, match="lh_family_set_sampler has not been called"):
        hip.eval_ancestral_batch(c.fam, c.T, c.depth, c.ops[0][None], c.trees[0][2][None], [rows[0]["er"]], [rows[0]["pi"]],
                                 [1.0], 4, [[root]])
    c.fam.close()


# ---- lh_eval_ancestral_batch: the evaluation, K5, K11a and K11b in one call ----

def _synth_eval(hip, tmp_path, R=4, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(**kw), out)
    rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    return EvalCase(hip, os.path.join(out, "cluster.yaml"), os.path.join(out, "hmm_params"), rows, R, tmp_path)


def _toy_eval(hip, data_dir, tmp_path):
    _, rows = toy(data_dir)
    return EvalCase(hip, os.path.join(data_dir, "phylo_hmm_input.yaml"), os.path.join(data_dir, "hmm_params"), rows, 4,
                    tmp_path)


def _check_eval(c, pairs):
    res, paths = c.run(pairs)
    rows = [p[0] for p in pairs]
    k5 = c.hip.eval_posterior_batch(c.family, *c.args(rows), want=("loglik", "posterior"))
    for i, (row, _) in enumerate(pairs):
        P = len(paths[i])
        marg, rp, sb, ll = c.oracle(row, paths[i])
        assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll)
        assert np.abs(res["site_base"][i] - sb).max() < BOUND
        # against K5's own device output of the same rows
        assert np.abs(res["site_base"][i] - lp.site_base(c.state_space, k5["posterior"][i])).max() < 1e-12
        assert np.abs(res["marg"][i, :P] - marg).max() < BOUND
        assert np.abs(res["rate_post"][i] - rp).max() < BOUND
        assert np.abs(res["marg"][i, :P].sum(axis=-1) - 1).max() < 1e-12
        assert np.abs(res["rate_post"][i].sum(axis=-1) - 1).max() < 1e-12
        assert np.abs(res["site_base"][i].sum(axis=-1) - 1).max() < 1e-12
        assert not res["marg"][i, P:].any()
    return res, paths


def test_eval_toy_family(hip, data_dir, tmp_path):
    c = _toy_eval(hip, data_dir, tmp_path)
    _, paths = _check_eval(c, [(i, t) for i in range(2) for t in range(1, c.T)])
    assert {len(p) for p in paths} == {1, 2}


@pytest.mark.parametrize("locus,kw", [("igh", {}), ("igk", {}), ("igh", dict(ragged=4, ambiguous=0.02))])
def test_eval_synthetic_families(hip, tmp_path, locus, kw):
    c = _synth_eval(hip, tmp_path, locus=locus, n_samples=3, **kw)
    _check_eval(c, [(i, t) for i in range(3) for t in (1, 3, 8)])


def test_eval_composition(hip, tmp_path):
    """lh_eval_ancestral_batch's marg equals lh_asr_marginals_batch fed the same call's site_base and the rates of the
    evaluation, bit for bit."""
    c = _synth_eval(hip, tmp_path, n_samples=3, seed=31)
    pairs = [(i, t) for i in range(3) for t in (2, 5, 7)]
    res, paths = c.run(pairs)
    rows = [p[0] for p in pairs]
    a = c.args(rows)
    fam = capi.Family.borrow(c.family, hip)
    _, ev = fam.eval_batch(*a, want=("rates",))
    marg, rp = fam.asr_marginals_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], res["site_base"],
                                       capi.pad_paths(paths))
    assert np.array_equal(marg, res["marg"]) and np.array_equal(rp, res["rate_post"])


@pytest.mark.parametrize("family", ["toy", "igk"])
def test_eval_extended_range_equals_default(hip, data_dir, tmp_path, family):
    c = _toy_eval(hip, data_dir, tmp_path) if family == "toy" else _synth_eval(hip, tmp_path, locus="igk", n_samples=2)
    pairs = [(i, t) for i in range(2) for t in (1, c.T - 1)]
    a, _ = c.run(pairs)
    c.hh.set_extended_range(True)
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    b, paths = c.run(pairs)
    for k in ("site_base", "marg", "rate_post"):
        assert np.isfinite(a[k]).all() and np.abs(a[k] - b[k]).max() < BOUND, k
    assert np.allclose(a["loglik"], b["loglik"], rtol=1e-12)


def test_eval_extended_range_overflow_row(hip, tmp_path):
    """configs[4] (500 leaves x 600 sites): on a tree sample whose default-mode log-likelihood overflows (the rows
    tests/test_gpu_posterior.py finds), the default mode gives NaN tables and the extended-range mode finite ones that
    equal the oracle's on that tree -- the oracle rescales every CLV by its largest entry, so it has no range to lose --
    fed the naive-base posterior of that mode's own forward arrays (K5's device output, pushed through
    posterior.site_base)."""
    from linearham_amd import host
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec(n_leaves=500, n_sites=600, n_samples=64), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = hh.flatten_tsv(tsv, 64)
    fam = fl["family"]
    tree_args = lambda sl: (fl["n_tips"], fl["max_depth"], fl["ops"][sl], fl["brlen"][sl], fl["er"][sl], fl["pi"][sl],
                            fl["alpha"][sl], 4)
    default = hip.eval_posterior_batch(fam, *tree_args(slice(0, 64)), want=("loglik",))
    bad = [i for i in range(64) if not np.isfinite(default["loglik"][i])]
    assert bad, "no overflow row in the first 64 samples"
    i = bad[0]
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    labels = list(o.xmsa_labels)
    T = len(labels)
    children, root, brlen = host.newick_arrays(rows[i]["tree"], labels)
    ops, depth = hip.schedule_tree(T, children, root)
    assert np.array_equal(ops, fl["ops"][i]) and np.array_equal(brlen, fl["brlen"][i])
    path = capi.seed_path(T, children, root, 1)
    sl = slice(i, i + 1)
    nan = hip.eval_ancestral_batch(fam, *tree_args(sl), [path], want=("loglik", "site_base", "marg"))
    assert np.isnan(nan["loglik"][0]) or np.isinf(nan["loglik"][0])
    assert np.isnan(nan["site_base"]).all() and np.isnan(nan["marg"]).all()
    hip.check(hip.lib.lh_family_set_extended_range(fam, 1))
    ext = hip.eval_ancestral_batch(fam, *tree_args(sl), [path], want=("loglik", "site_base", "marg", "rate_post"))
    k5 = hip.eval_posterior_batch(fam, *tree_args(sl), want=("posterior",))
    q = lp.site_base(hh.dump(1), k5["posterior"][0])
    assert np.isfinite(ext["loglik"][0]) and np.abs(ext["site_base"][0] - q).max() < 1e-12
    marg, rp = amo.marginals(children, root, brlen, T, o.msa, q, rows[i]["er"], np.asarray(rows[i]["pi"]),
                             orc.gamma_rates_mean(rows[i]["alpha"], 4), path)
    assert np.isfinite(ext["marg"]).all()
    assert np.abs(ext["marg"][0] - marg).max() < BOUND and np.abs(ext["rate_post"][0] - rp).max() < BOUND


def test_eval_rows_do_not_depend_on_their_batch(hip, tmp_path):
    c = _synth_eval(hip, tmp_path, n_samples=3, seed=23)
    pairs = [(i, t) for i in range(3) for t in (1, 6)]
    full, _ = c.run(pairs)
    for i, p in enumerate(pairs):
        alone, path = c.run([p])
        second, _ = c.run([pairs[(i + 1) % len(pairs)], p])
        k = len(path[0])
        for key in ("loglik", "site_base", "rate_post"):
            assert np.array_equal(alone[key][0], full[key][i]) and np.array_equal(second[key][1], full[key][i]), key
        assert np.array_equal(alone["marg"][0, :k], full["marg"][i, :k])
        assert np.array_equal(second["marg"][1, :k], full["marg"][i, :k])


def test_eval_weighted_sums(hip, tmp_path):
    """n = 256 + 1 rows (one past a slab of the reduction) with random log_offset: the weighted sums within n 2^-52 relative
    of a long-double host sum of the returned per-row tables, bit-stable over two calls, and two half batches combined by
    posterior.combine within 1e-14 of the whole."""
    c = _synth_eval(hip, tmp_path, n_samples=5, seed=27)
    n = 257
    rng = np.random.default_rng(12)
    pairs = [(i % 5, 1 + (i * 3) % (c.T - 1)) for i in range(n)]
    off = -1000.0 + 3.0 * rng.standard_normal(n)
    want = ("loglik", "marg", "rate_post", "weighted_sum", "weighted_rate", "weight_stats")
    res, paths = c.run(pairs, log_offset=off, want=want)
    again, _ = c.run(pairs, log_offset=off, want=want)
    for k in ("weighted_sum", "weighted_rate", "weight_stats"):
        assert np.array_equal(res[k], again[k]), k
    lw = res["loglik"] - off
    m = lw.max()
    w = np.exp(lw - m)
    st = res["weight_stats"]
    assert st[0] == m and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    wl = w.astype(np.longdouble)
    ends = np.stack([np.stack([res["marg"][i, 0], res["marg"][i, len(paths[i]) - 1]]) for i in range(n)])
    ref_sum = np.tensordot(wl, ends.astype(np.longdouble), axes=1)
    ref_rate = np.tensordot(wl, res["rate_post"].astype(np.longdouble), axes=1)
    tol = n * 2.0 ** -52
    assert (np.abs(res["weighted_sum"] - ref_sum) <= tol * np.abs(ref_sum)).all()
    assert (np.abs(res["weighted_rate"] - ref_rate) <= tol * np.abs(ref_rate)).all()
    h1 = 128
    a, _ = c.run(pairs[:h1], log_offset=off[:h1], want=want)
    b, _ = c.run(pairs[h1:], log_offset=off[h1:], want=want)
    for key in ("weighted_sum", "weighted_rate"):
        mean, mx, s1, s2 = lp.combine([(a[key], a["weight_stats"]), (b[key], b["weight_stats"])])
        assert np.allclose(mean, res[key] / st[1], rtol=1e-14, atol=1e-300), key
    assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]


def _worker(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ancestral_worker.py"), mode], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_across_the_launch_group_cut():
    """One call of each entry point that crosses its launch-group cut (LH_CHUNK=256, read once per process: a child
    process, as tests/batch_boundaries_worker.py): rows on both sides of the cut carry the bits they have alone."""
    res = _worker("chunk", {"LH_CHUNK": "256"})
    assert res["n"] == 259 and res["groups_eval"] == 2 and res["groups_marginals"] == 2
    assert res["rows_checked"] == [0, 255, 256, 258]
    assert res["mismatches"] == []


def test_device_entry_points_on_a_torch_stream():
    """The _device forms on a stream of torch's (its own process: torch brings its own HIP runtime, which has to come up
    first -- see test_asr_rejected_device_schedule_gets_the_sentinel): equal to the host-pointer forms; a rejected
    device-resident schedule, a path that is not a chain and a path whose last entry is not the root each give that
    sample NaN and raise the handle's error word once, the other samples keep their bits."""
    res = _worker("device")
    assert res["clean_status"] == "" and res["clean_equals_host"]
    for k in ("schedule", "not_a_chain", "not_the_root"):
        assert res[k]["victim_all_nan"] and res[k]["others_unchanged"], k
        assert res[k]["second_status"] == "", k
    assert "malformed schedule" in res["schedule"]["status"]
    assert "not a chain" in res["not_a_chain"]["status"] and "not a chain" in res["not_the_root"]["status"]
    assert res["eval_victim_all_nan"] and res["eval_weights_leave_the_victim_out"]
    assert "not a chain" in res["eval_status"] and res["eval_second_status"] == ""


def test_output_bound_names_the_largest_n():
    """The refusal of the host-pointer evaluation form, through its hook (LH_ANC_OUT_MB=1, read once per process)."""
    res = _worker("bound", {"LH_ANC_OUT_MB": "1"})
    assert res["most"] > 8
    assert "batch too large" in res["message"] and "at most %d samples per call" % res["most"] in res["message"]
    assert res["largest_passes"]


def test_eval_host_form_refuses_a_bad_path(hip, tmp_path):
    c = _synth_eval(hip, tmp_path, n_samples=1, seed=37)
    good = c.path(0, 1)
    assert len(good) >= 2
    c.hip.eval_ancestral_batch(c.family, *c.args([0]), [good], want=("marg",))
    for bad in ([good[::-1]], [good[:-1]], [[-1] + good[1:]]):
        with pytest.raises(RuntimeError, match="is not a chain"):
            c.hip.eval_ancestral_batch(c.family, *c.args([0]), bad, want=("marg",))
    with pytest.raises(RuntimeError, match="path length must be in 1 .. n_tips - 2"):
        c.hip.eval_ancestral_batch(c.family, *c.args([0]), [good + [-1] * c.T], want=("marg",))


# ---- the host library: PhyloHMM::AncestralMarginals, the pipeline over a RevBayes table, the CLI ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _pipeline_family(hip, tmp_path):
    """A 9-row synthetic table, its rows' oracle tables for the seed, and what the pipeline should make of them."""
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=9, seed=41), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = EvalCase(hip, yaml_path, pdir, rows, 4, tmp_path)
    tip = 3
    per_row = []
    for i in range(9):
        path = c.path(i, tip)
        marg, rp, _, ll = c.oracle(i, path)
        per_row.append((ll - rows[i]["likelihood"], marg[0], marg[-1], rp, len(path)))
    return c, (yaml_path, pdir, tsv), list(c.o.xmsa_labels)[tip], per_row


def _weighted(per_row, first):
    used = per_row[first:]
    lw = np.array([r[0] for r in used])
    w = np.exp(lw - lw.max())
    mean = lambda k: sum(wi * r[k] for wi, r in zip(w, used)) / w.sum()
    return mean(1), mean(2), mean(3), w, w.sum() ** 2 / (w * w).sum()


def _check_files(res, per_row, first):
    parent, mrca, rates, w, ess = _weighted(per_row, first)
    assert np.abs(res["parent"] - parent).max() < BOUND and np.abs(res["mrca"] - mrca).max() < BOUND
    assert np.abs(res["rates"] - rates).max() < BOUND
    for name in ("parent", "mrca"):
        assert res["map_base"][name] == ["ACGT"[k] for k in np.argmax(res[name], axis=1)]
        assert np.abs(res[name].sum(axis=1) - 1).max() < 1e-12
    assert [r[0] for r in res["rows"]] == list(range(first, 9))
    assert np.allclose([r[1] for r in res["rows"]], w, rtol=1e-9)
    assert [r[2] for r in res["rows"]] == [r[4] for r in per_row[first:]]
    assert res["summary"]["rows_used"] == 9 - first and res["summary"]["rows_skipped_nonfinite"] == 0
    assert abs(res["summary"]["kish_ess"] - ess) < 1e-9 * ess


FILES = ("parent.tsv", "mrca.tsv", "rates.tsv", "rows.tsv", "summary.tsv")


def test_pipeline_and_cli(hip, tmp_path):
    """PhyloHMM::RunAncestralMarginalsPipeline on a 9-row table, through the library (burn-in 0.25) and through
    `linearham --ancestral-marginals-pipeline` (no burn-in; once more with three rows per batch: byte-identical files),
    against the oracle's per-row tables weighted by exp(LHLogLikelihood - Likelihood); then PhyloHMM::AncestralMarginals
    and `linearham --ancestral-marginals` on the first row's tree; and the one-device refusal."""
    from linearham_amd import host
    c, (yaml_path, pdir, tsv), seed_seq, per_row = _pipeline_family(hip, tmp_path)
    _check_files(c.hh.run_ancestral_marginals_pipeline(tsv, seed_seq, str(tmp_path / "lib"), 4, burnin_frac=0.25), per_row, 2)
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq]
    for name, env in (("cli", {}), ("cli3", {"LH_PIPELINE_BATCH": "3"})):
        r = subprocess.run([_exe(), "--ancestral-marginals-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / name)] +
                           common, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
    _check_files(host.read_ancestral_marginals(str(tmp_path / "cli")), per_row, 0)
    for f in FILES:
        assert open(str(tmp_path / "cli") + "." + f, "rb").read() == open(str(tmp_path / "cli3") + "." + f, "rb").read(), f
    # one tree
    row = c.rows[0]
    path = c.path(0, 3)
    want, want_rp, _, ll = c.oracle(0, path)
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one = c.hh.ancestral_marginals(seed_seq)
    assert one["nodes"] == path and abs(one["loglik"] - ll) < 1e-9 * abs(ll)
    assert np.abs(one["marg"] - want).max() < BOUND and np.abs(one["rate_post"] - want_rp).max() < BOUND
    newick = str(tmp_path / "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    args = [_exe(), "--ancestral-marginals", "--newick-path", newick, "--alpha", repr(row["alpha"])] + common
    args += sum([["--er", repr(x)] for x in row["er"]], []) + sum([["--pi", repr(x)] for x in row["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.strip().split("\n\n")
    assert len(blocks) == len(path) + 1
    for s, block in enumerate(blocks[:-1]):
        lines = block.split("\n")
        assert lines[0] == "slot\t%d\tnode\t%d" % (s, path[s]) and lines[1] == "site\tA\tC\tG\tT\tmap_base"
        got = np.array([[float(x) for x in ln.split("\t")[1:5]] for ln in lines[2:]])
        assert np.abs(got - want[s]).max() < BOUND
    got_rp = np.array([[float(x) for x in ln.split("\t")[1:]] for ln in blocks[-1].split("\n")[1:]])
    assert np.abs(got_rp - want_rp).max() < BOUND
    r = subprocess.run([_exe(), "--ancestral-marginals-pipeline", "--input-path", "x", "--output-path", "y", "--devices", "0,1"] +
                       common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr
    r = subprocess.run([_exe(), "--ancestral-marginals-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / "z")] +
                       common[:-1] + ["naive"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot be 'naive'" in r.stderr
