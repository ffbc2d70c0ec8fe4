"""K12 (exact substitution posteriors along the edges of a seed's lineage: lh_asr_edges_batch, lh_eval_edges_batch) on the
device against tests/edge_oracle.py, against K11's own device output and against itself.

Bounds: tables against the oracle 1e-10 absolute (BOUND, the project's bound for the K5 / K9 / K10 / K11 tables); the margin
identities against lh_asr_marginals_batch's device output and the input q, and the reductions recomputed from edge on the
host, 1e-12; what is said to have the same bits is compared with array_equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import capi
from tests.ancestral_cases import BOUND, naive_dist, toy
from tests.edges_cases import TABLES, EdgeCase, EdgeEvalCase

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN = ("naive_edge", "chain_counts", "edge_load", "rate_post")


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def _synth(tmp_path, spec):
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(spec, out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    return h, sf.read_trees_tsv(os.path.join(out, "trees.tsv"))


# ---- lh_asr_edges_batch against the oracle ----

def test_toy_family(hip, data_dir):
    """T = 4: a seed under the root (one slot: the seed edge and the naive edge only) and seeds with an inner edge."""
    h, rows = toy(data_dir)
    c = EdgeCase(hip, h, rows, 4)
    out = c.check_edges([(i, t) for i in range(2) for t in range(1, c.T)], naive_dist(np.random.default_rng(1), 2, c.L))
    assert {len(p) for _, p in out} == {1, 2}
    c.fam.close()


@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_every_tip_as_the_seed(hip, tmp_path, locus):
    """Spec.small (8 leaves x 62 sites), three tree samples, every tip in turn as the seed, the three samples in one batch:
    the seed as either child of a cherry and as the tip of a tip-accumulate op, the path continuing through the popped and
    through the accumulator child, chains of different lengths in one batch (-1 padding)."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(locus=locus, n_samples=3, seed=5 if locus == "igk" else 7))
    c = EdgeCase(hip, h, rows, 4)
    pairs = [(i, t) for t in range(1, c.T) for i in range(3)]
    out = c.check_edges(pairs, naive_dist(np.random.default_rng(2), 3, c.L))
    assert len({len(p) for _, p in out}) > 1
    kinds = set()
    for row, tip in pairs:
        ops = c.ops[row]
        for op in ops:
            if (op[0] & 15) == 0 and tip in (op[1], op[2]):
                kinds.add("cherry_y" if op[1] == tip else "cherry_z")
            elif (op[0] & 15) == 1 and op[1] == tip:
                kinds.add("tip_acc")
    assert kinds == {"cherry_y", "cherry_z", "tip_acc"}
    assert any((c.ops[r][:, 0] & 15 == 2).any() for r in range(3))       # pop ops: a path through the popped child exists
    c.fam.close()


@pytest.mark.parametrize("R", [1, 8])
def test_rate_counts_at_both_ends(hip, tmp_path, R):
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_samples=2, n_leaves=17, seed=8 if R == 1 else 9))
    c = EdgeCase(hip, h, rows, R)
    c.check_edges([(i, t) for t in (1, 6, 11, 17) for i in range(2)], naive_dist(np.random.default_rng(3), 2, c.L))
    c.fam.close()


@pytest.mark.parametrize("preset", ["mixed_n", "mixed_n_deep"])
def test_n_inside_columns(hip, tmp_path, preset):
    """N inside columns and all-N columns, seed tips with N among them; the balanced 64-leaf tree (schedule stack >= 5)."""
    from tools import synth_family as sf
    spec = {"mixed_n": sf.Spec.small(n_leaves=20, n_samples=3, seed=42, ragged=6, ambiguous=0.02),
            "mixed_n_deep": sf.Spec.small(n_leaves=64, n_samples=2, seed=49, tree_shape="balanced", n_nni=0, ragged=6,
                                          ambiguous=0.01)}[preset]
    h, rows = _synth(tmp_path, spec)
    c = EdgeCase(hip, h, rows, 4)
    if preset == "mixed_n_deep":
        assert c.depth >= 5
    n_n = (h.msa == 4).sum(axis=0)
    partly = (n_n > 0) & (n_n < h.msa.shape[0])
    # seed tips that are N in a column where other tips are not, first
    with_n = [t for t in range(1, c.T) if ((h.msa[t - 1] == 4) & partly).any()]
    assert with_n
    tips = sorted(set(with_n[:2] + list(range(1, c.T, 7))))
    c.check_edges([(i, t) for t in tips for i in range(len(rows))], naive_dist(np.random.default_rng(4), len(rows), c.L))
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
    c = EdgeCase(hip, h, rows, 4)
    deepest = max(range(1, c.T), key=lambda t: len(c.path(0, t)))
    out = c.check_edges([(0, deepest), (0, 1)], naive_dist(rng, 1, c.L))
    assert len(out[0][1]) >= 30
    c.fam.close()


def test_at_the_alpha_floor(hip, tmp_path):
    """alpha = 0.05, R = 8: categories whose likelihood of a column is (all but) zero contribute 0, not NaN."""
    from tools import synth_family as sf
    h, rows = _synth(tmp_path, sf.Spec.small(n_leaves=14, n_samples=3, seed=9005, locus="igk", ambiguous=0.05,
                                             tree_shape="balanced"))
    rows = [dict(r, alpha=0.05) for r in rows]
    c = EdgeCase(hip, h, rows, 8)
    out = c.check_edges([(i, t) for t in (1, 5, 14) for i in range(3)], naive_dist(np.random.default_rng(5), 3, c.L))
    assert all(np.isfinite(got[k]).all() for got, _ in out for k in TABLES)
    c.fam.close()


# ---- identities on the device's own output ----

@pytest.fixture(scope="module")
def small(hip, tmp_path_factory):
    from tools import synth_family as sf
    h, rows = _synth(tmp_path_factory.mktemp("edges"), sf.Spec.small(n_samples=3, seed=21, ragged=4, ambiguous=0.02))
    c = EdgeCase(hip, h, rows, 4)
    yield c, naive_dist(np.random.default_rng(8), 3, c.L)
    c.fam.close()


def test_margins_against_k11(small):
    """sum_c edge[s] = marg[s], sum_a edge[s] = marg[s-1], sum_i naive_edge = q, sum_b naive_edge = marg[len-1], with marg
    from lh_asr_marginals_batch on the same rows."""
    c, q = small
    for tip in (1, 4, 8):
        rows = [0, 1, 2]
        res, paths = c.call(rows, tip, q)
        marg, rp, _ = c.batch([(r, tip) for r in rows], q)
        for i in rows:
            n = len(paths[i])
            edge, ne = res["edge"][i, :n], res["naive_edge"][i]
            assert np.abs(edge.sum(axis=-1) - marg[i, :n]).max() < 1e-12
            if n > 1:
                assert np.abs(edge[1:].sum(axis=-2) - marg[i, :n - 1]).max() < 1e-12
            assert np.abs(ne.sum(axis=-1) - q[i]).max() < 1e-12
            assert np.abs(ne.sum(axis=-2) - marg[i, n - 1]).max() < 1e-12
            assert np.array_equal(res["rate_post"][i], rp[i])


def test_lean_form_has_the_same_bits(small):
    c, q = small
    for tip in (2, 7):
        full, _ = c.call([0, 1, 2], tip, q)
        lean, _ = c.call([0, 1, 2], tip, q, want=LEAN)
        assert "edge" not in lean
        for k in LEAN:
            assert np.array_equal(full[k], lean[k]), k
        only, _ = c.call([1], tip, q, want=("chain_counts",))
        assert np.array_equal(only["chain_counts"][0], full["chain_counts"][1])


def test_reductions_from_edge_on_the_host(small):
    from tests import edge_oracle as eo
    c, q = small
    res, paths = c.call([0, 1, 2], 5, q)
    for i in range(3):
        n = len(paths[i])
        cc, load = eo.reductions(res["edge"][i, :n], res["naive_edge"][i])
        assert np.abs(res["chain_counts"][i] - cc).max() < 1e-12
        assert np.abs(np.concatenate([res["edge_load"][i, :n], res["edge_load"][i, -1:]]) - load).max() < 1e-12
        assert not res["edge"][i, n:].any() and not res["edge_load"][i, n:-1].any()
    assert len({len(p) for p in paths}) > 1 or res["edge"].shape[1] == len(paths[0])


def test_rows_do_not_depend_on_their_batch(small):
    c, q = small
    for tip in (1, 6):
        full, paths = c.call([0, 1, 2], tip, q)
        for i in range(3):
            alone, _ = c.call([i], tip, q)
            second, _ = c.call([(i + 1) % 3, i], tip, q)
            n = len(paths[i])
            for k in TABLES:
                a, s, f = alone[k][0], second[k][1], full[k][i]
                if k == "edge":
                    a, s, f = a[:n], s[:n], f[:n]
                elif k == "edge_load":
                    pick = lambda x: np.concatenate([x[:n], x[-1:]])
                    a, s, f = pick(a), pick(s), pick(f)
                assert np.array_equal(a, f) and np.array_equal(s, f), (tip, i, k)


def test_refusals(hip, data_dir):
    h, rows = toy(data_dir)
    c = EdgeCase(hip, h, rows[:1], 4)
    q = naive_dist(np.random.default_rng(9), 1, c.L)
    children, root, _ = c.trees[0]
    other = [v for v in (c.T, c.T + 1) if v != root][0]
    under_root = [int(t) for t in children[2 * (root - c.T):2 * (root - c.T) + 2] if t < c.T][0]
    under_other = [int(t) for t in children[2 * (other - c.T):2 * (other - c.T) + 2] if t < c.T][0]
    call = lambda path, tip, ops=None: c.fam.asr_edges_batch(
        c.T, c.depth, (c.ops[0] if ops is None else ops)[None], c.trees[0][2][None], [rows[0]["er"]], [rows[0]["pi"]], c.rates[:1],
        q, path, tip)
    call([[other, root]], under_other)
    call([[root]], under_root)
    for tip in (0, c.T, -1):
        with pytest.raises(RuntimeError, match="seed_tip must be a tip other than naive"):
            call([[other, root]], tip)
    with pytest.raises(RuntimeError, match="seed_tip %d is not a child of path\\[0\\] of sample 0" % under_root):
        call([[other, root]], under_root)
    with pytest.raises(RuntimeError, match="is not a child of path\\[0\\]"):
        call([[root]], under_other)
    with pytest.raises(RuntimeError, match="is not a chain"):
        call([[root, other]], under_other)
    with pytest.raises(RuntimeError, match="path length must be in 1 .. n_tips - 2"):
        call([[other, root, -1]], under_other)
    bad_ops = c.ops[0].copy()
    bad_ops[0, 1] = 99
    with pytest.raises(RuntimeError, match="malformed schedule op"):
        call([[root]], under_root, ops=bad_ops)
    # the evaluation form needs sampler tables
    with pytest.raises(RuntimeError, match="lh_family_set_sampler has not been called"):
        hip.eval_edges_batch(c.fam, c.T, c.depth, c.ops[0][None], c.trees[0][2][None], [rows[0]["er"]], [rows[0]["pi"]], [1.0], 4,
                             [[root]], under_root)
    c.fam.close()


# ---- lh_eval_edges_batch: the evaluation, K5, K11a and K12 in one call ----

def _synth_eval(hip, tmp_path, R=4, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(**kw), out)
    rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    return EdgeEvalCase(hip, os.path.join(out, "cluster.yaml"), os.path.join(out, "hmm_params"), rows, R, tmp_path)


def _toy_eval(hip, data_dir, tmp_path):
    _, rows = toy(data_dir)
    return EdgeEvalCase(hip, os.path.join(data_dir, "phylo_hmm_input.yaml"), os.path.join(data_dir, "hmm_params"), rows, 4,
                        tmp_path)


def test_eval_composition_and_oracle(hip, tmp_path):
    """lh_eval_edges_batch's tables equal lh_asr_edges_batch fed the same call's site_base and the rates of the evaluation,
    bit for bit; seed_edge is slot 0 of edge; and the tables equal the oracle's fed the oracle's own naive-base posterior."""
    c = _synth_eval(hip, tmp_path, n_samples=3, seed=31)
    fam = capi.Family.borrow(c.family, hip)
    rows = [0, 1, 2]
    a = c.args(rows)
    _, ev = fam.eval_batch(*a, want=("rates",))
    for tip in (2, 7):
        res, paths = c.run_edges(rows, tip, want=("loglik", "site_base", "seed_edge") + TABLES)
        got = fam.asr_edges_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], res["site_base"], capi.pad_paths(paths), tip)
        for k in TABLES:
            assert np.array_equal(got[k], res[k]), k
        assert np.array_equal(res["seed_edge"], res["edge"][:, 0])
        lean, _ = c.run_edges(rows, tip, want=("seed_edge",) + LEAN)
        for k in ("seed_edge",) + LEAN:
            assert np.array_equal(lean[k], res[k]), k
        for i in rows:
            _, _, sb, ll = c.oracle(i, paths[i])
            want = c.edge_oracle(i, paths[i], tip, sb)
            n = len(paths[i])
            assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll)
            assert np.abs(res["edge"][i, :n] - want["edge"]).max() < BOUND
            assert np.abs(res["naive_edge"][i] - want["naive_edge"]).max() < BOUND
            assert np.abs(res["chain_counts"][i] - want["chain_counts"]).max() < BOUND


@pytest.mark.parametrize("family", ["toy", "igk"])
def test_eval_extended_range_equals_default(hip, data_dir, tmp_path, family):
    c = _toy_eval(hip, data_dir, tmp_path) if family == "toy" else _synth_eval(hip, tmp_path, locus="igk", n_samples=2)
    tip = c.T - 1
    a, _ = c.run_edges([0, 1], tip)
    c.hh.set_extended_range(True)
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    b, _ = c.run_edges([0, 1], tip)
    for k in ("site_base",) + TABLES:
        assert np.isfinite(a[k]).all() and np.abs(a[k] - b[k]).max() < BOUND, k
    assert np.allclose(a["loglik"], b["loglik"], rtol=1e-12)


def test_eval_weighted_sums(hip, tmp_path):
    """n = 256 + 1 rows (one past a slab of the reduction) with random log_offset: the weighted sums within n 2^-52 relative
    of a long-double host sum of the returned per-row tables, bit-stable over two calls, and two half batches combined by
    posterior.combine within 1e-14 of the whole."""
    from linearham_amd import posterior as lp
    c = _synth_eval(hip, tmp_path, n_samples=5, seed=27)
    n, tip = 257, 3
    rng = np.random.default_rng(12)
    rows = [i % 5 for i in range(n)]
    off = -1000.0 + 3.0 * rng.standard_normal(n)
    sums = {"weighted_counts": "chain_counts", "weighted_seed_edge": "seed_edge", "weighted_naive_edge": "naive_edge"}
    want = ("loglik", "weight_stats") + tuple(sums) + tuple(sums.values())
    res, _ = c.run_edges(rows, tip, log_offset=off, want=want)
    again, _ = c.run_edges(rows, tip, log_offset=off, want=want)
    for k in tuple(sums) + ("weight_stats",):
        assert np.array_equal(res[k], again[k]), k
    lw = res["loglik"] - off
    m = lw.max()
    w = np.exp(lw - m)
    st = res["weight_stats"]
    assert st[0] == m and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    wl = w.astype(np.longdouble)
    tol = n * 2.0 ** -52
    for k, rows_key in sums.items():
        ref = np.tensordot(wl, res[rows_key].astype(np.longdouble), axes=1)
        assert (np.abs(res[k] - ref) <= tol * np.abs(ref)).all(), k
    h1 = 128
    a, _ = c.run_edges(rows[:h1], tip, log_offset=off[:h1], want=want)
    b, _ = c.run_edges(rows[h1:], tip, log_offset=off[h1:], want=want)
    for key in sums:
        mean, mx, s1, s2 = lp.combine([(a[key], a["weight_stats"]), (b[key], b["weight_stats"])])
        assert np.allclose(mean, res[key] / st[1], rtol=1e-14, atol=1e-300), key
    assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]


def test_eval_host_form_refuses_a_bad_seed(hip, tmp_path):
    c = _synth_eval(hip, tmp_path, n_samples=1, seed=37)
    good = c.path(0, 1)
    c.hip.eval_edges_batch(c.family, *c.args([0]), [good], 1, want=("chain_counts",))
    stranger = [t for t in range(1, c.T) if c.path(0, t)[0] != good[0]][0]
    with pytest.raises(RuntimeError, match="is not a child of path\\[0\\]"):
        c.hip.eval_edges_batch(c.family, *c.args([0]), [good], stranger, want=("chain_counts",))
    with pytest.raises(RuntimeError, match="seed_tip must be a tip other than naive"):
        c.hip.eval_edges_batch(c.family, *c.args([0]), [good], c.T, want=("chain_counts",))
    if len(good) >= 2:
        with pytest.raises(RuntimeError, match="is not a chain"):
            c.hip.eval_edges_batch(c.family, *c.args([0]), [good[::-1]], 1, want=("chain_counts",))


# ---- worker processes: hooks read once per process, torch's stream ----

def _worker(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edges_worker.py"), mode], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_across_the_launch_group_cut():
    """One call of each entry point that crosses its launch-group cut (LH_CHUNK=256, read once per process): rows on both
    sides of the cut carry the bits they have alone."""
    res = _worker("chunk", {"LH_CHUNK": "256"})
    assert res["n"] == 259 and res["groups_eval"] == 2 and res["groups_edges"] == 2
    assert res["rows_checked"] == [0, 255, 256, 258]
    assert res["mismatches"] == []


def test_device_entry_points_on_a_torch_stream():
    """The _device forms on a stream of torch's: equal to the host-pointer forms; a rejected device-resident schedule, a
    path that is not a chain and a seed_tip that is not a child of path[0] each give that sample NaN and raise the handle's
    error word once, the other samples keep their bits; the evaluation form leaves the victim out of its weighted sums."""
    res = _worker("device")
    assert res["clean_status"] == "" and res["clean_equals_host"]
    for k in ("schedule", "not_a_chain", "not_a_child"):
        assert res[k]["victim_all_nan"] and res[k]["others_unchanged"], k
        assert res[k]["second_status"] == "", k
    assert "malformed schedule" in res["schedule"]["status"]
    assert "not a chain" in res["not_a_chain"]["status"] and "not a chain" in res["not_a_child"]["status"]
    assert res["eval_victim_all_nan"] and res["eval_weights_leave_the_victim_out"]
    assert "not a chain" in res["eval_status"] and res["eval_second_status"] == ""


def test_output_bound_names_the_largest_n():
    """The refusal of the host-pointer forms, through its hook (LH_EDGE_OUT_MB=1, read once per process)."""
    res = _worker("bound", {"LH_EDGE_OUT_MB": "1"})
    assert res["most"] > 2
    assert "batch too large" in res["message"] and "at most %d samples per call" % res["most"] in res["message"]
    assert res["largest_passes"]


# ---- the host library: PhyloHMM::LineageSubstitutions, the pipeline over a RevBayes table, the CLI ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


FILES = ("substitutions.tsv", "seed_edge.tsv", "naive_edge.tsv", "rows.tsv", "summary.tsv")


def _check_files(res, per_row, first):
    used = per_row[first:]
    lw = np.array([r["lw"] for r in used])
    w = np.exp(lw - lw.max())
    mean = lambda k: sum(wi * r[k] for wi, r in zip(w, used)) / w.sum()
    assert np.abs(res["counts"] - mean("chain_counts")).max() < BOUND
    assert np.abs(res["seed_edge"] - mean("seed_edge")).max() < BOUND
    assert np.abs(res["naive_edge"] - mean("naive_edge")).max() < BOUND
    assert np.abs(res["substitutions"] - (res["counts"] * (1 - np.eye(4))).sum(axis=(1, 2))).max() < 1e-12
    assert [r[0] for r in res["rows"]] == list(range(first, 9))
    assert np.allclose([r[1] for r in res["rows"]], w, rtol=1e-9)
    assert [r[2] for r in res["rows"]] == [r["len"] for r in used]
    assert np.abs(np.array([r[3] for r in res["rows"]]) - np.array([r["edge_load"].sum() for r in used])).max() < BOUND
    assert res["summary"]["rows_used"] == 9 - first and res["summary"]["rows_skipped_nonfinite"] == 0
    ess = w.sum() ** 2 / (w * w).sum()
    assert abs(res["summary"]["kish_ess"] - ess) < 1e-9 * ess


def test_pipeline_and_cli(hip, tmp_path):
    """PhyloHMM::RunLineageSubstitutionsPipeline on a 9-row table, through the library (burn-in 0.25) and through
    `linearham --lineage-substitutions-pipeline` (no burn-in; once more with three rows per batch: byte-identical files),
    against the oracle's per-row tables weighted by exp(LHLogLikelihood - Likelihood); then PhyloHMM::LineageSubstitutions
    and `linearham --lineage-substitutions` on the first row's tree; and the one-device refusal."""
    from linearham_amd import host
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=9, seed=41), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = EdgeEvalCase(hip, yaml_path, pdir, rows, 4, tmp_path)
    tip = 3
    seed_seq = list(c.o.xmsa_labels)[tip]
    per_row = []
    for i in range(9):
        path = c.path(i, tip)
        _, _, sb, ll = c.oracle(i, path)
        want = c.edge_oracle(i, path, tip, sb)
        per_row.append(dict(want, lw=ll - rows[i]["likelihood"], seed_edge=want["edge"][0], len=len(path), loglik=ll))
    _check_files(c.hh.run_lineage_substitutions_pipeline(tsv, seed_seq, str(tmp_path / "lib"), 4, burnin_frac=0.25), per_row, 2)
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq]
    for name, env in (("cli", {}), ("cli3", {"LH_PIPELINE_BATCH": "3"})):
        r = subprocess.run([_exe(), "--lineage-substitutions-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / name)] +
                           common, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
    _check_files(host.read_lineage_substitutions(str(tmp_path / "cli")), per_row, 0)
    for f in FILES:
        assert open(str(tmp_path / "cli") + "." + f, "rb").read() == open(str(tmp_path / "cli3") + "." + f, "rb").read(), f
    # one tree
    row, want = c.rows[0], per_row[0]
    path = c.path(0, tip)
    P = len(path)
    children, root, brlen = c.trees[0]
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one = c.hh.lineage_substitutions(seed_seq)
    assert one["nodes"] == path and abs(one["loglik"] - want["loglik"]) < 1e-9 * abs(want["loglik"])
    assert np.abs(one["edge"] - want["edge"]).max() < BOUND and np.abs(one["naive_edge"] - want["naive_edge"]).max() < BOUND
    assert np.abs(one["chain_counts"] - want["chain_counts"]).max() < BOUND
    lower = [tip] + path[:-1] + [path[-1]]
    assert [(e[0], e[1]) for e in one["edges"]] == list(zip(path + [0], lower))
    assert [e[2] for e in one["edges"]] == [brlen[v] for v in lower[:-1]] + [brlen[0]]
    assert np.abs(np.array([e[3] for e in one["edges"]]) - want["edge_load"]).max() < BOUND
    newick = str(tmp_path / "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    args = [_exe(), "--lineage-substitutions", "--newick-path", newick, "--alpha", repr(row["alpha"])] + common
    args += sum([["--er", repr(x)] for x in row["er"]], []) + sum([["--pi", repr(x)] for x in row["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.strip().split("\n\n")
    assert len(blocks) == P + 3
    lines = blocks[0].split("\n")
    assert lines[0] == "edge\tupper\tlower\tbrlen\texpected_substitutions" and len(lines) == P + 2
    for e, ln in enumerate(lines[1:]):
        cells = ln.split("\t")
        assert [int(x) for x in cells[:3]] == [e, one["edges"][e][0], one["edges"][e][1]]
        assert float(cells[3]) == one["edges"][e][2] and float(cells[4]) == one["edges"][e][3]
    table = lambda block, skip: np.array([[float(x) for x in ln.split("\t")[1:]] for ln in block.split("\n")[skip:]])
    assert np.array_equal(table(blocks[1], 1)[:, :16].reshape(-1, 4, 4), one["chain_counts"])
    for s in range(P):
        assert blocks[2 + s].split("\n")[0] == "edge\t%d\tupper\t%d\tlower\t%d" % (s, path[s], lower[s])
        assert np.array_equal(table(blocks[2 + s], 2).reshape(-1, 4, 4), one["edge"][s])
    assert blocks[-1].split("\n")[0] == "edge\t%d\tupper\t0\tlower\t%d" % (P, path[-1])
    assert np.array_equal(table(blocks[-1], 2).reshape(-1, 5, 4), one["naive_edge"])
    r = subprocess.run([_exe(), "--lineage-substitutions-pipeline", "--input-path", "x", "--output-path", "y", "--devices", "0,1"] +
                       common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr
    r = subprocess.run([_exe(), "--lineage-substitutions-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / "z")] +
                       common[:-1] + ["naive"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot be 'naive'" in r.stderr
