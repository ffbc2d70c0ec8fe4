"""K13 (exact posterior probabilities of candidate ancestral sequences: lh_family_set_ancestral_candidates,
lh_eval_ancestral_candidates_batch) on the device against tests/ancestral_probs_oracle.py, against K11's own device output
and against itself.

Bounds: the tables `cond` against the oracle 1e-10 absolute (ancestral_cases.BOUND, the project's bound for the K5 / K9 /
K10 / K11 tables) and against five one-hot calls of lh_asr_marginals_batch on the device 1e-12; one-site candidates
against lh_eval_ancestral_batch's marg 1e-10; the 64 three-site candidates sum to 1 within 1e-10.  log_cand against the
oracle: LOG_CAND_BOUND, 100 times the largest deviation this module measured on an MI355X (2.49e-13, on Spec.small igk;
every test prints its own), to leave room for other seeds and compiler versions, and never looser than 1e-8: K11's tables
measured 5.9e-15 against 1e-10, and the sweep carries the project's 1e-12 relative bound on log-likelihoods of order 1e2.
What is said to have the same bits is compared with array_equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import capi
from linearham_amd import posterior as lp
from tests import ancestral_probs_oracle as apo
from tests.ancestral_cases import BOUND
from tests.ancestral_probs_cases import MRCA, PARENT, synth, toy_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_CAND_BOUND = 2.5e-11
NODES = (PARENT, MRCA)


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


# ---- cond: the conditional tables ----

def _one_hot_on_device(c, pairs, paths, node):
    """G from five calls of lh_asr_marginals_batch with one-hot naive distributions, on the rates of the evaluation."""
    rows = [p[0] for p in pairs]
    a = c.args(rows)
    fam = capi.Family.borrow(c.family, c.hip)
    _, ev = fam.eval_batch(*a, want=("rates",))
    G = np.zeros((len(pairs), c.L, 5, 4))
    for b in range(5):
        q = np.zeros((len(pairs), c.L, 5))
        q[:, :, b] = 1.0
        marg, _ = fam.asr_marginals_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], q, capi.pad_paths(paths),
                                          want=("marg",))
        for i, p in enumerate(paths):
            G[i, :, b] = marg[i, apo.slot_of(node, p)]
    return G


def _check_cond(c, pairs):
    """Both nodes against the oracle and against K11 on the device; rows whose path has one node give the same bits at
    both.  Returns the paths."""
    c.hip.set_ancestral_candidates(c.family, np.full((1, c.L), apo.OPEN))
    got = {}
    worst = 0.0
    for node in NODES:
        res, paths = c.probs(pairs, node, want=("cond",))
        got[node] = res["cond"]
        k11 = _one_hot_on_device(c, pairs, paths, node)
        assert np.abs(res["cond"] - k11).max() < 1e-12
        for i, (row, _) in enumerate(pairs):
            worst = max(worst, np.abs(res["cond"][i] - c.oracle_tables(row, paths[i], node)).max())
        assert np.abs(res["cond"].sum(axis=-1) - 1).max() < 1e-12
    print("cond: worst difference from the oracle %.3g" % worst)
    assert worst < BOUND
    for i, p in enumerate(paths):
        if len(p) == 1:
            assert np.array_equal(got[PARENT][i], got[MRCA][i])
    return paths


def test_cond_toy_family(hip, data_dir, tmp_path):
    """T = 4: a seed under the root (parent = MRCA: the same bits) and seeds with a chain of two."""
    c = toy_case(hip, data_dir, tmp_path)
    paths = _check_cond(c, [(i, t) for i in range(2) for t in range(1, c.T)])
    assert {len(p) for p in paths} == {1, 2}


@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_cond_every_tip_as_the_seed(hip, tmp_path, locus):
    """Spec.small (8 leaves x 62 sites), three tree samples, every tip in turn as the seed: chains of different lengths in
    one batch, through popped and accumulator children."""
    c = synth(hip, tmp_path, locus=locus, n_samples=3, seed=5 if locus == "igk" else 7)
    paths = _check_cond(c, [(i, t) for t in range(1, c.T) for i in range(3)])
    assert len({len(p) for p in paths}) > 1
    assert any((c.ops[r][:, 0] & 15 == 2).any() for r in range(3))


@pytest.mark.parametrize("R", [1, 8])
def test_cond_rate_counts_at_both_ends(hip, tmp_path, R):
    c = synth(hip, tmp_path, R=R, n_samples=2, n_leaves=17, seed=8 if R == 1 else 9)
    _check_cond(c, [(i, t) for t in (1, 6, 11, 17) for i in range(2)])


@pytest.mark.parametrize("preset", ["mixed_n", "mixed_n_deep"])
def test_cond_n_inside_columns(hip, tmp_path, preset):
    """N inside columns and all-N columns; the balanced 64-leaf tree (schedule stack >= 5: the MRCA form's upward pass
    keeps only what its stack needs)."""
    kw = {"mixed_n": dict(n_leaves=20, n_samples=3, seed=42, ragged=6, ambiguous=0.02),
          "mixed_n_deep": dict(n_leaves=64, n_samples=2, seed=49, tree_shape="balanced", n_nni=0, ragged=6, ambiguous=0.01)}
    c = synth(hip, tmp_path, **kw[preset])
    if preset == "mixed_n_deep":
        assert c.depth >= 5
    n_n = (c.o.msa == 4).sum(axis=0)
    assert ((n_n > 0) & (n_n < c.o.msa.shape[0])).any() and (n_n == c.o.msa.shape[0]).any()
    _check_cond(c, [(i, t) for t in range(1, c.T, 7) for i in range(len(c.rows))])


def test_cond_ladder_of_forty(hip, tmp_path):
    """A ladder-shaped 40-leaf tree with the deepest tip as the seed: a chain of 39."""
    rng = np.random.default_rng(6)

    def ladder(rows):
        import re
        leaves = [lab for lab in re.findall(r"[(,]([^(),:;\[]+)[\[:]", rows[0]["tree"]) if lab != "naive"]
        assert len(leaves) == 40
        bl = lambda: "%.6f" % max(rng.exponential(0.02), 1e-4)
        sub = "(%s:%s,%s:%s)" % (leaves[-2], bl(), leaves[-1], bl())
        for lab in reversed(leaves[1:-2]):
            sub = "(%s:%s,%s:%s)" % (lab, bl(), sub, bl())
        return [dict(rows[0], tree="(naive:%s,%s:%s,%s:%s);" % (bl(), leaves[0], bl(), sub, bl()))]
    c = synth(hip, tmp_path, rows=ladder, n_leaves=40, n_samples=1, seed=11)
    deepest = max(range(1, c.T), key=lambda t: len(c.path(0, t)))
    paths = _check_cond(c, [(0, deepest), (0, 1)])
    assert len(paths[0]) == 39


def test_cond_at_the_alpha_floor(hip, tmp_path):
    """alpha = 0.05, R = 8: categories whose likelihood of a column is (all but) zero contribute 0, not NaN."""
    c = synth(hip, tmp_path, R=8, rows=lambda rows: [dict(r, alpha=0.05) for r in rows], n_leaves=14, n_samples=3, seed=9005,
              locus="igk", ambiguous=0.05, tree_shape="balanced")
    _check_cond(c, [(i, t) for t in (1, 5, 14) for i in range(3)])
    res, _ = c.probs([(0, 1)], PARENT, want=("cond",))
    assert np.isfinite(res["cond"]).all()


# ---- log_cand ----

def _candidates(c, row, path, node):
    """The oracle's own ancestral draws, the one-site candidates of three sites, the 64 candidates of three sites and the
    all-open one: (candidates, {name: slice})."""
    L = c.L
    sites = [0, L // 2, L - 1]
    parts = [("draws", c.oracle_draws(row, path, node, 6, 17))] + \
        [("one%d" % j, apo.one_site(L, j)) for j in sites] + \
        [("three", apo.constrained(L, sites)), ("open", np.full((1, L), apo.OPEN, dtype=np.uint8))]
    where, at = {}, 0
    for name, a in parts:
        where[name] = slice(at, at + len(a))
        at += len(a)
    return np.concatenate([a for _, a in parts]), where, sites


def _check_log_cand(c, pairs):
    worst = 0.0
    for row, tip in pairs:
        path = c.path(row, tip)
        marg, _ = c.run([(row, tip)], want=("marg",))
        for node in NODES:
            cands, where, sites = _candidates(c, row, path, node)
            res, _ = c.probs([(row, tip)], node, cands)
            lc = res["log_cand"][0]
            want = c.oracle_log_cand(row, c.oracle_tables(row, path, node), cands)
            finite = np.isfinite(want)
            assert np.array_equal(np.isfinite(lc), finite)
            worst = max(worst, np.abs(lc[finite] - want[finite]).max())
            assert lc[where["open"]][0] == 0.0
            assert abs(np.exp(lc[where["three"]]).sum() - 1) < 1e-10
            for j in sites:
                k11 = marg["marg"][0, apo.slot_of(node, path), j]
                assert np.abs(np.exp(lc[where["one%d" % j]]) - k11).max() < 1e-10
    print("log_cand: worst difference from the oracle %.3g" % worst)
    assert worst < LOG_CAND_BOUND, worst


def test_log_cand_toy_family(hip, data_dir, tmp_path):
    c = toy_case(hip, data_dir, tmp_path)
    _check_log_cand(c, [(i, t) for i in range(2) for t in range(1, c.T)])


@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_log_cand_small_families(hip, tmp_path, locus):
    c = synth(hip, tmp_path, locus=locus, n_samples=2, seed=5 if locus == "igk" else 7)
    _check_log_cand(c, [(0, 1), (1, 4), (1, c.T - 1)])


# ---- launch shapes ----

@pytest.fixture(scope="module")
def small(hip, tmp_path_factory):
    return synth(hip, tmp_path_factory.mktemp("probs"), n_samples=5, seed=45)


def _random_candidates(L, K, seed):
    rng = np.random.default_rng(seed)
    cands = rng.integers(0, 4, size=(K, L)).astype(np.uint8)
    cands[rng.random((K, L)) < 0.6] = apo.OPEN
    return cands


@pytest.mark.parametrize("K", [1, 2, 255, 256, 257])
def test_candidate_counts(small, K):
    """K = 1, two identical candidates, and one workgroup of the pairs' kernels less one, full, and one more: every
    candidate carries the bits it has when it is registered alone."""
    c = small
    cands = _random_candidates(c.L, K, 100 + K)
    if K == 2:
        cands[1] = cands[0]
    pairs = [(0, 1), (3, 5)]
    res, _ = c.probs(pairs, MRCA, cands, want=("log_cand",))
    assert res["log_cand"].shape == (2, K) and np.isfinite(res["log_cand"]).all()
    if K == 2:
        assert np.array_equal(res["log_cand"][:, 0], res["log_cand"][:, 1])
    for k in sorted({0, K // 2, K - 1}):
        alone, _ = c.probs(pairs, MRCA, cands[k:k + 1], want=("log_cand",))
        assert np.array_equal(alone["log_cand"][:, 0], res["log_cand"][:, k])


def test_rows_do_not_depend_on_their_batch(small):
    c = small
    cands = _random_candidates(c.L, 3, 7)
    pairs = [(i, t) for i in range(3) for t in (1, 6)]
    for node in NODES:
        full, _ = c.probs(pairs, node, cands)
        for i, p in enumerate(pairs):
            alone, _ = c.probs([p], node)
            second, _ = c.probs([pairs[(i + 1) % len(pairs)], p], node)
            for key in ("loglik", "cond", "log_cand"):
                assert np.array_equal(alone[key][0], full[key][i]) and np.array_equal(second[key][1], full[key][i]), key


def _worker(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ancestral_probs_worker.py"), mode], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_a_group_of_pairs_cuts_rows_and_candidates(small):
    """LH_ANC_PAIRS=7 with n = 5 and K = 3 (read once per process: a child process): three groups of pairs, cut inside a
    row's candidates and across rows, give the bits of this process's single group."""
    from tests import ancestral_probs_worker as w
    c = small
    here, _ = c.probs([(i, 1 + i) for i in range(5)], MRCA, w.pairs_candidates(c.L), want=("log_cand", "weighted_sum"))
    there = _worker("pairs", {"LH_ANC_PAIRS": "7"})
    assert [[x.hex() for x in row] for row in here["log_cand"].tolist()] == there["log_cand"]
    assert [x.hex() for x in here["weighted_sum"].tolist()] == there["weighted_sum"]


def test_across_the_launch_group_cut():
    res = _worker("chunk", {"LH_CHUNK": "256"})
    assert res["n"] == 259 and res["groups"] == 2
    assert res["rows_checked"] == [0, 255, 256, 258]
    assert res["mismatches"] == []


def test_weighted_sums(small):
    """n = 256 + 1 rows (one past a slab of the reduction), K = 3, random log_offset: weighted_sum within n 2^-52 relative
    of a long-double host sum of the returned rows, bit-stable over two calls, and two half batches combined by
    posterior.combine within 1e-14 of the whole."""
    c = small
    n = 257
    rng = np.random.default_rng(12)
    pairs = [(i % 5, 1 + (i * 3) % (c.T - 1)) for i in range(n)]
    off = -1000.0 + 3.0 * rng.standard_normal(n)
    want = ("loglik", "log_cand", "weighted_sum", "weight_stats")
    res, _ = c.probs(pairs, PARENT, _random_candidates(c.L, 3, 9), log_offset=off, want=want)
    again, _ = c.probs(pairs, PARENT, log_offset=off, want=want)
    for k in ("weighted_sum", "weight_stats"):
        assert np.array_equal(res[k], again[k]), k
    lw = res["loglik"] - off
    m = lw.max()
    w = np.exp(lw - m)
    st = res["weight_stats"]
    assert st[0] == m and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    ref = np.tensordot(w.astype(np.longdouble), np.exp(res["log_cand"]).astype(np.longdouble), axes=1)
    assert (np.abs(res["weighted_sum"] - ref) <= n * 2.0 ** -52 * np.abs(ref)).all()
    h1 = 128
    a, _ = c.probs(pairs[:h1], PARENT, log_offset=off[:h1], want=want)
    b, _ = c.probs(pairs[h1:], PARENT, log_offset=off[h1:], want=want)
    mean, mx, s1, s2 = lp.combine([(a["weighted_sum"], a["weight_stats"]), (b["weighted_sum"], b["weight_stats"])])
    assert np.allclose(mean, res["weighted_sum"] / st[1], rtol=1e-14, atol=1e-300)
    assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]


def test_device_entry_point_on_a_torch_stream():
    """The _device form on a stream of torch's (its own process): equal to the host-pointer form; a rejected
    device-resident schedule, a path that is not a chain and a path whose last entry is not the root each give that row
    NaN and no weight and raise the handle's error word once, the other rows keep their bits."""
    res = _worker("device")
    assert res["clean_status"] == "" and res["clean_equals_host"]
    for k in ("schedule", "not_a_chain", "not_the_root"):
        assert res[k]["victim_all_nan"] and res[k]["others_unchanged"] and res[k]["weights_leave_the_victim_out"], k
        assert res[k]["second_status"] == "", k
    assert "malformed schedule" in res["schedule"]["status"]
    assert "not a chain" in res["not_a_chain"]["status"] and "not a chain" in res["not_the_root"]["status"]


# ---- refusals ----

def test_refusals(hip, tmp_path):
    c = synth(hip, tmp_path, n_samples=1, seed=37)
    pairs = [(0, 1)]
    with pytest.raises(RuntimeError, match="lh_family_set_ancestral_candidates has not been called"):
        c.probs(pairs, MRCA)
    good = _random_candidates(c.L, 2, 1)
    bad = good.copy()
    bad[1, 3] = 5
    c.hip.set_ancestral_candidates(c.family, good)
    with pytest.raises(RuntimeError, match="candidate 1, site 3: base 5"):
        c.hip.set_ancestral_candidates(c.family, bad)
    assert c.hip.ancestral_candidates_info(c.family) == (0, c.L)      # a call that fails leaves no candidates
    with pytest.raises(RuntimeError, match="K must be 1 .. 65536"):
        c.hip.set_ancestral_candidates(c.family, np.zeros((0, c.L), dtype=np.uint8))
    with pytest.raises(ValueError, match="sites"):
        c.hip.set_ancestral_candidates(c.family, good[:, :-1])
    # K6's candidates stay registered beside K13's
    c.hip.set_candidates(c.family, np.zeros((2, c.L), dtype=np.uint8))
    c.hip.set_ancestral_candidates(c.family, good)
    assert c.hip.candidates_info(c.family)[0] == 2 and c.hip.ancestral_candidates_info(c.family) == (2, c.L)
    with pytest.raises(RuntimeError, match="node must be 0"):
        c.probs(pairs, 2)
    path = c.path(0, 1)
    assert len(path) >= 2
    with pytest.raises(RuntimeError, match="is not a chain"):
        c.hip.eval_ancestral_candidates_batch(c.family, *c.args([0]), [path[::-1]], MRCA)
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    with pytest.raises(RuntimeError, match="extended-range mode"):
        c.probs(pairs, MRCA)
    capi.Family.borrow(c.family, hip).set_extended_range(False)
    res, _ = c.probs(pairs, MRCA)
    assert np.isfinite(res["log_cand"]).all()


def test_refused_without_an_msa(hip, data_dir):
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    h = orc.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    desc = db.build_family_desc(h)
    desc.msa = np.zeros(0, dtype=np.uint8)          # no alignment: a forward-only family
    fam = linearham_amd.Family(desc, hip)
    assert hip.ancestral_candidates_info(fam) == (0, 0)
    with pytest.raises(RuntimeError, match="without an MSA"):
        hip.set_ancestral_candidates(fam, np.zeros((1, 0), dtype=np.uint8))
    fam.close()


def test_output_bound_names_the_largest_n():
    """The refusal of the host-pointer form, through its hook (LH_ANC_OUT_MB=1, read once per process)."""
    res = _worker("bound", {"LH_ANC_OUT_MB": "1"})
    assert res["most"] > 8
    assert "batch too large" in res["message"] and "at most %d samples per call" % res["most"] in res["message"]
    assert res["largest_passes"]


# ---- the host library: PhyloHMM::AncestralCandidatePosterior, the pipeline over a RevBayes table, the CLI ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _check_files(res, names, cands, per_row, first):
    used = per_row[first:]
    lw = np.array([r[0] for r in used])
    w = np.exp(lw - lw.max())
    want = sum(wi * r[1] for wi, r in zip(w, used)) / w.sum()
    got = dict(zip(res["names"], res["prob"]))
    assert sorted(got) == sorted(names)
    assert max(abs(got[n] - want[k]) for k, n in enumerate(names)) < BOUND
    assert list(res["prob"]) == sorted(res["prob"], reverse=True)
    assert dict(zip(res["names"], res["seqs"])) == {n: "".join("ACGTN"[x] for x in cands[k]) for k, n in enumerate(names)}
    assert [r[0] for r in res["rows"]] == list(range(first, 9))
    assert np.allclose([r[1] for r in res["rows"]], w, rtol=1e-9)
    assert [r[2] for r in res["rows"]] == [r[2] for r in used]
    sm = res["summary"]
    assert sm["rows_used"] == 9 - first and sm["rows_skipped_nonfinite"] == 0
    assert abs(sm["kish_ess"] - w.sum() ** 2 / (w * w).sum()) < 1e-9 * sm["kish_ess"]
    full = [k for k in range(len(cands)) if (cands[k] != apo.OPEN).all()]
    assert sm["candidates"] == len(cands) and sm["candidates_constrained"] == len(full) == 3
    assert abs(sm["covered_mass"] - want[full].sum()) < BOUND and sm["covered_mass"] <= 1.0


def test_pipeline_and_cli(hip, tmp_path):
    """PhyloHMM::RunAncestralProbsPipeline on a 9-row table, through the library (burn-in 0.25) and through `linearham
    --ancestral-probs-pipeline` (no burn-in; once more with three rows per batch: byte-identical files), against the
    oracle's per-row probabilities weighted by exp(LHLogLikelihood - Likelihood); then PhyloHMM::AncestralCandidatePosterior
    and `linearham --ancestral-probs` on the first row's tree; and the one-device refusal."""
    from linearham_amd import host
    from tests.ancestral_probs_cases import ProbsCase
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=9, seed=41), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = ProbsCase(hip, yaml_path, pdir, rows, 4, tmp_path)
    tip, L = 3, c.L
    seed_seq = list(c.o.xmsa_labels)[tip]
    cands = np.concatenate([apo.constrained(L, [2, L // 2]), apo.one_site(L, 5), c.oracle_draws(0, c.path(0, tip), MRCA, 3, 5)])
    assert len({bytes(x) for x in cands}) == len(cands) == 23
    names = ["cand%d" % k for k in range(len(cands))]
    text = ["".join("ACGTN"[x] for x in row) for row in cands]
    fasta = str(tmp_path / "cands.fa")
    open(fasta, "w").write("".join(">%s\n%s\n" % (n, q) for n, q in zip(names, text)))
    per_row = []
    for i in range(9):
        path = c.path(i, tip)
        ll = c.set_row(i)
        per_row.append((ll - rows[i]["likelihood"], np.exp(c.oracle_log_cand(i, c.oracle_tables(i, path, MRCA), cands)), len(path)))
    _check_files(c.hh.run_ancestral_probs_pipeline(tsv, seed_seq, "mrca", fasta, str(tmp_path / "lib"), 4, burnin_frac=0.25), names,
                 cands, per_row, 2)
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq,
              "--candidates", fasta]
    for name, env in (("cli", {}), ("cli3", {"LH_PIPELINE_BATCH": "3"})):
        r = subprocess.run([_exe(), "--ancestral-probs-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / name),
                            "--node", "mrca"] + common, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
    _check_files(host.read_ancestral_probs(str(tmp_path / "cli")), names, cands, per_row, 0)
    for f in ("probs.tsv", "rows.tsv", "summary.tsv"):
        assert open(str(tmp_path / "cli") + "." + f, "rb").read() == open(str(tmp_path / "cli3") + "." + f, "rb").read(), f
    # one tree, the other node
    row = c.rows[0]
    path = c.path(0, tip)
    want = c.oracle_log_cand(0, c.oracle_tables(0, path, PARENT), cands)
    ll = c.set_row(0)
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one = c.hh.ancestral_candidate_posterior(seed_seq, "parent", text)
    assert one["node"] == path[0] and abs(one["loglik"] - ll) < 1e-9 * abs(ll)
    assert np.abs(one["log_cand"] - want).max() < LOG_CAND_BOUND
    newick = str(tmp_path / "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    args = [_exe(), "--ancestral-probs", "--newick-path", newick, "--alpha", repr(row["alpha"]), "--node", "parent"] + common
    args += sum([["--er", repr(x)] for x in row["er"]], []) + sum([["--pi", repr(x)] for x in row["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln.split("\t") for ln in r.stdout.strip().split("\n")]
    assert lines[0] == ["name", "sequence", "probability"] and len(lines) == 24
    got = {ln[0]: float(ln[2]) for ln in lines[1:]}
    assert max(abs(got[n] - np.exp(want[k])) for k, n in enumerate(names)) < BOUND
    r = subprocess.run([_exe(), "--ancestral-probs-pipeline", "--input-path", "x", "--output-path", "y", "--node", "mrca",
                        "--devices", "0,1"] + common, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr


# ---- what the probabilities are probabilities of ----

def _sample_states(hip, family, T, depth, ops, brl, er, pi, alpha, R, mt_seed):
    """lh_eval_sample_batch: one state path per row from the posterior, on std::mt19937(mt_seed)'s outputs."""
    import ctypes as C
    from oracle import linearham_oracle as orc
    lib = hip.lib
    n = len(alpha)
    nw, ns = lib.lh_sample_words(family), lib.lh_sample_states(family)
    rng = orc.MT19937(mt_seed)
    words = np.array([rng() for _ in range(n * nw)], dtype=np.uint32).reshape(n, nw)
    ll, st = np.zeros(n), np.zeros((n, ns), dtype=np.int32)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.lh_eval_sample_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, i32] + [f64] * 4 + \
        [C.c_int32, C.POINTER(C.c_uint32), f64, f64, i32]
    p = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(t)
    ops, brl, er, pi, alpha = (np.ascontiguousarray(ops, dtype=np.int32),) + tuple(
        np.ascontiguousarray(a, dtype=np.float64) for a in (brl, er, pi, alpha))
    hip.check(lib.lh_eval_sample_batch(family, n, T, depth, p(ops, i32), p(brl, f64), p(er, f64), p(pi, f64), p(alpha, f64), R,
                                       p(words, C.POINTER(C.c_uint32)), p(ll, f64), None, p(st, i32)))
    assert np.isfinite(ll).all()
    return st

def test_two_site_tables_against_device_draws(hip, data_dir, tmp_path):
    """20 000 draws of the device on one toy row -- lh_eval_sample_batch (naive states from the posterior),
    lh_naive_sequences, lh_asr_batch (the inner nodes under each naive sequence) -- against the exact two-site tables at
    both nodes: every cell within 5 sigma + 1/N."""
    c = toy_case(hip, data_dir, tmp_path)
    row, tip, N = 1, 1, 20000
    path = c.path(row, tip)
    assert len(path) == 2
    T, depth, ops, brl, er, pi, alpha, R = c.args([row])
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a), N, axis=0))
    fam = capi.Family.borrow(c.family, hip)
    _, ev = fam.eval_batch(T, depth, ops, brl, er, pi, alpha, R, want=("rates",))
    states = _sample_states(hip, c.family, T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(alpha), R, 5)
    naive, _ = hip.naive_sequences(c.family, states)
    anc, _ = fam.asr_batch(T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(ev["rates"]), naive, 23, 0)
    pairs_of_sites = ((5, 6), (1, c.L - 2))
    cands = np.concatenate([apo.constrained(c.L, list(s)) for s in pairs_of_sites])
    for node in NODES:
        res, _ = c.probs([(row, tip)], node, cands, want=("log_cand",))
        seqs = anc[:, path[apo.slot_of(node, path)] - T]
        for k, (a, b) in enumerate(pairs_of_sites):
            p = np.exp(res["log_cand"][0, 16 * k:16 * k + 16]).reshape(4, 4)
            freq = np.zeros((4, 4))
            np.add.at(freq, (seqs[:, a], seqs[:, b]), 1.0 / N)
            assert abs(p.sum() - 1) < 1e-10
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (node, a, b)
