"""Every batched entry point of the C ABI across its launch-group boundaries.

A batch is cut into staging sub-chunks (12 288 rows, two reused pinned slots), launch groups (49 152 rows over one reused
workspace; 8 192 for K3 and K7; 8192 / D for the chain) and reduction slabs (256 rows), and every piece reads and writes
at base + off * stride.  A wrong stride gives finite, plausible, wrong rows, so the reference has two steps:

1. Anchor: 23 distinct tree samples as ONE 23-row call, checked here against the CPU references with the bounds the
   per-kernel tests use (test_anchor_rows_match_the_cpu_references).
2. Position independence: in a large call row i is anchor row pick[i] = (7 i + i // G) % 23 -- position p of group k and
   of group k + 1 hold different rows -- and carries that row's BITS in every output.  Draws that depend on the sample
   number (K3, K7, the chain) have no 23-row anchor: oracle/asr_oracle.py at the row's own sample number on the rows next
   to each boundary, and the tail and the head of the batch as calls of their own with first_sample moved.

LH_CHUNK and LH_HOST_SUB are read once per process and the device forms take torch tensors: every case is one run of
tests/batch_boundaries_worker.py, one child at a time, which reports the first bad row of each output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import batch_boundaries_worker as bw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"LH_HOST_SUB": "1536", "LH_CHUNK": "1024"}
CHUNK = {"LH_CHUNK": "1024"}
SLABS = "2053,2304,2305"     # 2 x 1024 + 5, 2048 + 256 (group and slab edges coincide), 2048 + 257


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """The families and the anchors, computed once: (directory, anchors)."""
    import linearham_amd
    assert linearham_amd.load_library().device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    d = str(tmp_path_factory.mktemp("batch_boundaries"))
    return d, bw.build_anchors(d)


FAULTED = []   # a child that was killed by a signal or ran out of time: nothing more is started on the device


def run_case(work, case, env=None, timeout=180, **kw):
    assert not FAULTED, "no child is started after %s" % FAULTED[0]
    e = {k: v for k, v in os.environ.items() if k not in HOOKS}
    e.update(env or {})
    try:
        r = subprocess.run([sys.executable, "-m", "tests.batch_boundaries_worker", case, work[0]] +
                           ["%s=%s" % kv for kv in kw.items()], cwd=ROOT, env=e, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        FAULTED.append("case %s ran out of its %d s" % (case, timeout))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        FAULTED.append("case %s ended with status %d" % (case, r.returncode))
    assert r.returncode == 0, "worker exited %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res["info"]))
    assert res["failures"] == [], "\n".join(res["failures"])
    return res["info"]


# ---- 1. the anchors against the CPU references ----

def check_anchors(d, A):
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tests import naive_probs_oracle as npo
    from tests import posterior_oracle as po
    from tests.test_gpu_naive_probs import _tol
    from tests.test_gpu_parity import compare, expand_forward
    from tests.test_gpu_posterior import BOUND
    for locus, runs in (("igh", [(4, 0), (4, 1), (8, 0), (8, 1)]), ("igk", [(4, 0)])):
        F = bw.Fam(d, locus)
        o, draws = F.o, orc.PhyloHMM(F.yaml, 0, F.pdir, bw.MT_SEED)
        desc = db.build_family_desc(o)
        # the 23 samples are distinct, so a neighbour's row shows as a different number
        assert len({r["tree"] for r in F.rows}) == len(set(F.alpha)) == len({tuple(r["er"]) for r in F.rows}) == \
            len({tuple(r["pi"]) for r in F.rows}) == bw.N_SETS
        n_n = (o.msa == 4).sum(axis=0)
        assert ((n_n > 0) & (n_n < o.msa.shape[0])).any()        # N inside alignment columns: the N-aware forms run
        for R in sorted({r for r, _ in runs}):
            ref = []
            for i, s in enumerate(F.rows):
                o.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], R, is_path=False)
                o.initialize_phylo_emission()
                r = {"loglik": o.log_likelihood(), "rates": np.array(o.sr), "xmsa_emission": o.xmsa_emission.copy()}
                keys = ["vgerm_forward", "vd_junction_forward", "jgerm_forward", "vgerm_scaler_count",
                        "vd_junction_scaler_counts", "jgerm_scaler_count"]
                if o.locus == "igh":
                    keys += ["dgerm_forward", "dj_junction_forward", "dgerm_scaler_count", "dj_junction_scaler_counts"]
                for k in keys:
                    v = getattr(o, k)
                    r[k] = v.copy() if isinstance(v, np.ndarray) else v
                ref.append(r)
                if locus == "igh" and R == 4:
                    # K5, and the naive draw from the same std::mt19937 stream
                    assert np.max(np.abs(A["post_posterior"][i] - po.to_compact(o, po.smoothing(o)))) < BOUND, i
                    assert abs(A["post_loglik"][i] - r["loglik"]) <= 1e-12 * abs(r["loglik"])
                    assert abs(A["sample_loglik"][i] - r["loglik"]) <= 1e-12 * abs(r["loglik"])
                    draws.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], R, is_path=False)
                    draws.initialize_phylo_emission()
                    draws.log_likelihood()
                    assert "".join(bw.BASES[b] for b in A["naive"][i]) == draws.sample_naive_sequence(), i
            assert len({r["loglik"] for r in ref}) == bw.N_SETS
            for ext in sorted({e for r, e in runs if r == R}):
                pre = "igk_eval_" if locus == "igk" else "eval_R%d_x%d_" % (R, ext)
                res = {k[len(pre):]: A[k] for k in A if k.startswith(pre)}
                if not ext:
                    compare(o, desc, res["loglik"], res, ref)
                    continue
                # extended range scales its forward arrays differently (documented): tests/test_gpu_parity.py's
                # test_extended_range_equals_default_where_finite states what is comparable
                for i, r in enumerate(ref):
                    assert abs(res["loglik"][i] - r["loglik"]) <= 1e-10 * abs(r["loglik"]), i
                    np.testing.assert_allclose(res["rates"][i], r["rates"], rtol=1e-9)
                    np.testing.assert_allclose(res["xmsa_emission"][i], r["xmsa_emission"], rtol=1e-10)
                    ex = expand_forward(o, desc, res["forward"][i], res["scaler_counts"][i])
                    got = np.log(ex["jgerm_forward"].sum()) - ex["jgerm_scaler_count"] * np.log(2.0 ** 256)
                    assert abs(got - r["loglik"]) <= 1e-10 * abs(r["loglik"])
                    big = r["jgerm_forward"] > r["jgerm_forward"].max() * 1e-100
                    sh = (ex["jgerm_scaler_count"] - r["jgerm_scaler_count"]) * 256
                    np.testing.assert_allclose(ex["jgerm_forward"][big], np.ldexp(r["jgerm_forward"][big], sh), rtol=1e-9)
        F.close()
    # K6 on the enumerated-complete candidate set
    o, fam, sets, inp, cands = bw.toy_family()
    fam.close()
    for i, s in enumerate(sets):
        o.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        ll = o.log_likelihood()
        assert abs(A["cand_loglik"][i] - ll) < 1e-9 * abs(ll)
        # every row against the sum over all state paths; the first and the last against the factorised form too
        bf = npo.by_enumeration(o)
        assert sorted(bf) == [tuple(c) for c in cands.tolist()]
        for k, c in enumerate(cands.tolist()):
            want = np.log(bf[tuple(c)])
            assert abs(A["cand_log_cand"][i, k] - want) < _tol(ll), (i, k, A["cand_log_cand"][i, k], want)
            if i in (0, bw.N_SETS - 1):
                want = npo.log_cand(o, c, ll)
                assert abs(A["cand_log_cand"][i, k] - want) < _tol(ll), (i, k, A["cand_log_cand"][i, k], want)
        assert abs(np.exp(A["cand_log_cand"][i]).sum() - 1.0) < 1e-12


def test_anchor_rows_match_the_cpu_references(work):
    """oracle/linearham_oracle.py for log-likelihood, rates, emissions, forward arrays (1e-12 / 1e-9 / 1e-10 / 1e-9),
    scaler counts and the naive draw (exact); tests/posterior_oracle.py for K5 and tests/naive_probs_oracle.py for K6
    with their tests' bounds.  K3 has no anchor: its cases run oracle/asr_oracle.py at each row's own sample number."""
    check_anchors(*work)


# ---- 2. position independence ----

@pytest.mark.parametrize("R,ext", [(4, 0), (4, 1), (8, 0), (8, 1)])
def test_eval_batch_outputs_across_sub_chunks_and_groups(work, R, ext):
    """a. lh_eval_batch, all four optional outputs, LH_HOST_SUB=1536 and LH_CHUNK=1024: n = 2 x 1536 + 5, every sub-chunk
    in groups of 1024 + 512, the third re-entering pinned slot 0, a tail of 5.  Every edge is a multiple of 512, the group
    of pick.  R = 4 (fused K1) and 8 (unfused, K2a mixes), extended range off and on."""
    run_case(work, "eval_host", HOOKS, n=3077, G=512, R=R, ext=ext)


def test_eval_batch_outputs_light_chain(work):
    run_case(work, "eval_host", HOOKS, n=3077, G=512, locus="igk")


def test_eval_batch_outputs_across_the_real_staging_edge(work):
    """b. n = 12 289 with host pointers and no hook."""
    run_case(work, "eval_host", n=12289, G=12288)


def test_eval_batch_device_outputs_across_groups(work):
    """c. torch tensors, LH_CHUNK=1024, n = 2053, the null stream and a stream of torch's."""
    run_case(work, "eval_device", CHUNK, n=2053, G=1024)


def test_sample_batch_across_groups(work):
    """d. n = 2053 is no multiple of K4's 16 rows per workgroup; every row has its own engine words and is compared
    with a 23-row call that keeps them."""
    run_case(work, "sample", CHUNK, n=2053, G=1024)


def test_posterior_batch_across_groups_and_slabs(work):
    """e. per-row posteriors bitwise; weighted_sum and weight_stats against a long-double host sum at n 2^-52."""
    run_case(work, "posterior", CHUNK, ns=SLABS, G=1024)


def test_candidates_batch_across_groups_and_slabs(work):
    """f. The candidate set must be enumerated-complete for the rows to sum to 1; the synthetic light-chain family has
    4.3 million sequences of non-zero prior, so this case runs on the toy family of tests/golden (a few hundred), the
    family tests/test_gpu_naive_probs.py enumerates, with 23 varied models."""
    run_case(work, "candidates", CHUNK, ns=SLABS, G=1024)


def test_draw_batch_across_groups(work):
    """g. naive sequences, hashes and lh_draws_rows_read of the first, boundary and last rows."""
    run_case(work, "draw", CHUNK, n=2053, G=1024)


def test_asr_batch_past_one_group(work):
    """h. n = 8195, first_sample = 5, R = 4 and 3; then lh_asr_batch_device with rate_choice null."""
    run_case(work, "asr", n=8195, G=8192)


def test_lineage_batch_past_one_group(work):
    """i. hashes against lh_asr_batch's bases; slot P is K6c's hash of the naive sequence."""
    run_case(work, "lineage", n=8195, G=8192)


@pytest.mark.parametrize("D,n,G,env", [(3, 2 * 2730 + 3, 2730, {}), (1, 2053, 1024, CHUNK)], ids=["D3", "D1-chunk1024"])
def test_lineage_chain_past_one_group(work, D, n, G, env):
    """j. D = 3: groups of 8192 / 3 = 2730 rows; D = 1 with LH_CHUNK=1024: the evaluation's limit binds."""
    run_case(work, "chain", env, n=n, G=G, D=D)


def test_small_call_after_a_large_one(work):
    """k. grow-only buffers and the handles' last-batch records after a call of several groups."""
    run_case(work, "stale", CHUNK, n=2053, G=1024)
