"""An evaluation's launch group in sub-batches: K2 of one sub-batch beside K1 of the next, on the handle's two streams.

Rows are computed independently of their neighbours (tests/test_gpu_batch_boundaries.py, tests/test_gpu_k2_forms.py hold
a row's bits whatever row shares its wave), and a sub-batch is its own rows of the launch group's workspace.  So every
output of every call must be BIT-IDENTICAL between LH_EVAL_SPLIT=1 -- the single-stream path -- and any other value; what
can go wrong is a stride of a workspace array, a K2 that starts before its K1, and a call that starts under its
predecessor's K2.  LH_EVAL_SPLIT (and LH_CHUNK) are read once per process: one run of tests/eval_overlap_worker.py per
value, one child at a time, each writing all its outputs into a file; the tests compare the files.

The shapes are the smallest that can go wrong: tools.synth_family.Spec.small (heavy chain, 23 tree samples) and the toy
family of tests/golden.

* sizes: n in {1, 2, 3, 5, 8, 9} with S in {1, 2, 3, 4} -- n < S, empty and unequal sub-batches, odd cuts that a pair of
  the V-D and D-J junction kernels straddles; loglik, forward, scaler_counts, rates, xmsa_emission; the device-pointer and
  the host-pointer entry point; profiling on: one launch group per call and a time above zero for every stage.
* launch-group edge: LH_CHUNK=256, n = 2 x 256 + 5, S = 2 and 3.
* streams: the legacy default stream and a stream of torch's that is not its default; three calls back to back with
  different inputs and nothing waited for in between against the same calls waited for one by one.
* lh_eval_sample_batch_device and lh_asr_batch_device at n = 5, S = 3 (the ancestral-sequence step has no K2 and is not
  split: it must not notice the hook).
* a malformed device schedule in the second sub-batch (row 3 of 5 at S = 3): the same NaN rows, the same
  lh_family_status, and a clean call afterwards.
* twenty handles created and destroyed with one evaluation each: no error, hipGetLastError clean."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_overlap_worker as ow

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("LH_EVAL_SPLIT", "LH_EVAL_FWD_PRIORITY", "LH_CHUNK")
SPLITS = (2, 3, 4)
FAULTED = []   # a child that was killed by a signal or ran out of time: nothing more is started on the device


def run_worker(d, name, env):
    assert not FAULTED, "no child is started after %s" % FAULTED[0]
    e = {k: v for k, v in os.environ.items() if k not in HOOKS}
    e.update(env)
    out = os.path.join(d, name + ".npz")
    try:
        r = subprocess.run([sys.executable, "-m", "tests.eval_overlap_worker", out, d], cwd=ROOT, env=e,
                           capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        FAULTED.append("%s ran out of its time" % name)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        FAULTED.append("%s ended with status %d" % (name, r.returncode))
    assert r.returncode == 0, "worker exited %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(name, json.dumps(rep["info"]))
    return rep["failures"], dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every child's (failures, outputs): "s1" .. "s4", and "chunk_s1" .. "chunk_s3" with LH_CHUNK=256."""
    import linearham_amd
    assert linearham_amd.load_library().device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    d = str(tmp_path_factory.mktemp("eval_overlap"))
    got = {}
    for s in (1,) + SPLITS:
        got["s%d" % s] = run_worker(d, "s%d" % s, {"LH_EVAL_SPLIT": str(s)})
    for s in (1, 2, 3):
        got["chunk_s%d" % s] = run_worker(d, "chunk_s%d" % s, {"LH_EVAL_SPLIT": str(s), "LH_CHUNK": str(ow.GROUP)})
    return got


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def differing(got, want, prefixes):
    keys = sorted(k for k in want if k.startswith(prefixes))
    assert keys, prefixes
    return [k for k in keys if k not in got or not same(got[k], want[k])]


def test_children_report_no_failure(runs):
    """Profile counters (one launch group per call, three with LH_CHUNK; every stage's time above zero), the handle loop
    and hipGetLastError, as each child judged them."""
    for name, (failures, _) in runs.items():
        assert failures == [], name + ": " + "\n".join(failures)


def test_single_stream_reference_is_sane(runs):
    """The S = 1 outputs the others are compared with: finite, distinct rows, the outputs written."""
    _, ref = runs["s1"]
    ll = ref["dev_n9_loglik"]
    assert np.isfinite(ll).all() and len(set(ll.tolist())) == 9
    assert (ref["dev_n9_scaler_counts"] != -7).all() and (ref["dev_n9_rates"] > 0).all()
    assert np.isfinite(ref["toy_n5_loglik"]).all() and np.isfinite(ref["handles_loglik"]).all()
    for k in ow.KEYS:   # a call's rows are the rows of a larger call
        assert same(ref["dev_n5_" + k], ref["dev_n9_" + k][:5]), k


@pytest.mark.parametrize("s", SPLITS)
def test_sizes_and_outputs(runs, s):
    _, ref = runs["s1"]
    _, got = runs["s%d" % s]
    assert differing(got, ref, ("dev_n", "host_n", "toy_n")) == []


@pytest.mark.parametrize("s", (2, 3))
def test_launch_group_edge(runs, s):
    _, ref = runs["chunk_s1"]
    _, got = runs["chunk_s%d" % s]
    assert np.isfinite(ref["groups_loglik"]).all()
    assert differing(got, ref, ("groups_",)) == []


@pytest.mark.parametrize("s", (1,) + SPLITS)
def test_streams_and_back_to_back_calls(runs, s):
    _, ref = runs["s1"]
    _, got = runs["s%d" % s]
    assert differing(got, ref, ("null_", "side_", "one_")) == []
    for i in range(3):
        for k in ow.KEYS:
            want = ref["one_%d_%s" % (i, k)]
            for stream in ("null", "side"):
                assert same(got["b2b_%s_%d_%s" % (stream, i, k)], want), (stream, i, k)
    for k in ow.KEYS:
        assert same(ref["null_" + k], ref["dev_n9_" + k]) and same(ref["side_" + k], ref["dev_n9_" + k]), k


def test_sampler_and_ancestral_entry_points(runs):
    _, ref = runs["s1"]
    _, got = runs["s3"]
    assert (ref["sample_states"] >= 0).all() and (ref["asr_anc"] <= 3).all()
    assert differing(got, ref, ("sample_", "asr_")) == []


@pytest.mark.parametrize("s", (1,) + SPLITS)
def test_malformed_schedule_in_the_second_sub_batch(runs, s):
    _, ref = runs["s1"]
    _, got = runs["s%d" % s]
    nan = np.isnan(ref["bad_loglik"])
    assert nan.tolist() == [i == ow.VICTIM for i in range(5)]
    assert "malformed schedule" in str(ref["bad_status"][0]) and str(ref["bad_status"][1]) == ""
    assert got["bad_status"].tolist() == ref["bad_status"].tolist()
    assert differing(got, ref, ("bad_loglik", "bad_rates", "bad_xmsa", "bad_forward", "bad_scaler", "after_bad_")) == []
    for k in ow.KEYS:
        assert same(got["after_bad_" + k], ref["dev_n5_" + k]), k


@pytest.mark.parametrize("s", (1,) + SPLITS)
def test_handle_lifecycle(runs, s):
    _, ref = runs["s1"]
    _, got = runs["s%d" % s]
    assert got["handles_loglik"].shape == (20, 5)
    assert same(got["handles_loglik"], np.tile(ref["toy_n5_loglik"], (20, 1)))
