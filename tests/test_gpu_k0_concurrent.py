"""K0a (model set-up) beside K0c (schedule rewrite) in front of every launch group's K1.

K0a reads er / pi / alpha and writes rates / eig; K0c reads ops / brlen and writes wops / wlen / tabs / hdr: neither reads
what the other writes, so an evaluation forks K0a onto one of the handle's internal streams and joins it in front of K1
(eval_device, eval_group_split in lh_capi.hip).  LH_K0_SERIAL=1 restores K0a -> K0c -> K1 in a row on one stream.  The
kernels are the same, so every output must be BIT-IDENTICAL between the two; what can go wrong is a K1 that starts before
K0a has ended, a K0a of the next launch group or the next call that overwrites rates / eig under a K1 still running, and a
K0c whose verdict on a schedule gets lost.  The hooks are read once per process: one run of tests/k0_concurrent_worker.py
per setting, one child at a time, each writing all its outputs into a file; the tests compare the files.

* families: tools.synth_family.Spec.small, heavy chain with 9 tips and light chain with 12 tips, 23 tree samples with
  different schedules.
* sizes: n in {1, 3, 130, 517} with LH_CHUNK=256 (the hook's smallest value: 130 samples are one launch group, 517 are two
  full groups and a remainder -- a K0a of the next group behind the fork while the last group's K2 still runs);
  loglik, rates, xmsa_emission, forward, scaler_counts of lh_eval_batch_device and of the host-pointer entry point;
  lh_eval_sample_batch_device at n = 130; profiling on: a time above zero for every stage.
* the same with LH_EVAL_SPLIT=2 (K0a beside the first sub-batch's K0c only).
* a corrupted schedule (row 3 of 5): that row NaN, lh_family_status reports it once, the other rows as in a clean call.
* two calls back to back on one handle with nothing waited for in between, against the same calls waited for one by one:
  the join, and the fork behind the first call's K2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import k0_concurrent_worker as kw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("LH_K0_SERIAL", "LH_EVAL_SPLIT", "LH_EVAL_FWD_PRIORITY", "LH_CHUNK")
SETTINGS = {"default": {}, "serial": {"LH_K0_SERIAL": "1"}, "split": {"LH_EVAL_SPLIT": "2"},
            "split_serial": {"LH_EVAL_SPLIT": "2", "LH_K0_SERIAL": "1"}}
PAIRS = (("default", "serial"), ("split", "split_serial"), ("split", "serial"))
FAULTED = []   # a child that was killed by a signal or ran out of time: nothing more is started on the device


def run_worker(d, name, env):
    assert not FAULTED, "no child is started after %s" % FAULTED[0]
    e = {k: v for k, v in os.environ.items() if k not in HOOKS}
    e.update(env, LH_CHUNK=str(kw.GROUP))
    out = os.path.join(d, name + ".npz")
    try:
        r = subprocess.run([sys.executable, "-m", "tests.k0_concurrent_worker", out, d], cwd=ROOT, env=e,
                           capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        FAULTED.append("%s ran out of its time" % name)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        FAULTED.append("%s ended with status %d" % (name, r.returncode))
    assert r.returncode == 0, "worker exited %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(name, json.dumps(rep["info"]))
    return rep, dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import linearham_amd
    assert linearham_amd.load_library().device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    d = str(tmp_path_factory.mktemp("k0_concurrent"))
    return {name: run_worker(d, name, env) for name, env in SETTINGS.items()}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def differing(got, want, part):
    keys = sorted(k for k in want if k.split("_", 1)[1].startswith(part))
    assert keys, part
    return [k for k in keys if k not in got or not same(got[k], want[k])]


def test_children_report_no_failure(runs):
    """every stage's time above zero and the launch groups counted, as each child judged them; the families as described"""
    for name, (rep, _) in runs.items():
        assert rep["failures"] == [], name + ": " + "\n".join(rep["failures"])
        assert rep["info"]["igh"]["tips"] == 9 and rep["info"]["igk"]["tips"] == 12
        for fam in kw.FAMILIES:
            assert rep["info"][fam]["distinct_schedules"] >= 2, (name, fam)


def test_serial_reference_is_sane(runs):
    _, ref = runs["serial"]
    for fam in kw.FAMILIES:
        ll = ref[fam + "_dev_n130_loglik"]
        assert np.isfinite(ll).all() and len(set(ll.tolist())) >= 20
        assert (ref[fam + "_dev_n517_scaler_counts"] != -7).all() and (ref[fam + "_dev_n517_rates"] > 0).all()
        assert (ref[fam + "_sample_states"] >= 0).all()
        for k in kw.KEYS:   # a call's rows are the rows of a larger call; host and device pointers agree
            assert same(ref["%s_dev_n3_%s" % (fam, k)], ref["%s_dev_n130_%s" % (fam, k)][:3]), (fam, k)
            assert same(ref["%s_host_n517_%s" % (fam, k)], ref["%s_dev_n517_%s" % (fam, k)]), (fam, k)


@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_output_is_bit_identical(runs, pair):
    _, got = runs[pair[0]]
    _, ref = runs[pair[1]]
    assert differing(got, ref, ("dev_n", "host_n", "sample_")) == []


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_corrupted_schedule(runs, setting):
    _, got = runs[setting]
    _, ref = runs["serial"]
    for fam in kw.FAMILIES:
        nan = np.isnan(got[fam + "_bad_loglik"])
        assert nan.tolist() == [i == kw.VICTIM for i in range(kw.N_BAD)], (fam, nan)
        status = got[fam + "_bad_status"].tolist()
        assert "malformed schedule" in status[0] and status[1] == "", status
        others = [i for i in range(kw.N_BAD) if i != kw.VICTIM]
        for k in kw.KEYS:
            assert same(got["%s_bad_%s" % (fam, k)][others], got["%s_clean_%s" % (fam, k)][others]), (fam, k)
            assert same(got["%s_after_bad_%s" % (fam, k)], got["%s_clean_%s" % (fam, k)]), (fam, k)
    assert differing(got, ref, ("bad_", "clean_", "after_bad_")) == []


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_back_to_back_calls(runs, setting):
    _, got = runs[setting]
    _, ref = runs["serial"]
    for fam in kw.FAMILIES:
        for i in range(len(kw.CALLS)):
            for k in kw.KEYS:
                want = ref["%s_one_%d_%s" % (fam, i, k)]
                assert np.isfinite(want).all()
                assert same(got["%s_one_%d_%s" % (fam, i, k)], want), (fam, i, k)
                assert same(got["%s_b2b_%d_%s" % (fam, i, k)], want), (fam, i, k)
