"""K1's rescaling cadence where a LIVE rate category goes subnormal between two tests of the assembly walk
(tests/cadence_cases.py: the rows, their classes and the references; tests/test_cadence_cases_cpu.py: the same without a GPU).

The assembly walk of the cherry-table form tests for the 2^256 rescaling after every fourth walk op, on the largest entry of
the conditional-likelihood vector; the C++ walks test after every op.  On the rows here the column's emission is below
2^-1100 -- 0 in the default mode whichever walk runs -- and the entry the next mutated tip needs falls through the subnormals
between two tests of the assembly walk: a double-precision restatement of that walk is 2 to 100 % off on the live category
(`lossy`, `zeroed`), the restatement with a test after every op is exact.  So the extended-range mode, which exists to return
a finite log-likelihood on such columns, runs the every-op walk (lh_prune.hip launch_prune), and this module holds it to an
independent reference:

 a. extended range, every K1 form (the hooks of tests/test_gpu_extreme_parameters.FORMS, one child process each, the form
    asserted through lh_family_prune_form; all rows in one call): the log-likelihood of every row against the mpmath forward
    sweep on the exact emissions, at test_gpu_parity.compare's bound (1e-12; 8 d_C on a control or deep row where the C
    restatement is itself further off -- cadence_worker.ll_bound); the forms against each other: log-likelihood 1e-13,
    counts exactly;
 b. the mode's emissions column by column through K6b: log_cand - prior + loglik of a few candidate sequences against the
    exact sum of log E, at test_gpu_naive_probs' tolerance;
 c. default mode, every form: an exact emission below 1e-308 comes back 0, the log-likelihood is finite exactly where the
    numpy oracle's is, the control rows pass compare();
 d. every row bit-identical alone and as row 1 of a call of two, in extended range;
 e. K3 on the lossy and zeroed rows: every deep site draws the rate category the exact per-rate values make certain.
The same five on the compound family (cmp180: a balanced block of eight four-tip ladders spliced into the ladder of
background tips, schedule stack depth 4), where the join of two deep subtrees needs MORE THAN ONE 2^256 rescaling per op: the
C++ walks and K3b's upward pass rescale until the largest entry is back at or above 2^-256, counting each (lh_device.h
rescale_steps).  With one rescaling per op every form returned -8949.78 for -7742.19 on compound_zeroed and was 2.7e-6 off on
compound_lossy, and K3 drew the dead category on all four deep sites of compound_zeroed (profiles/r23_compound_joins_gpu.txt).
LH_CADENCE_DIR keeps the children's files and profile_gpu.txt, the figures per row and form."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_extreme_parameters import FORMS, HOOKS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cadence_worker.py")
CHILD_TIMEOUT = 120

# The forms lh_family_prune_form must report for both families (cad190: 191 tips, stack depth 1, 16 site patterns; cmp180: 181
# tips, stack depth 4 -- still within the four register slots of the <4,...> kernels; R = 2; %N: whether
# the alignment mixes N with bases -- it does not): (default mode, extended range, K3's unfused launch).  Fused, the shape
# takes the cherry-table kernel; a workgroup per (sample, rate) would hold fewer than five waves per SIMD next to a whole tip
# table, so unfused it takes the segmented register-stack kernel unless a tables hook asks for the cherry-table form.  In
# extended range, and for K3's unmixed planes in either mode, the cherry-table form runs its C++ walk (the last template
# argument).
CT, CT_CXX, CT_UNFUSED_CXX = r"ct[456]<4,false,true,true>", r"ct[456]<4,false,true,false>", r"ct[456]<4,false,false,false>"
SEG, STACK = r"seg4<4,false>", r"w[456]<[34],false>"
EXPECT = {"default": (CT, CT_CXX, SEG), "stack": (STACK, STACK, SEG), "tables": (CT, CT_CXX, CT_UNFUSED_CXX),
          "tables_cxx": (CT_CXX, CT_CXX, CT_UNFUSED_CXX), "no_tables": (CT, CT_CXX, CT_UNFUSED_CXX), "no_fuse": (SEG, SEG, SEG),
          "segments": (SEG, SEG, SEG)}
# Read off lh_family_prune_form on an MI355X and pinned, per family: (default mode, extended range, K3's unfused launch).  The
# register-stack kernel's first template argument is its number of register slots: cad190 (stack depth 1) takes the three-slot
# kernel, cmp180 (depth 4) the four-slot one; every other form has the same arguments for both.
PINNED = {
    "cad190": {"default": ("ct4<4,false,true,true>", "ct4<4,false,true,false>", "seg4<4,false>"),
               "stack": ("w4<3,false>", "w4<3,false>", "seg4<4,false>"),
               "tables": ("ct4<4,false,true,true>", "ct4<4,false,true,false>", "ct4<4,false,false,false>"),
               "tables_cxx": ("ct4<4,false,true,false>", "ct4<4,false,true,false>", "ct4<4,false,false,false>"),
               "no_tables": ("ct4<4,false,true,true>", "ct4<4,false,true,false>", "ct4<4,false,false,false>"),
               "no_fuse": ("seg4<4,false>",) * 3, "segments": ("seg4<4,false>",) * 3},
}
PINNED["cmp180"] = dict(PINNED["cad190"], stack=("w4<4,false>", "w4<4,false>", "seg4<4,false>"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The CPU side once, then one child process per hook set, one after the other, each under its own time limit; nothing
    more is started after a child that did not end cleanly."""
    from tests import cadence_worker as cw
    out = os.environ.get("LH_CADENCE_DIR") or str(tmp_path_factory.mktemp("cadence"))
    os.makedirs(out, exist_ok=True)
    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    cpu_text, cpu = cw.cpu_side(out, str(tmp_path_factory.mktemp("cadence_family")), jobs=jobs)
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    reports, stopped = {}, None
    for tag, (hooks, _) in FORMS.items():
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, "--gpu", out, "--tag", tag]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(env, **hooks), cwd=ROOT)
        if r.returncode != 0:
            stopped = "%s: exit status %d\n%s\n%s" % (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            break
        reports[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    lines = ["Rescaling cadence rows on the device: relative deviation of the extended-range log-likelihood from the reference per "
             "row and K1 form (default mode / extended range / K3), largest |log_cand - prior + loglik - sum log E| over the candidates"]
    for tag, rep in reports.items():
        lines.append("%s: %s" % (tag, "; ".join("%s %s / %s / %s" % (fam, fo["default"], fo["extended"], fo["asr"])
                                                for fam, fo in rep["forms"]["families"].items())))
        for f in rep["figures"]:
            k3 = "  K3 wrong category on %d of %d deep sites" % (f["asr_wrong"], f["asr_sites"]) if "asr_sites" in f else ""
            lines.append("  %-16s %-16s extended %.12f  reference %.12f  d %.2g (bound %.2g)  default mode %s  candidates %.2g%s" %
                         (f["row"], f["cls"], f["loglik_ext"], f["reference"], f["d_ll_ext"], f["bound"], f["loglik_default"],
                          f["d_candidates"], k3))
        for g, fl in rep["failures"].items():
            lines += ["  FAILED %s: %s" % (g, t) for t in fl]
    with open(os.path.join(out, "profile_gpu.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out, "figures.json"), "w") as f:
        json.dump(reports, f)
    assert stopped is None, stopped
    return out, reports, cpu


def _no_failures(reports, tag, group):
    fl = reports[tag]["failures"][group]
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl))


@pytest.mark.parametrize("tag", list(FORMS))
def test_forms_ran(runs, tag):
    """The form each mode's launch reports under this hook set, and that no row was skipped."""
    from tests import cadence_cases as cc
    _, reports, _ = runs
    rep = reports[tag]
    assert rep["rows"] == len(cc.ROWS) == len(rep["figures"])
    assert set(rep["forms"]["families"]) == set(cc.FAMILIES)
    for family, forms in rep["forms"]["families"].items():
        for mode, pattern, pinned in zip(("default", "extended", "asr"), EXPECT[tag], PINNED[family][tag]):
            assert re.fullmatch(pattern, forms[mode]), (tag, family, mode, forms[mode], pattern)
            assert forms[mode] == pinned, (tag, family, mode, forms[mode], pinned)


@pytest.mark.parametrize("tag", list(FORMS))
def test_extended_range_against_the_reference(runs, tag):
    """(a): every row, the lossy and zeroed ones included, within compare's bound of the mpmath forward sweep on the exact
    emissions."""
    _no_failures(runs[1], tag, "extended")


@pytest.mark.parametrize("tag", [t for t in FORMS if t != "default"])
def test_forms_agree_in_extended_range(runs, tag):
    """(a): a hooked form against the default one in extended range: log-likelihood 1e-13, counts exactly."""
    out = runs[0]
    from tests import cadence_cases as cc
    a, b = np.load(os.path.join(out, "gpu_default.npz")), np.load(os.path.join(out, "gpu_%s.npz" % tag))
    for family in cc.FAMILIES:
        la, lb = a["ll_ext_" + family], b["ll_ext_" + family]
        assert np.all(np.isfinite(la)) and np.all(np.isfinite(lb)), family
        d = np.abs(la - lb) / np.abs(la)
        assert d.max() <= 1e-13, (family, d.tolist())
        assert np.array_equal(a["sc_ext_" + family], b["sc_ext_" + family]), family


@pytest.mark.parametrize("tag", list(FORMS))
def test_candidate_emissions_in_extended_range(runs, tag):
    """(b)"""
    _no_failures(runs[1], tag, "candidates")


@pytest.mark.parametrize("tag", list(FORMS))
def test_default_mode(runs, tag):
    """(c)"""
    _no_failures(runs[1], tag, "default")


@pytest.mark.parametrize("tag", list(FORMS))
def test_rows_do_not_depend_on_their_batch(runs, tag):
    """(d)"""
    _no_failures(runs[1], tag, "independence")


@pytest.mark.parametrize("tag", list(FORMS))
def test_asr_draws_the_certain_category(runs, tag):
    """(e): K3 reads K1's unmixed planes; a category whose vector the walk zeroed would leave the draw to the dead ones."""
    _no_failures(runs[1], tag, "asr")
