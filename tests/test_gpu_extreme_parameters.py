"""K0a and K1 at extreme substitution-model parameters, against the exact reference (tests/exact_model_oracle.py).

A fixed, stratified list of rows (ROWS below: data, not a random stream) crosses
  base frequencies    U uniform | D Dirichlet(0.2), floored at 1e-6 | P1 one component at 1e-6 | P2 two components at 1e-6
  exchangeabilities   EQ all equal | K2 transitions 2, transversions 1 | K1e9 transitions 1 + 1e-9 | TNe TN93 with equal transition
                      rates (3, 3) | TNu TN93 with 1e-9-unequal ones (3, 3 (1 + 1e-9)) | LU log-uniform over six decades
                      (hence JC69 = EQ/U, F81 = EQ/skewed, K80 = K2/U, HKY = K2/skewed, each with its repeated eigenvalues, and
                      the NEARLY repeated ones of K1e9 and TNu)
  alpha               0.005, 0.02, 0.05, 1, 150, 1000, 1e4          with R in 1, 2, 4, 8
  branch lengths      a tree sample of the family scaled by 1e-2, 1, 1e2 (floor 1e-6, as the Newick reader applies it) |
                      every branch 1e-6 | every branch 100 (saturation: expm1 -> -1, every row of P -> pi)
on four families (tools/synth_family.py): ragged14 (14 leaves, ragged reads and ambiguous bases: N inside columns, the kN
kernels), plain14 (no N), balanced64 (stack depth >= 5) and, for three rows, forms_worker's mixed_500 (the segmented kernels; the
exact side on the 40 columns with the most distinct states; "q1": its tree sample with the branch lengths quantised to 16
levels, so that the exact side forms 16 R matrices instead of 1000 R).  Every (model class, alpha), (model class, branch
class) and (alpha, R) pair occurs.

Per row (tests/extreme_worker.py does the work, in a process of its own per K1 form -- the launcher's hooks are read once per
process -- reusing tests/test_gpu_parity.py's run_family and compare):
 a. rates against the exact category means: 1e-9 relative (1e-13 absolute below that), mean 1 to 1e-12;
 b. log-likelihood, rates, emissions, forward arrays, ScaleMatrix counts: compare() at its own bounds against the numpy
    oracle run with the EXACT P-matrices rounded to double (oracle.linearham_oracle.gtr_pmatrices monkeypatched; the oracle file
    does not change).  Where the plain double-precision C restatement of the same formula (oracle_kernels.c) is itself
    further than that from the exact value -- d_C, measured per row on the CPU -- the bound is max(compare's, 8 d_C): 8 for
    another summation order of the same formula (fused multiply-adds, three modes instead of four), nothing else;
 c. the emissions against the exact entries directly (no double-precision oracle in between), same rule; an exact emission
    below 1e-308 must come back 0;
 d. all of it under every K1 form (default, LH_K1_STACK, LH_K1_TABLES, LH_K1_TABLES + LH_K1_CXX_WALK, LH_K1_NO_TABLES,
    LH_K1_NO_FUSE, LH_K1_SEGMENTS), the form asserted through lh_family_prune_form; any two forms' emissions agree to 1e-13
    where the exact emission is above 1e-290, their ScaleMatrix counts exactly, and they are zero together.  The assembly
    walk tests for rescaling after every fourth op, the C++ walk (LH_K1_CXX_WALK) after every op: this is the direct check
    of that cadence;
 e. extended-range mode: finite on every row, equal to the default mode's log-likelihood to 1e-10 where that is finite;
 f. K3 (ancestral sequences) on four rows: every draw the oracle's, and no varying column drawn into a rate category whose
    exact per-rate likelihood is below 2^-1000 of the column's best.
Before any of it the numpy oracle's log-likelihood was checked finite on every row kept (python tests/extreme_worker.py
--oracle-only); the tests assert that no row was skipped.

test_batch_boundaries: tests/dev_tools/batch_boundaries.py as a test."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "extreme_worker.py")

# (family, exchangeabilities, base frequencies, alpha, R, branch lengths)
ROWS = [
    ("ragged14", "EQ", "U", 0.005, 1, "x0.01"), ("plain14", "EQ", "U", 0.02, 2, "x100"), ("ragged14", "EQ", "U", 0.05, 4, "all100"),
    ("balanced64", "EQ", "U", 1, 8, "x1"), ("ragged14", "EQ", "U", 150, 1, "all1e-6"), ("plain14", "EQ", "U", 1000, 2, "x0.01"),
    ("ragged14", "EQ", "U", 10000, 4, "x100"), ("balanced64", "EQ", "D", 0.005, 2, "x1"), ("ragged14", "EQ", "D", 0.02, 4, "all1e-6"),
    ("plain14", "EQ", "D", 0.05, 8, "x0.01"), ("ragged14", "EQ", "D", 1, 1, "x100"), ("balanced64", "EQ", "D", 150, 2, "all100"),
    ("ragged14", "EQ", "D", 1000, 4, "x1"), ("plain14", "EQ", "D", 10000, 8, "all1e-6"), ("ragged14", "EQ", "P1", 0.005, 4, "x100"),
    ("balanced64", "EQ", "P1", 0.02, 8, "all100"), ("ragged14", "EQ", "P1", 0.05, 1, "x1"), ("plain14", "EQ", "P1", 1, 2, "all1e-6"),
    ("ragged14", "EQ", "P1", 150, 4, "x0.01"), ("balanced64", "EQ", "P1", 1000, 8, "x100"), ("ragged14", "EQ", "P1", 10000, 1, "all100"),
    ("plain14", "EQ", "P2", 0.005, 8, "all1e-6"), ("ragged14", "EQ", "P2", 0.02, 1, "x0.01"), ("balanced64", "EQ", "P2", 0.05, 2, "x100"),
    ("ragged14", "EQ", "P2", 1, 4, "all100"), ("plain14", "EQ", "P2", 150, 8, "x1"), ("ragged14", "EQ", "P2", 1000, 1, "all1e-6"),
    ("balanced64", "EQ", "P2", 10000, 2, "x0.01"), ("ragged14", "K2", "U", 0.005, 1, "all100"), ("plain14", "K2", "U", 0.02, 2, "x1"),
    ("ragged14", "K2", "U", 0.05, 4, "all1e-6"), ("balanced64", "K2", "U", 1, 8, "x0.01"), ("ragged14", "K2", "U", 150, 1, "x100"),
    ("plain14", "K2", "U", 1000, 2, "all100"), ("ragged14", "K2", "U", 10000, 4, "x1"), ("balanced64", "K2", "D", 0.005, 2, "x0.01"),
    ("ragged14", "K2", "D", 0.02, 4, "x100"), ("plain14", "K2", "D", 0.05, 8, "all100"), ("ragged14", "K2", "D", 1, 1, "x1"),
    ("balanced64", "K2", "D", 150, 2, "all1e-6"), ("ragged14", "K2", "D", 1000, 4, "x0.01"), ("plain14", "K2", "D", 10000, 8, "x100"),
    ("ragged14", "K2", "P1", 0.005, 4, "x1"), ("balanced64", "K2", "P1", 0.02, 8, "all1e-6"), ("ragged14", "K2", "P1", 0.05, 1, "x0.01"),
    ("plain14", "K2", "P1", 1, 2, "x100"), ("ragged14", "K2", "P1", 150, 4, "all100"), ("balanced64", "K2", "P1", 1000, 8, "x1"),
    ("ragged14", "K2", "P1", 10000, 1, "all1e-6"), ("plain14", "K2", "P2", 0.005, 8, "x100"), ("ragged14", "K2", "P2", 0.02, 1, "all100"),
    ("balanced64", "K2", "P2", 0.05, 2, "x1"), ("ragged14", "K2", "P2", 1, 4, "all1e-6"), ("plain14", "K2", "P2", 150, 8, "x0.01"),
    ("ragged14", "K2", "P2", 1000, 1, "x100"), ("ragged14", "K2", "P2", 10000, 2, "all100"), ("ragged14", "K1e9", "U", 0.005, 1, "all1e-6"),
    ("plain14", "K1e9", "U", 0.02, 2, "x0.01"), ("ragged14", "K1e9", "U", 0.05, 4, "x100"), ("balanced64", "K1e9", "U", 1, 8, "all100"),
    ("ragged14", "K1e9", "U", 150, 1, "x1"), ("plain14", "K1e9", "U", 1000, 2, "all1e-6"), ("ragged14", "K1e9", "U", 10000, 4, "x0.01"),
    ("balanced64", "K1e9", "D", 0.005, 2, "all100"), ("ragged14", "K1e9", "D", 0.02, 4, "x1"), ("plain14", "K1e9", "D", 0.05, 8, "all1e-6"),
    ("ragged14", "K1e9", "D", 1, 1, "x0.01"), ("plain14", "K1e9", "D", 150, 2, "x100"), ("ragged14", "K1e9", "D", 1000, 4, "all100"),
    ("plain14", "K1e9", "D", 10000, 8, "x1"), ("ragged14", "K1e9", "P1", 0.005, 4, "x0.01"), ("balanced64", "K1e9", "P1", 0.02, 8, "x100"),
    ("ragged14", "K1e9", "P1", 0.05, 1, "all100"), ("plain14", "K1e9", "P1", 1, 2, "x1"), ("ragged14", "K1e9", "P1", 150, 4, "all1e-6"),
    ("balanced64", "K1e9", "P1", 1000, 8, "x0.01"), ("ragged14", "K1e9", "P1", 10000, 1, "x100"), ("plain14", "K1e9", "P2", 0.005, 8, "x1"),
    ("ragged14", "K1e9", "P2", 0.02, 1, "all1e-6"), ("balanced64", "K1e9", "P2", 0.05, 2, "x0.01"), ("ragged14", "K1e9", "P2", 1, 4, "x100"),
    ("plain14", "K1e9", "P2", 150, 8, "all100"), ("ragged14", "K1e9", "P2", 1000, 1, "x1"), ("balanced64", "K1e9", "P2", 10000, 2, "all1e-6"),
    ("ragged14", "TNe", "U", 0.005, 1, "x100"), ("plain14", "TNe", "U", 0.02, 2, "all100"), ("ragged14", "TNe", "U", 0.05, 4, "x1"),
    ("balanced64", "TNe", "U", 1, 8, "all1e-6"), ("ragged14", "TNe", "U", 150, 1, "x0.01"), ("plain14", "TNe", "U", 1000, 2, "x100"),
    ("ragged14", "TNe", "U", 10000, 4, "all100"), ("balanced64", "TNe", "D", 0.005, 2, "all1e-6"), ("ragged14", "TNe", "D", 0.02, 4, "x0.01"),
    ("plain14", "TNe", "D", 0.05, 8, "x100"), ("ragged14", "TNe", "D", 1, 1, "all100"), ("balanced64", "TNe", "D", 150, 2, "x1"),
    ("ragged14", "TNe", "D", 1000, 4, "all1e-6"), ("plain14", "TNe", "D", 10000, 8, "x0.01"), ("ragged14", "TNe", "P1", 0.005, 4, "all100"),
    ("balanced64", "TNe", "P1", 0.02, 8, "x1"), ("ragged14", "TNe", "P1", 0.05, 1, "all1e-6"), ("plain14", "TNe", "P1", 1, 2, "x0.01"),
    ("ragged14", "TNe", "P1", 150, 4, "x100"), ("plain14", "TNe", "P1", 1000, 8, "all100"), ("ragged14", "TNe", "P1", 10000, 1, "x1"),
    ("plain14", "TNe", "P2", 0.005, 8, "x0.01"), ("ragged14", "TNe", "P2", 0.02, 1, "x100"), ("balanced64", "TNe", "P2", 0.05, 2, "all100"),
    ("ragged14", "TNe", "P2", 1, 4, "x1"), ("plain14", "TNe", "P2", 150, 8, "all1e-6"), ("ragged14", "TNe", "P2", 1000, 1, "x0.01"),
    ("ragged14", "TNe", "P2", 10000, 2, "x100"), ("ragged14", "TNu", "U", 0.005, 1, "x1"), ("plain14", "TNu", "U", 0.02, 2, "all1e-6"),
    ("ragged14", "TNu", "U", 0.05, 4, "x0.01"), ("balanced64", "TNu", "U", 1, 8, "x100"), ("ragged14", "TNu", "U", 150, 1, "all100"),
    ("plain14", "TNu", "U", 1000, 2, "x1"), ("ragged14", "TNu", "U", 10000, 4, "all1e-6"), ("balanced64", "TNu", "D", 0.005, 2, "x100"),
    ("ragged14", "TNu", "D", 0.02, 4, "all100"), ("plain14", "TNu", "D", 0.05, 8, "x1"), ("ragged14", "TNu", "D", 1, 1, "all1e-6"),
    ("balanced64", "TNu", "D", 150, 2, "x0.01"), ("ragged14", "TNu", "D", 1000, 4, "x100"), ("plain14", "TNu", "D", 10000, 8, "all100"),
    ("ragged14", "TNu", "P1", 0.005, 4, "all1e-6"), ("balanced64", "TNu", "P1", 0.02, 8, "x0.01"), ("ragged14", "TNu", "P1", 0.05, 1, "x100"),
    ("plain14", "TNu", "P1", 1, 2, "all100"), ("ragged14", "TNu", "P1", 150, 4, "x1"), ("balanced64", "TNu", "P1", 1000, 8, "all1e-6"),
    ("ragged14", "TNu", "P1", 10000, 1, "x0.01"), ("plain14", "TNu", "P2", 0.005, 8, "all100"), ("ragged14", "TNu", "P2", 0.02, 1, "x1"),
    ("balanced64", "TNu", "P2", 0.05, 2, "all1e-6"), ("ragged14", "TNu", "P2", 1, 4, "x0.01"), ("plain14", "TNu", "P2", 150, 8, "x100"),
    ("ragged14", "TNu", "P2", 1000, 1, "all100"), ("balanced64", "TNu", "P2", 10000, 2, "x1"), ("ragged14", "LU", "U", 0.005, 1, "x0.01"),
    ("plain14", "LU", "U", 0.02, 2, "x100"), ("ragged14", "LU", "U", 0.05, 4, "all100"), ("balanced64", "LU", "U", 1, 8, "x1"),
    ("ragged14", "LU", "U", 150, 1, "all1e-6"), ("plain14", "LU", "U", 1000, 2, "x0.01"), ("ragged14", "LU", "U", 10000, 4, "x100"),
    ("balanced64", "LU", "D", 0.005, 2, "x1"), ("ragged14", "LU", "D", 0.02, 4, "all1e-6"), ("plain14", "LU", "D", 0.05, 8, "x0.01"),
    ("ragged14", "LU", "D", 1, 1, "x100"), ("balanced64", "LU", "D", 150, 2, "all100"), ("ragged14", "LU", "D", 1000, 4, "x1"),
    ("plain14", "LU", "D", 10000, 8, "all1e-6"), ("ragged14", "LU", "P1", 0.005, 4, "x100"), ("balanced64", "LU", "P1", 0.02, 8, "all100"),
    ("ragged14", "LU", "P1", 0.05, 1, "x1"), ("plain14", "LU", "P1", 1, 2, "all1e-6"), ("ragged14", "LU", "P1", 150, 4, "x0.01"),
    ("plain14", "LU", "P1", 1000, 8, "x100"), ("ragged14", "LU", "P1", 10000, 1, "all100"), ("plain14", "LU", "P2", 0.005, 8, "all1e-6"),
    ("ragged14", "LU", "P2", 0.02, 1, "x0.01"), ("balanced64", "LU", "P2", 0.05, 2, "x100"), ("ragged14", "LU", "P2", 1, 4, "all100"),
    ("plain14", "LU", "P2", 150, 8, "x1"), ("ragged14", "LU", "P2", 1000, 1, "all1e-6"), ("balanced64", "LU", "P2", 10000, 2, "x0.01"),
    ("ragged14", "K2", "D", 0.005, 8, "all1e-6"), ("ragged14", "EQ", "U", 0.02, 8, "all1e-6"), ("balanced64", "EQ", "U", 0.005, 8, "all1e-6"),
    ("balanced64", "LU", "P1", 0.02, 8, "all1e-6"), ("balanced64", "K1e9", "P2", 0.005, 8, "x0.01"),
    ("mixed_500", "EQ", "U", 0.02, 8, "q1"), ("mixed_500", "K2", "U", 1, 4, "q1"), ("mixed_500", "K1e9", "U", 0.005, 8, "q1"),
]

# The form lh_family_prune_form must report, per hook and family (%N: the family's N-awareness).  The patterns are those of
# tests/test_gpu_forms.py for the same hooks; where the launcher (lh_prune.hip launch_prune) does not let a hook act on a
# shape -- the register-stack and segmented kernels hold at most four stack slots, balanced64 needs five or more; mixed_500
# is never fused -- the form expected is the one the launcher documents for that shape.  %F: balanced64 has more than 128 site
# patterns (two waves per rate), so its rates share a workgroup up to R = 4 and take one each at R = 8.
SMALL, DEEP, LARGE = ("ragged14", "plain14"), ("balanced64",), ("mixed_500",)
N_AWARE = {"ragged14": "true", "plain14": "false", "balanced64": "false", "mixed_500": "true"}
FORMS = {
    "default": ({}, {SMALL: r"ct[456]<4,%N,true,true>", DEEP: r"ct[456]<16,%N,%F,true>", LARGE: r"seg4<4,%N>"}),
    "stack": ({"LH_K1_STACK": "1"}, {SMALL: r"w[456]<[34],%N>", DEEP: r"ct[456]<16,%N,%F,true>", LARGE: r"seg4<4,%N>"}),
    "tables": ({"LH_K1_TABLES": "1"}, {SMALL: r"ct[456]<4,%N,true,true>", DEEP: r"ct[456]<16,%N,%F,true>",
                                      LARGE: r"ct[456]<4,%N,false,true>"}),
    "tables_cxx": ({"LH_K1_TABLES": "1", "LH_K1_CXX_WALK": "1"},
                   {SMALL: r"ct[456]<4,%N,true,false>", DEEP: r"ct[456]<16,%N,%F,false>", LARGE: r"ct[456]<4,%N,false,false>"}),
    "no_tables": ({"LH_K1_NO_TABLES": "1"}, {SMALL: r"ct[456]<4,%N,true,true>", DEEP: r"ct[456]<16,%N,%F,true>",
                                            LARGE: r"ct[456]<4,%N,false,true>"}),
    "no_fuse": ({"LH_K1_NO_FUSE": "1"}, {SMALL: r"ct[456]<4,%N,false,true>", DEEP: r"ct[456]<16,%N,false,true>",
                                        LARGE: r"seg4<4,%N>"}),
    "segments": ({"LH_K1_SEGMENTS": "1"}, {SMALL: r"seg4<4,%N>", DEEP: r"ct[456]<16,%N,false,true>", LARGE: r"seg4<4,%N>"}),
}
HOOKS = ("LH_K1_TABLES", "LH_K1_STACK", "LH_K1_NO_TABLES", "LH_K1_CXX_WALK", "LH_K1_NO_FUSE", "LH_K1_SEGMENTS", "LH_K1_SEG_WAVES",
         "LH_K1_TILE_CAP")


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The exact side of every row (CPU, a pool of processes), then every K1 form and the extended-range mode over all rows,
    each in a child process of its own, side by side.  LH_EXTREME_DIR keeps the files (figures.json: every run's numbers)."""
    out = os.environ.get("LH_EXTREME_DIR") or str(tmp_path_factory.mktemp("extreme"))
    os.makedirs(out, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    jobs = max(1, min(12, len(os.sched_getaffinity(0))))
    r = subprocess.run([sys.executable, WORKER, "--exact", out, "--jobs", str(jobs)], capture_output=True, text=True,
                       timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, "%s\n%s" % (r.stdout[-2000:], r.stderr[-4000:])
    procs = {}
    for tag, hooks in [(t, f[0]) for t, f in FORMS.items()] + [("extended", {})]:
        cmd = [sys.executable, WORKER, "--gpu", out, "--tag", tag] + (["--extended"] if tag == "extended" else [])
        procs[tag] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(env, **hooks), cwd=ROOT)
    reports = {}
    try:
        for tag, p in procs.items():
            so, se = p.communicate(timeout=1500)
            assert p.returncode == 0, "%s: %s\n%s" % (tag, so[-2000:], se[-4000:])
            reports[tag] = json.loads(so.strip().splitlines()[-1])
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    with open(os.path.join(out, "figures.json"), "w") as f:
        json.dump(reports, f)
    return out, reports


@pytest.mark.parametrize("tag", list(FORMS))
def test_every_row_in_every_form(runs, tag):
    """(a), (b), (c) of the module docstring on every row under one K1 form, and that the form ran."""
    _, reports = runs
    rep = reports[tag]
    assert rep["rows"] == len(ROWS) == len(rep["figures"]), "no row may be skipped"
    for families, pattern in FORMS[tag][1].items():
        for fam in families:
            assert rep["forms"][fam] and all(re.fullmatch(pattern.replace("%N", N_AWARE[fam]).replace("%F", "(true|false)"), f) for f in rep["forms"][fam]), \
                (tag, fam, rep["forms"][fam], pattern)
    assert not rep["failures"], "%d rows:\n%s" % (len(rep["failures"]), "\n".join(rep["failures"]))


@pytest.mark.parametrize("tag", [t for t in FORMS if t != "default"])
def test_forms_agree_with_each_other(runs, tag):
    """(d): emissions and ScaleMatrix counts of a hooked form against the default form's -- hence of any two forms: counts
    exactly, values to 1e-13 relative wherever the exact emission is above 1e-290 (on the other columns: wherever either
    form's is), zero together below 1e-308.  "tables_cxx" against "default" is the C++ walk (rescaling test after every op)
    against the assembly walk (after every fourth)."""
    out, _ = runs
    a, b = np.load(os.path.join(out, "gpu_default.npz")), np.load(os.path.join(out, "gpu_%s.npz" % tag))
    bad = []
    for i in range(len(ROWS)):
        x = np.load(os.path.join(out, "row%d.npz" % i))
        ea, eb = a["em%d" % i], b["em%d" % i]
        exact = np.full(ea.shape, np.nan)
        exact[x["columns"]] = x["emission"]
        big = np.where(np.isnan(exact), np.maximum(ea, eb), exact) > 1e-290
        with np.errstate(all="ignore"):
            d = float(np.max(np.abs(ea[big] - eb[big]) / eb[big])) if big.any() else 0.0
        tiny = np.nan_to_num(exact, nan=1.0) < 1e-308
        if not np.array_equal(a["sc%d" % i], b["sc%d" % i]):
            bad.append("row %d %r: ScaleMatrix counts differ" % (i, ROWS[i]))
        if not d <= 1e-13:
            bad.append("row %d %r: emissions differ by %.3g" % (i, ROWS[i], d))
        if not (np.array_equal(ea == 0, eb == 0) and np.all(ea[tiny] == 0)):
            bad.append("row %d %r: not zero together" % (i, ROWS[i]))
    assert not bad, "\n".join(bad)


def test_extended_range_mode(runs):
    """(e): finite on every row; the default mode's log-likelihood to 1e-10 wherever that is finite."""
    out, reports = runs
    assert reports["extended"]["rows"] == len(ROWS) and not reports["extended"]["failures"], reports["extended"]["failures"]
    a, b = np.load(os.path.join(out, "gpu_default.npz")), np.load(os.path.join(out, "gpu_extended.npz"))
    for i in range(len(ROWS)):
        d, e = float(a["ll%d" % i]), float(b["ll%d" % i])
        assert np.isfinite(e), (i, ROWS[i], e)
        if np.isfinite(d):
            assert abs(e - d) <= 1e-10 * abs(d), (i, ROWS[i], e, d)


def _first_row(pred):
    return next(i for i, r in enumerate(ROWS) if r[0] in SMALL and pred(r))


ASR_ROWS = {"jc69": _first_row(lambda r: r[1:3] == ("EQ", "U")), "small_pi": _first_row(lambda r: r[2] == "P1"),
            "alpha_0.005_r8_short": _first_row(lambda r: r[3:] == (0.005, 8, "all1e-6")),
            "saturation": _first_row(lambda r: r[5] == "all100")}


@pytest.mark.parametrize("which", list(ASR_ROWS))
def test_asr_on_extreme_rows(hip, which):
    """(f): K3 draws from K1's UNMIXED per-rate planes, so a per-rate underflow that the rate mixture hides shows here."""
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tests import exact_model_oracle as ex
    from tests import extreme_worker as xw
    from tests import test_gpu_asr as ta
    i = ASR_ROWS[which]
    fams = xw.Families()
    try:
        h, base = fams.get(ROWS[i][0])
        sample, R = xw.sample_of(i, ROWS[i], base)
        mism, total, anc, choice = ta._run(hip, h, [sample], R, seed=9100 + i, first_sample=2, rng=np.random.default_rng(i))
        assert mism == 0, (mism, total)
        L, T = h.msa.shape[1], h.msa.shape[0] + 1
        naive = np.random.default_rng(i).integers(0, 5, size=(1, L)).astype(np.uint8)      # (what _run drew)
        varies = [j for j in range(L) if len(set(h.msa[:, j][h.msa[:, j] < 4])) > 1]
        assert len(varies) >= 3
        children, root, brlen = db.tree_arrays(orc.parse_newick(sample["tree"]), h.xmsa_labels)
        model = ex.ExactModel(sample["er"], sample["pi"], [float(x) for x in orc.gamma_rates_mean(sample["alpha"], R)])
        per_rate = model.prune(T, children, root, brlen, np.vstack([naive[0], h.msa]), varies)["per_rate_log2"]
        for k, j in enumerate(varies):
            assert per_rate[choice[0][j], k] >= per_rate[:, k].max() - 1000, (which, j, int(choice[0][j]), per_rate[:, k].tolist())
    finally:
        fams.close()


def test_batch_boundaries(hip, tmp_path):
    """Batch sizes around every boundary of lh_eval_batch with host pointers (staging sub-chunks of 12 288 through two pinned
    slots, launch groups of 49 152): eight distinct rows cycled to n; every row's log-likelihood, rates and scaler counts must
    carry the BITS of its row in the 8-row call (the forward arrays: tests/test_gpu_batch_boundaries.py).  The eight rows take eight of ROWS' parameter sets (those with R = 4 on unscaled branches), so
    that a line left over from a neighbour shows as another number."""
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tests import extreme_worker as xw
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_leaves=16, n_samples=8, seed=9, ragged=4, ambiguous=0.02), out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    picked = [i for i, r in enumerate(ROWS) if r[4] == 4 and r[5] == "x1"][:8]
    assert len(picked) == 8 and len(rows) == 8
    T = h.msa.shape[0] + 1
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    ops, brl, depth = [], [], 0
    for s in rows:
        children, root, brlen = db.tree_arrays(orc.parse_newick(s["tree"]), h.xmsa_labels)
        o, d = hip.schedule_tree(T, children, root)
        ops.append(o)
        brl.append(brlen)
        depth = max(depth, d)
    ops, brl = np.stack(ops), np.stack(brl)
    par = [xw.model_parameters(i, ROWS[i][1], ROWS[i][2]) for i in picked]
    er, pi = np.array([p[0] for p in par]), np.array([p[1] for p in par])
    al = np.array([float(ROWS[i][3]) for i in picked])
    assert len(set(map(tuple, pi))) + len(set(al)) > 8          # the rows are different models
    ll8, res8 = fam.eval_batch(T, depth, ops, brl, er, pi, al, 4, want=("rates", "scaler_counts"))
    assert np.all(np.isfinite(ll8)) and len(set(ll8)) == 8
    bad = []
    for n in [1, 63, 64, 65, 6143, 6144, 6145, 12287, 12288, 12289, 24577, 49151, 49152, 49153, 61441, 98305]:
        idx = np.arange(n) % 8
        ll, res = fam.eval_batch(T, depth, ops[idx], brl[idx], er[idx], pi[idx], al[idx], 4, want=("rates", "scaler_counts"))
        if not (np.array_equal(ll, ll8[idx]) and np.array_equal(res["rates"], res8["rates"][idx])):
            bad.append((n, np.nonzero(ll != ll8[idx])[0][:8].tolist()))
        sc = (res["scaler_counts"] != res8["scaler_counts"][idx]).any(axis=1)
        if sc.any():
            bad.append((n, "scaler_counts", np.nonzero(sc)[0][:8].tolist()))
    fam.close()
    assert not bad, bad
