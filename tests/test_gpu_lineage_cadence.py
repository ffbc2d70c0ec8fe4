"""K11, K12 and K13 on trees whose upward pass needs more than one 2^256 rescaling per op, against an exact reference.

lh_asr_marginals_batch, lh_asr_edges_batch and the ancestral-candidates tables run on lh_treepass.h's upward pass (tree_upward_pattern), which used to rescale
a conditional-likelihood vector once per op.  At the join of two subtrees that each sit up to 256 binades down that is not
enough (tests/cadence_cases.py, "Joins"): two levels later the live rate category's vector is 0, K11b's rate weights drop the
category, and the marginals of the deep columns sum to less than 1 -- or, one binade short of that, to 1 with the wrong
entries.  The double-precision numpy oracles these kernels are otherwise compared with share the benign parameters of their
tests; here the reference is tests/exact_lineage_oracle.py (mpmath, no rescaling anywhere), on the compound family's rows
and on cad190's lossy and zeroed rows, for three seed tips (cmp180: inside the block under a tip that differs, under one that
does not, on the background ladder above the block) and three naive-base distributions (the naive sequence one-hot, benign
Dirichlet rows, all mass on N).  One child process per family (tests/lineage_cadence_worker.py), each under its own time
limit; nothing more is started after a child that did not end cleanly.

Asserted per row, seed tip and distribution:
  * marg, rate_post (K11) and edge, naive_edge, chain_counts, edge_load, rate_post (K12, the full and the lean kernel) against
    the exact reference at max(1e-10, 8 d_ref), d_ref the distance of the double-precision oracles -- fed the exact
    P-matrices and an upward pass that rescales until the largest entry is back at 2^-256 -- from the same reference;
  * marginals and rate posteriors sum to 1 within 1e-12;
  * K12's four margin identities against K11's device output, 1e-12;
  * rows bit-identical alone and in the batch;
and per row and seed tip K13b's conditional tables -- lh_eval_ancestral_candidates_batch's `cond` at the seed's parent and at
the MRCA (the form that stores only what it pops), on the family as the host library reads it
(cadence_cases.write_family_files; default mode, the entry point takes no extended-range handle) -- against the exact reference at the same bound, against five one-hot calls of
lh_asr_marginals_batch at 1e-12, rows summing to 1 within 1e-12.
LH_LINEAGE_CADENCE_DIR keeps the children's files and profile_gpu.txt, d_ref and the device's deviation per row and kernel."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "lineage_cadence_worker.py")
CHILD_TIMEOUT = 120
KERNELS = {"K11": ("k11_marg", "k11_rate_post"),
           "K12": ("k12_edge", "k12_naive_edge", "k12_chain_counts", "k12_edge_load", "k12_rate_post"),
           "K12 lean": ("k12lean_naive_edge", "k12lean_chain_counts", "k12lean_edge_load", "k12lean_rate_post")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests import lineage_cadence_worker as lw
    out = os.environ.get("LH_LINEAGE_CADENCE_DIR") or str(tmp_path_factory.mktemp("lineage_cadence"))
    os.makedirs(out, exist_ok=True)
    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    cpu = lw.cpu_side(out, jobs)
    reports, stopped = {}, None
    for family in lw.SEEDS:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, "--gpu", out, "--family", family]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            stopped = "%s: exit status %d\n%s\n%s" % (family, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            break
        reports[family] = json.loads(r.stdout.strip().splitlines()[-1])
    lines = ["K11 and K12 on the compound and deep rows: largest |device - exact| per row and kernel over three seed tips and three "
             "naive-base distributions (d_ref: the double-precision oracles against the same reference); sums to 1; K12's margins "
             "against K11"]
    for family, rep in reports.items():
        rows = []
        for f in rep["figures"]:
            if f["row"] not in rows:
                rows.append(f["row"])
        for row in rows:
            figs = [f for f in rep["figures"] if f["row"] == row]
            parts = []
            for kernel, keys in KERNELS.items():
                d = max(f[k] for f in figs for k in keys)
                ref = max(v for f in figs for k, v in f.items() if k.startswith("ref_" + keys[0][:3]))
                parts.append("%s %.2g (d_ref %.2g)" % (kernel, d, ref))
            cf = [f for f in rep["cond_figures"] if f["row"] == row]
            parts.append("K13 %.2g (d_ref %.2g; against K11 %.2g)" % (max(f["k13_cond"] for f in cf), max(f["ref_k13"] for f in cf),
                                                                   max(f["k13_vs_k11"] for f in cf)))
            lines.append("  %-8s %-16s %s  sums %.2g  identities %.2g  (exact side %.1f s)" %
                         (family, row, "  ".join(parts), max(f["sum_to_one"] for f in figs + cf), max(f["identities"] for f in figs),
                          cpu[row][1]))
        lines += ["  FAILED %s" % t for t in rep["failures"]]
    with open(os.path.join(out, "profile_gpu.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out, "figures.json"), "w") as f:
        json.dump(reports, f)
    assert stopped is None, stopped
    return reports


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_every_row_ran(runs, family):
    from tests import lineage_cadence_worker as lw
    rep = runs[family]
    assert rep["rows"] == len(lw.rows_of(family)) == 4
    assert len(rep["figures"]) == rep["rows"] * len(lw.SEEDS[family]) * len(lw.Q_KINDS)
    # the three seed tips' paths differ: through the block, and above it
    assert len({(f["tip"], f["path"]) for f in rep["figures"]}) >= 3
    assert len(rep["cond_figures"]) == rep["rows"] * len(lw.SEEDS[family]) * 2


def _failures(rep, words):
    return [t for t in rep["failures"] if any(w in t for w in words)]


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_tables_against_the_exact_reference(runs, family):
    fl = _failures(runs[family], ("off the exact reference",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_tables_are_distributions(runs, family):
    fl = _failures(runs[family], ("do not sum to 1", "padding slots"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_edge_margins_are_the_node_tables(runs, family):
    fl = _failures(runs[family], ("K12's margins against K11",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_rows_do_not_depend_on_their_batch(runs, family):
    fl = _failures(runs[family], ("not bit-identical",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_conditional_tables_are_five_one_hot_marginals(runs, family):
    """K13b's cond against K11's device output for the five naive basis vectors."""
    fl = _failures(runs[family], ("five one-hot K11 calls",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))
