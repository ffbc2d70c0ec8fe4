"""K11 to K15 on trees whose upward pass needs more than one 2^256 rescaling per op, against an exact reference.

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

K14 and K15 (lh_node_codon.hip, lh_codon_edges.hip) run on the same tree pass and were written after that work.  A second
child per family (--gpu-codons), started after the first two and only if every child before it ended cleanly, runs the
given-rates forms lh_asr_codon_edges_batch (with cond_edge) and lh_asr_node_codons_batch (seed's parent and MRCA) on the
family as the host library reads it, the four rows in one batch, for every seed tip in frame 0 and the first seed tip in
frames 1 and 2 (every deep site takes every position in a codon), with three naive codon posteriors (the naive sequence's
triples one-hot, sparse Dirichlet rows, all mass on NNN).  The chains are 113, 115 and 80 slots on cmp180 and 152, 38 and 10
on cad190.  Asserted per row, seed tip, distribution and frame:
  * cond_edge (K15b's H) against the exact cond_edge, K15's codon_counts, aa_counts, seed_change, edge_change, edge_load and
    K14's codons and change at both nodes against the same contractions of the exact tables, at max(1e-10, 8 d_ref);
  * codon_edges_cases.rules, K14's rows summing to 1 within 1e-12, zeros in the padding slots of edge_change and edge_load;
  * on the device at 1e-12: sum_c cond_edge at slot 0 / the last slot = lh_eval_ancestral_candidates_batch's cond at the
    parent / the MRCA, sum_b q(b) cond_edge = lh_asr_edges_batch's edge, edge_change[P] = K14's change[0..2] at the MRCA;
  * for the first seed tip every row alone gives the batch's bits on its own slots;
  * the longest chain of the family's batches is above 100 slots;
and on cmp180 the evaluation forms lh_eval_codon_edges_batch and lh_eval_node_codons_batch on the control row batched with
the three deep rows (seed tip 44, frame 0): the deep rows' log-likelihoods are not finite in default mode, they hold NaN and
carry no weight, the control row keeps the bits it has alone and the weighted sums are its own within 1e-14, and its tables
are bit for bit the given-rates forms' on the evaluation's rates and the host-expanded K9 table.
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
CODON_KERNELS = {"K14": tuple("k14_%s_%s" % (n, k) for n in ("parent", "mrca") for k in ("codons", "change")),
                 "K15b": ("k15b_cond_edge",),
                 "K15": ("k15_codon_counts", "k15_aa_counts", "k15_seed_change", "k15_edge_change", "k15_edge_load")}
IDENTITIES = ("k15b_vs_k13", "k15b_vs_k12", "k15_vs_k14")


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
    codons = {}
    for family in lw.SEEDS:             # the codons children, after the others and only if each of those ended cleanly
        if stopped is not None:
            break
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, "--gpu-codons", out, "--family", family]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            stopped = "%s (codons): exit status %d\n%s\n%s" % (family, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            break
        codons[family] = json.loads(r.stdout.strip().splitlines()[-1])
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
    lines.append("K14, K15b (cond_edge) and K15 on the same rows: largest |device - exact| per row and kernel over three seed tips, "
                 "three naive-codon distributions and the frames of lineage_cadence_worker.COMBOS (d_ref: the double-precision "
                 "oracles against the same reference); K14's sums to 1; identities against K12, K13 and K14 on the device")
    for family, rep in codons.items():
        rows = []
        for f in rep["figures"]:
            if f["row"] not in rows:
                rows.append(f["row"])
        for row in rows:
            figs = [f for f in rep["figures"] if f["row"] == row]
            parts = []
            for kernel, keys in CODON_KERNELS.items():
                parts.append("%s %.2g (d_ref %.2g)" % (kernel, max(f[k] for f in figs for k in keys),
                                                       max(f["ref_" + k] for f in figs for k in keys)))
            lines.append("  %-8s %-16s %s  sums %.2g  identities %.2g  (longest chain %d)" %
                         (family, row, "  ".join(parts), max(f["sum_to_one"] for f in figs),
                          max(f[k] for f in figs for k in IDENTITIES if k in f), max(f["path"] for f in figs)))
        if "eval" in rep:
            e = rep["eval"]
            lines.append("  %-8s evaluation forms, control row with the three deep rows, chain %d: log-likelihoods %s; weighted sums "
                         "within %.2g relative of the control row's alone; given-rates forms bit-identical: %s" %
                         (family, e["chain"], e["loglik"], e["weighted_rel"], all(e["given_rates_same"].values())))
        lines += ["  FAILED %s" % t for t in rep["failures"]]
    with open(os.path.join(out, "profile_gpu.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out, "figures.json"), "w") as f:
        json.dump(dict(reports, codons=codons), f)
    assert stopped is None, stopped
    return dict(reports, codons=codons)


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


# ---- K14, K15b and K15: the codons children ----

@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_every_codon_combination_ran(runs, family):
    """Every (row, seed tip, Q kind, frame) once, and a chain above 100 slots in the family's batches (cmp180: 113 and 115,
    cad190: 152), so that K15's slot loop is stressed."""
    from tests import lineage_cadence_worker as lw
    rep = runs["codons"][family]
    assert rep["rows"] == len(lw.rows_of(family)) == 4
    seen = {(f["row"], f["tip"], f["q"], f["frame"]) for f in rep["figures"]}
    want = {(r[0], lw.SEEDS[family][si], kind, frame) for r in lw.rows_of(family) for si, frame in lw.COMBOS for kind in lw.Q_KINDS}
    assert seen == want and len(rep["figures"]) == rep["rows"] * len(lw.COMBOS) * len(lw.Q_KINDS)
    assert {f["frame"] for f in rep["figures"] if f["tip"] == lw.SEEDS[family][0]} == {0, 1, 2}
    for f in rep["figures"]:
        assert all(k in f for keys in CODON_KERNELS.values() for k in keys)
    assert rep["longest_chain"] > 100 and rep["longest_chain"] == max(f["path"] for f in rep["figures"])
    assert not _failures(rep, ("slot loop is not stressed",))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_codon_tables_against_the_exact_reference(runs, family):
    """cond_edge (K15b), K15's five tables and K14's two at both nodes, at max(1e-10, 8 d_ref)."""
    fl = _failures(runs["codons"][family], ("off the exact reference",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_codon_tables_are_distributions(runs, family):
    """codon_edges_cases.rules, K14's rows summing to 1, zeros in the padding slots."""
    fl = _failures(runs["codons"][family], ("sum rules", "do not sum to 1", "padding slots"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_codon_tables_against_the_older_kernels(runs, family):
    """sum_c cond_edge = K13b's cond at both nodes, sum_b q cond_edge = K12's edge, edge_change[P] = K14's change at the MRCA."""
    rep = runs["codons"][family]
    fl = _failures(rep, ("identities against K12, K13 and K14",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))
    for k in IDENTITIES:
        assert any(k in f for f in rep["figures"]), k


@pytest.mark.parametrize("family", ["cmp180", "cad190"])
def test_codon_rows_do_not_depend_on_their_batch(runs, family):
    fl = _failures(runs["codons"][family], ("not bit-identical alone and in the batch",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


def test_evaluation_forms_on_the_deep_rows(runs):
    """lh_eval_codon_edges_batch and lh_eval_node_codons_batch on cmp180's control row batched with its three deep rows."""
    rep = runs["codons"]["cmp180"]
    e = rep["eval"]
    assert e["chain"] > 100
    ll = e["loglik"]
    assert len(ll) == 4 and ll[0] == ll[0] and abs(ll[0]) != float("inf")
    assert all(x != x or abs(x) == float("inf") for x in ll[1:]), "a deep row has a finite log-likelihood: the case is vacuous"
    fl = _failures(rep, ("evaluation forms:",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))
    assert e["weighted_rel"] <= 1e-14 and all(e["given_rates_same"].values())
