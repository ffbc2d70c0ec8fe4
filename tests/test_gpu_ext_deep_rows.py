"""K4, K5, K8, K9, K10 and the evaluation forms of K11, K12, K14 and K15 in extended range, on rows where the default mode
underflows, against references that share nothing with the device's rescaling.

Everything that reads the extended-range forward arrays and K1's (value, 2^-256 count) columns AFTER the forward sweep used to
be tested on such rows through the log-likelihood alone; the crafted-emission tests of K5, K8 and K10 feed plain doubles, so
every column's count is 0 there.  Per-site counts of 4 to 14 that differ from site to site come only out of K1.  The rows
(tests/ext_deep_cases.py): four SPREAD rows (alpha = 1, branches times 0.05 to 0.2: deep columns below 2^-1074, posteriors
spread over alleles, junction states and naive bases), the four hard rows of tests/cadence_cases.py (one-hot posteriors; hard
for K1 and RatePlanes) and the two control rows.  References: doubles on the site-shifted exact emissions with forward rows
normalised by their own sum, pinned by mpmath sweeps with clamped columns (tests/test_ext_deep_cases_cpu.py); the lineage
tables from tests/exact_lineage_oracle.py.  d_ref per table is the pin's distance; every bound is max(1e-10, 8 d_ref).

One child process per family (tests/ext_deep_worker.py), each under its own time limit, one after the other; nothing is
started after a child that did not end cleanly.  The family is the one the host library reads, default K1 form; all rows of a
family in one call, control and deep rows alternating.  Asserted per row, in extended range:
  * lh_eval_batch's log-likelihood against mpmath at cadence_worker.ll_bound; every other entry point's bit for bit the same;
  * K5: compact posterior, site_base, gene posteriors at the bound; site marginals sum to 1 within 1e-12;
  * K9: windows and genes expanded with linearham_amd.posterior.codon_table against Q in frames 0, 1, 2; rows sum to 1;
  * K10: against events_oracle.dense; test_gpu_events' sum rules;
  * K8: the reference's states; log_path within 1e-12 (1 + |log_path|);
  * K4 (lh_eval_sample_batch, fixed engine words): the oracle's dense draw on the row's own device forward arrays, and -- where
    every uniform is more than 1e-7 relative from every partial sum at which the answer changes -- the draw on the reference
    alpha rows; at least three quarters of the spread rows qualify;
  * lh_eval_ancestral_batch, lh_eval_edges_batch (full and lean), lh_eval_node_codons_batch (both nodes),
    lh_eval_codon_edges_batch: every table and rate_post against the exact reference mixed with the reference site_base /
    contracted with the reference Q (hard rows: lineage_cadence_worker.COMBOS; other rows: first seed tip, frame 0); sums
    to 1; bit for bit the given-rates forms fed the device's own rates, K5 site_base and K9 table; with log_offset the
    weighted outputs and weight_stats against numpy over ALL rows, 1e-12 relative (the deep rows carry weight);
  * every distinct row alone and as row 1 of a call of two: every output bit-identical;
in default mode, same batch: non-control rows have no finite log-likelihood, NaN tables, K8 states -1; the control rows pass
all of the above at the same bounds; and between the modes the control rows' K5, K9, K10 and evaluation-form tables agree
within 1e-12 and K8 has equal bits.
LH_EXT_DEEP_DIR keeps the rows' npz, profile_gpu.txt and figures.json: per row and kernel the device's deviation, d_ref and
the bound (profiles/r27_ext_deep_rows.txt is a copy)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ext_deep_worker.py")
CHILD_TIMEOUT = 120
FAMILIES = ["cad190", "cmp180"]
FIRST = ("k5_posterior", "k5_site_base", "k5_genes", "k10_events", "k8", "k4", "loglik")


def _profile(reports, built):
    lines = ["K4-K15 on the rows of tests/ext_deep_cases.py: largest |device - reference| per row, mode and kernel (d_ref: the "
             "reference's own distance from its mpmath pin / the exact lineage tables; bound max(1e-10, 8 d_ref))"]
    for family, rep in reports.items():
        lines.append("%s: K1 form %s, %d rows in one call: %s" % (family, rep["form"], rep["rows"], " ".join(rep["kinds"])))
        for f in rep["figures"]:
            if "position" not in f:
                lines.append("  %-16s %s" % (f["row"], "  ".join("%s %s" % (k, v) for k, v in f.items() if k not in ("row", "mode"))))
                continue
            if f["mode"] == "both":
                lines.append("  %-16s at %d  the two modes: tables within %.2g, K8 equal bits: %s" % (f["row"], f["position"], f["modes_far"], f["k8_same_bits"]))
                continue
            if "default_nan_tables" in f:
                lines.append("  %-16s at %d  default: not finite, %d NaN tables, K8 states -1" % (f["row"], f["position"], f["default_nan_tables"]))
                continue
            groups = {}
            for k, v in f.items():
                if isinstance(v, dict) and "d_ref" in v:
                    g = k.split("@")[0].split("_")[0].upper()
                    d, r, b = groups.get(g, (0.0, 0.0, 0.0))
                    groups[g] = (max(d, v["d"]), max(r, v["d_ref"]), max(b, v["bound"]))
            parts = ["%s %.2g (d_ref %.2g, bound %.2g)" % ((g,) + groups[g]) for g in sorted(groups, key=lambda s: (int("".join(ch for ch in s if ch.isdigit())), s))]
            lines.append("  %-16s at %d  %-8s loglik %.2g (bound %.2g)  %s  K8 states equal: %s, log_path %.2g  K4 tier 1: %s, margin %.2g%s  "
                         "K5 sums %.2g  K10 rules %.2g" %
                         (f["row"], f["position"], f["mode"], f["loglik"]["d"], f["loglik"]["bound"], "  ".join(parts), f["k8_states_equal"],
                          f["k8_log_path"]["d"], f["k4_tier1"], f["k4_margin"], ", tier 2: %s" % f["k4_tier2"] if "k4_tier2" in f else "",
                          f["k5_sums"], f.get("k10_rules", float("nan"))))
        lines += ["  FAILED %s" % t for t in rep["failures"]]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests import ext_deep_cases as xd
    out = os.environ.get("LH_EXT_DEEP_DIR") or str(tmp_path_factory.mktemp("ext_deep"))
    os.makedirs(out, exist_ok=True)
    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    built = xd.build(out, jobs)
    reports, stopped = {}, None
    for family in FAMILIES:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, "--gpu", out, "--family", family]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            stopped = "%s: exit status %d\n%s\n%s" % (family, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
            break
        reports[family] = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(out, "profile_gpu.txt"), "w") as f:
        f.write(xd.report(built) + _profile(reports, built))
    with open(os.path.join(out, "figures.json"), "w") as f:
        json.dump(dict(reports=reports, built={k: dict(figures=v[0], d_ref=v[1]) for k, v in built.items()}), f)
    assert stopped is None, stopped
    return reports


def _failures(rep, words, without=()):
    return [t for t in rep["failures"] if any(w in t for w in words) and not any(w in t for w in without)]


@pytest.mark.parametrize("family", FAMILIES)
def test_every_row_and_table_was_checked(runs, family):
    from tests import ext_deep_cases as xd
    rep = runs[family]
    rows = xd.rows_of(family)
    n = len(rows)
    assert rep["rows"] == n == {"cad190": 10, "cmp180": 6}[family] and rep["kinds"] == [xd.kind_of(r) for r in rows]
    assert rep["kinds"][0::2] == ["control"] * (n // 2) and "control" not in rep["kinds"][1::2]
    c = rep["checked"]
    per_mode = n + n // 2              # every position in extended range, the control positions in default mode too
    for k in FIRST:
        assert c[k] == per_mode, (k, c[k])
    assert c["k9_table"] == 3 * per_mode and c["default_nan_rows"] == n // 2
    held = [r for r in rows] + [r for r in rows if xd.kind_of(r) == "control"]
    all_level = sum(sum(1 for _, f in xd.combos_of(r) if f == 0) for r in held)
    codons = sum(len(xd.combos_of(r)) for r in held)
    for k in ("k11_marg", "k11_rate_post", "k11_site_base") + tuple("k12_" + t for t in xd.K12_TABLES) + \
            tuple("k12lean_" + t for t in xd.K12_TABLES[1:]):
        assert c[k] == all_level, (k, c[k], all_level)
    for k in tuple("k15_" + t for t in xd.K15_TABLES) + tuple("k14_%s_%s" % (nd, t) for nd in ("parent", "mrca") for t in xd.K14_TABLES):
        assert c[k] == codons, (k, c[k], codons)
    distinct = len(xd.distinct_rows(family))
    assert c["independence"] == 2 * distinct and c["modes"] == n // 2
    assert c["given_rates"] == 3 * (2 + 5 + 4 + 5 + 4) + 2 * (5 + 4) and c["weighted"] == 2 + 2 + 3 + 4 + 6
    # per-row figures exist for every position in extended range and for the control positions in default mode
    seen = {(f["position"], f["mode"]) for f in rep["figures"] if "position" in f and "k5_posterior" in f}
    assert seen == {(i, "extended") for i in range(n)} | {(i, "default") for i in range(0, n, 2)}


@pytest.mark.parametrize("family", FAMILIES)
def test_loglikelihood_against_mpmath(runs, family):
    fl = _failures(runs[family], ("mpmath", "log-likelihood bit for bit"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_posteriors_codons_and_events(runs, family):
    """K5, K9 and K10 at max(1e-10, 8 d_ref), their sums and sum rules."""
    fl = _failures(runs[family], (": k5_", ": k9_", ": k10_", "K5's", "K9's", "K10's"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_viterbi_paths(runs, family):
    fl = _failures(runs[family], ("K8's",), without=("default mode", "between the modes"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_draws(runs, family):
    fl = _failures(runs[family], ("K4's",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


def test_draws_on_the_reference_forward_rows(runs):
    """Tier 2 must not be vacuous: at least three quarters of the spread rows have the margin for it, and drew those states."""
    from tests import ext_deep_cases as xd
    spread = [f for rep in runs.values() for f in rep["figures"] if f.get("kind") == "spread" and f.get("mode") == "extended"]
    assert len(spread) == len(xd.SPREAD)
    ok = [f for f in spread if f["k4_qualifies"]]
    assert 4 * len(ok) >= 3 * len(spread), [(f["row"], f["k4_margin"]) for f in spread]
    assert all(f["k4_tier2"] for f in ok)


@pytest.mark.parametrize("family", FAMILIES)
def test_evaluation_forms_against_the_exact_lineage_tables(runs, family):
    fl = _failures(runs[family], (": k11_", ": k12_", ": k12lean_", ": k14_", ": k15_", "evaluation forms do not sum"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_evaluation_forms_are_the_given_rates_forms(runs, family):
    fl = _failures(runs[family], ("given-rates forms",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_weighted_outputs_over_all_rows(runs, family):
    fl = _failures(runs[family], ("weighted outputs", "carries no weight"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_do_not_depend_on_their_batch(runs, family):
    fl = _failures(runs[family], ("not bit-identical with the batch",))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


@pytest.mark.parametrize("family", FAMILIES)
def test_default_mode(runs, family):
    """The deep rows: nothing finite, NaN tables, no path.  The control rows: the two modes agree."""
    fl = _failures(runs[family], ("default mode", "the two modes differ", "between the modes"))
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:40]))


def test_nothing_else_failed(runs):
    fl = [t for rep in runs.values() for t in rep["failures"]]
    assert not fl, "%d:\n%s" % (len(fl), "\n".join(fl[:60]))
