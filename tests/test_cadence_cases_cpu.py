"""tests/cadence_cases.py without a GPU: every row reaches its class on the references alone, the every-op restatement of
K1's walk is the exact value, the log-likelihood reference agrees with its independent restatements, and the rows
discriminate -- a test after every fourth op instead of every op moves the lossy rows a thousand million times the bound the
device is held to --, and one rescaling per op instead of rescaling until the largest entry is back at 2^-256 zeroes or spoils
the compound rows.  Figures: profiles/r11_rescaling_cadence_cpu.txt, profiles/r23_compound_joins_cpu.txt (python
tests/cadence_worker.py --cpu DIR --profile FILE)."""
import os

import numpy as np
import pytest

from tests import cadence_cases as cc
from tests import cadence_worker as cw


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cadence"))
    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    text, figs = cw.cpu_side(out, str(tmp_path_factory.mktemp("cadence_family")), profile=os.path.join(out, "cpu.txt"), jobs=jobs)
    return out, text, figs


def test_every_row_reaches_its_class(built):
    """cpu_side ran check_row on every row; here what the list as a whole must hold: a control per tree, a deep row, at least
    two lossy rows whose lossy columns start at different places of the four-op window, a zeroed row."""
    _, _, figs = built
    assert set(figs) == {r[0] for r in cc.ROWS}
    classes = [f["cls"] for f in figs.values()]
    assert classes.count("control") >= 2 and classes.count("deep") >= 1 and classes.count("lossy") >= 2
    assert classes.count("zeroed") >= 1, "no zeroed row: largest window fall %.0f" % min(f["entry_fall"] for f in figs.values())
    for cls in ("compound_control", "compound_clear", "compound_lossy", "compound_zeroed"):
        assert classes.count(cls) >= 1, cls
    assert {f["family"] for f in figs.values()} == set(cc.FAMILIES)
    # (what the families' exact sides cost is recorded in the profile file, not asserted: a wall-clock figure)
    assert all(f["seconds"] > 0 for f in figs.values())


def test_lossy_rows_sit_at_different_window_alignments(tmp_path):
    h = cc.load_family(cw.FAMILY, tmp_path)
    starts = {}
    for row in cc.ROWS:
        if row[2] != "lossy":
            continue
        a = cc.analyse_row(h, row)
        x = a["exact"]
        site = cc.kc.column_sites(h)
        groups = cc.walk_groups(x["ops"])
        walk_op_of_tip = {}
        for wi, g in enumerate(groups):
            for k in g:
                for t in (x["ops"][k][1], x["ops"][k][2]):
                    if 1 <= t < x["T"]:
                        walk_op_of_tip.setdefault(int(t), wi)
        off = a["dev_cols"]["w4"].max(axis=0) > 1e-3
        first = {s: f for s, f, _ in cc.FAMILIES[row[1]]["deep"]}
        starts[row[0]] = {walk_op_of_tip[first[int(t)] + 1] % 4 for t in set(site[off])}     # (tip t is alignment row t - 1)
    assert len(starts) >= 2 and len(set().union(*starts.values())) >= 2, starts


def test_every_op_restatement_is_exact_and_the_window_discriminates(built):
    """The mutation check: w = 1 agrees with the exact per-rate values to 1e-12 on every row; flipping the window to 4 puts
    the lossy and zeroed rows more than 1e8 times the device's bound (1e-12) away."""
    _, _, figs = built
    for name, f in figs.items():
        if f["cls"] in ("compound_lossy", "compound_zeroed"):
            continue                                       # test_rescale_until_is_exact_and_one_rescale_per_op_discriminates
        assert f["dev_w1"] <= 1e-12 and f["dev_w1_flush"] <= 1e-12, (name, f["dev_w1"], f["dev_w1_flush"])
        if f["cls"] == "compound_clear":
            continue                                       # (the four-op window is not what the compound rows are about)
        if f["cls"] in ("lossy", "zeroed"):
            assert f["dev_w4"] > 1e8 * 1e-12, (name, f["dev_w4"])
        else:
            assert f["dev_w4"] <= 1e-12 and f["dev_w4_no_tables"] <= 1e-12, (name, f["dev_w4"])


def test_rescale_until_is_exact_and_one_rescale_per_op_discriminates(built):
    """The mutation check of the joins: rescaling until the largest entry is back at 2^-256 agrees with the exact per-rate
    values to 1e-12 on EVERY row of both families, with and without cherry tables, and is unchanged when subnormals are
    flushed (one op's own product stays above 2^-1022: the residual reach).  One rescaling per op -- exact on every other row
    -- loses the live category's vector on the compound_zeroed row and is finitely more than 1e9 times the device's bound
    off on the compound_lossy row, whose last join lands in the subnormals."""
    _, _, figs = built
    for name, f in figs.items():
        assert max(f["dev_u1"], f["dev_u1_no_tables"], f["dev_u1_flush"]) <= 1e-12, (name, f["dev_u1"], f["dev_u1_flush"])
        assert f["join_low_u1"] > -1022, (name, f["join_low_u1"])
        assert f["depth"] <= 4, (name, f["depth"])
        if f["cls"] == "compound_zeroed":
            assert f["zeroed_w1"] and f["dev_w1"] == 1.0, (name, f["dev_w1"])
        elif f["cls"] == "compound_lossy":
            assert not f["zeroed_w1"] and 1e-3 < f["dev_w1"] < 1.0, (name, f["dev_w1"])
            assert -1074 < f["join_low_w1"] < -1022, (name, f["join_low_w1"])
        else:
            assert not f["zeroed_w1"] and f["dev_w1"] <= 1e-12, (name, f["dev_w1"])
        if f["family"] == "cmp180":
            assert f["depth"] == 4, (name, "the block's joins need a stack", f["depth"])
            if f["cls"] != "compound_control":
                assert f["deepest"] < cc.DEEP_LOG2 and f["spread"] <= cc.EXT_SPREAD_BITS, (name, f["deepest"], f["spread"])


def test_reference_against_its_restatements(built):
    """The log-likelihood reference is the mpmath forward sweep on the exact emissions (no scaling anywhere).  The
    column-scaling identity through the numpy oracle -- one integer per site, ln 2 * sum k taken off -- agrees with it to
    1e-14 wherever the numpy oracle's forward sweep is finite (the control rows: on the deep ones its ScaleMatrix, which
    rescales by the SMALLEST positive entry of a row, overflows on states five mismatches of 2^-214 apart -- documented
    reference behaviour); oc_eval_batch_ext agrees to 1e-12 on the control and deep rows.  On the lossy and zeroed rows
    oc_eval_batch_ext is off by 0.3 and more: it keeps one scaler per site for all rate categories, the saturated category
    holds it while the live one underflows."""
    _, _, figs = built
    for name, f in figs.items():
        control = f["cls"] in ("control", "compound_control")
        if control:
            assert f["d_identity"] <= 1e-14, (name, f["d_identity"])
        if control or f["cls"] == "deep":
            assert f["d_c"] <= 1e-12, (name, f["d_c"])
        else:
            assert f["d_c"] > 0.1, (name, "oc_eval_batch_ext follows the lossy rows: say so in cadence_worker.ll_bound", f["d_c"])
        assert np.isfinite(f["loglik"])
        assert f["numpy_finite"] == control


def test_entry_window_drop_sees_what_four_op_drop_misses(built):
    """A vector enters a window with its largest entry at 2^-256 or above.  On the lossy rows the largest entry then stays
    above 2^-1074 over four ops, while an entry that can reach the result goes below 2^-1022; on the zeroed row the largest
    itself can fall through."""
    _, _, figs = built
    for name, f in figs.items():
        if f["family"] != cw.FAMILY:                       # the four-op window is cad190's subject
            continue
        assert f["entry_fall"] <= f["four_op_fall"]
        if f["cls"] == "lossy":
            assert f["four_op_fall"] - 256 > -1074 and f["entry_fall"] - 256 < -1022, (name, f["four_op_fall"], f["entry_fall"])
        elif f["cls"] == "zeroed":
            assert f["four_op_fall"] - 256 < -1074, (name, f["four_op_fall"])
        else:
            assert f["entry_fall"] - 256 > -1022, (name, f["entry_fall"])
