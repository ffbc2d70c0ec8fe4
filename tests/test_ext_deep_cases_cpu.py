"""tests/ext_deep_cases.py without a GPU: the rows' conditions and the mpmath pins of their references.

The builder asserts the conditions per row (ext_deep_cases.check_row) and measures d_ref per table (pin_row); here they are
asserted again on the figures it returns, so that a row that drifted fails with its figures in the output (pytest -s shows
them for passing runs too)."""
import os

import pytest

from tests import ext_deep_cases as xd

D_REF_CEILING = 1e-10     # a pin further than this from the double-precision reference: one of the two is wrong


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = os.environ.get("LH_EXT_DEEP_DIR") or str(tmp_path_factory.mktemp("ext_deep_cpu"))
    jobs = max(1, min(8, len(os.sched_getaffinity(0))))
    return xd.build(out, jobs, with_lineage=False)


def test_report(built, capsys):
    """Per row the conditions' figures and d_ref per table, in the run's output."""
    with capsys.disabled():
        print("\n" + xd.report(built))
    assert len(built) == 10


def test_draw_margins(built):
    """K4's engine words (ext_deep_cases.k4_words): at least three quarters of the spread rows keep every uniform more than
    K4_MARGIN relative from every partial sum at which the draw on the reference forward rows changes."""
    spread = [f["k4_margin"] for f, _ in built.values() if f["kind"] == "spread"]
    assert 4 * sum(m > xd.K4_MARGIN for m in spread) >= 3 * len(spread), spread


def test_rows_and_order(built):
    names = {f: [r[0] for r in xd.rows_of(f)] for f in xd.FAMILIES}
    assert set(built) == {n for v in names.values() for n in v}
    assert sum(1 for f in built.values() if f[0]["kind"] == "spread") == 4
    assert sum(1 for f in built.values() if f[0]["kind"] == "hard") == 4
    assert sum(1 for f in built.values() if f[0]["kind"] == "control") == 2
    for f, order in names.items():      # control and deep rows alternate
        assert all(n in xd.CONTROL for n in order[0::2]) and not any(n in xd.CONTROL for n in order[1::2]), order


def test_conditions(built):
    from tests import cadence_cases as cc
    from tests import test_gpu_viterbi as tv
    for name, (f, d) in built.items():
        assert f["d_smoothing"] <= 1e-12 and f["d_q_sites"] <= 1e-12, (name, f)
        assert f["d_ll_fb"] <= 1e-12, (name, f["d_ll_fb"])
        if f["kind"] == "control":
            assert f["numpy_finite"], name
            continue
        assert f["deep_max_log2"] < -1074 and not f["numpy_finite"], (name, f)
        assert f["spread_bits"] < cc.EXT_SPREAD_BITS and len(f["counts"]) >= 3, (name, f)
        assert min(f["deep_counts"]) >= 4, (name, f["deep_counts"])
        if f["kind"] == "spread":
            assert f["vd_spread"] >= 30 and f["dj_spread"] >= 30 and f["spread_sites"] >= 15 and f["alleles"] >= 2, (name, f)
            assert f["margin"] > tv.MIN_MARGIN, (name, f["margin"])


def test_the_existing_deep_rows_are_one_hot(built):
    """Why the spread rows exist: on the hard rows hardly a junction state posterior lies in (0.01, 0.99)."""
    for name, (f, d) in built.items():
        if f["kind"] == "hard":
            assert f["vd_spread"] < 10 and f["spread_sites"] < f["vd_spread"] + f["dj_spread"] + 10, (name, f)


def test_pins(built):
    for name, (f, d) in built.items():
        full = name in xd.FULL_PIN
        # (a clamp exists for every (site, base) pair that has an xMSA column: 136 on cad190, 13 sites' worth on the other rows)
        assert f["n_site_sweeps"] >= (120 if full else 20), (name, f["n_site_sweeps"])
        assert (f["n_q_sweeps"] >= 6) == full, (name, f["n_q_sweeps"])
        assert f["n_gene_sweeps"] == 10, (name, f["n_gene_sweeps"])
        for table in ("site_base", "Q", "genes", "posterior", "events"):
            assert d[table] <= D_REF_CEILING, (name, table, d[table])
