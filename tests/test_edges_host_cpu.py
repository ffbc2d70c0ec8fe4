"""The host side of the lineage substitution tables, no GPU: PhyloHMM::WritePairTable, host.read_lineage_substitutions on
files in the pipeline's format, and the refusals that come before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

from linearham_amd import host

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def _text(table, n_rows, with_sum):
    lib = host.load_host()
    f = lib.lhh_write_pair_table
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    out = C.c_char_p()
    table = np.ascontiguousarray(table, dtype=np.float64)
    assert f(table.ctypes.data, table.shape[0], n_rows, int(with_sum), C.byref(out)) == 0
    return out.value.decode()


def _phylo():
    return host.PhyloHMM(os.path.join(D, "phylo_hmm_input.yaml"), 0, os.path.join(D, "hmm_params"), 0)


def test_pair_table_writer():
    """Header: site, then <ancestor><descendant> over ACGT(N) x ACGT row-major, `substitutions` last where asked for; one
    line per site; %.17g round-trips every double; the sum is the off-diagonal one of the first four rows."""
    rng = np.random.default_rng(1)
    t = rng.random((3, 4, 4))
    t[1, 2, 3] = 1.0 / 3.0
    lines = _text(t, 4, True).strip("\n").split("\n")
    assert lines[0].split("\t") == ["site"] + [a + c for a in "ACGT" for c in "ACGT"] + ["substitutions"]
    assert len(lines) == 4
    for j, ln in enumerate(lines[1:]):
        cells = ln.split("\t")
        assert cells[0] == str(j)
        got = np.array([float(x) for x in cells[1:]])
        assert np.array_equal(got[:16].reshape(4, 4), t[j])
        off = 0.0
        for a in range(4):
            for c in range(4):
                if a != c:
                    off += t[j, a, c]
        assert got[16] == off
    assert "0.33333333333333331" in lines[2]
    five = rng.random((2, 5, 4))
    lines = _text(five, 5, False).strip("\n").split("\n")
    assert lines[0].split("\t") == ["site"] + [a + c for a in "ACGTN" for c in "ACGT"]
    assert np.array_equal(np.array([float(x) for x in lines[2].split("\t")[1:]]).reshape(5, 4), five[1])


def test_reader_reads_what_the_writer_writes(tmp_path):
    rng = np.random.default_rng(2)
    L = 5
    counts, seed, naive = rng.random((L, 4, 4)), rng.random((L, 4, 4)), rng.random((L, 5, 4))
    prefix = str(tmp_path / "out")
    open(prefix + ".substitutions.tsv", "w").write(_text(counts, 4, True))
    open(prefix + ".seed_edge.tsv", "w").write(_text(seed, 4, False))
    open(prefix + ".naive_edge.tsv", "w").write(_text(naive, 5, False))
    open(prefix + ".rows.tsv", "w").write("row\tweight\tchain_length\texpected_substitutions\n3\t1\t2\t7.25\n4\t0.5\t3\t8.5\n")
    open(prefix + ".summary.tsv", "w").write("key\tvalue\nrows_used\t2\nrows_skipped_nonfinite\t0\nkish_ess\t1.8\n")
    res = host.read_lineage_substitutions(prefix)
    assert np.array_equal(res["counts"], counts) and np.array_equal(res["seed_edge"], seed)
    assert np.array_equal(res["naive_edge"], naive)
    assert np.allclose(res["substitutions"], (counts * (1 - np.eye(4))).sum(axis=(1, 2)), rtol=1e-15)
    assert res["rows"] == [(3, 1.0, 2, 7.25), (4, 0.5, 3, 8.5)]
    assert res["summary"]["rows_used"] == 2 and res["summary"]["kish_ess"] == 1.8
    # a file in another layout is not read as if it were this one
    open(prefix + ".seed_edge.tsv", "w").write(_text(naive, 5, False))
    with pytest.raises(AssertionError):
        host.read_lineage_substitutions(prefix)


def test_refusals_before_any_device_work(tmp_path):
    h = _phylo()
    with pytest.raises(RuntimeError, match="InitializePhyloParameters must be called first"):
        h.lineage_substitutions("anything")
    out = str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="burn-in fraction must be in"):
        h.run_lineage_substitutions_pipeline("missing.tsv", "naive", out, 4, burnin_frac=1.0)
    with pytest.raises(RuntimeError, match="cannot be 'naive'"):
        h.run_lineage_substitutions_pipeline("missing.tsv", "naive", out, 4)
    with pytest.raises(RuntimeError, match="is not a sequence of this clonal family"):
        h.run_lineage_substitutions_pipeline("missing.tsv", "no-such-sequence", out, 4)
    assert not os.path.exists(out + ".substitutions.tsv")
