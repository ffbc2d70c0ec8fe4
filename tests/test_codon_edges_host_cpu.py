"""The host side of the lineage's amino-acid replacements, no GPU: the three writers and host.read_lineage_replacements on
files in the pipeline's format, posterior.edge_classes and posterior.aa_symbols against the host's TranslateDna, and the
refusals that come before any device work."""
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import host
from linearham_amd import posterior as lp

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def _phylo():
    return host.PhyloHMM(os.path.join(D, "phylo_hmm_input.yaml"), 0, os.path.join(D, "hmm_params"), 0)


def _tables(n=4, seed=2):
    rng = np.random.default_rng(seed)
    aa = rng.gamma(0.05, size=(n, 21, 21))
    aa[aa < 1e-3] = 0.0
    aa[0] = 0.0
    k, r, stop = (lp.AA_SYMBOLS.index(a) for a in "KR*")
    aa[0, k, r], aa[0, r, stop], aa[0, k, k] = 1.0 / 3.0, 1e-300, 2.5
    counts = rng.gamma(1.0, size=(n, 4))
    counts[1] = [0.0, 0.0, 0.0, 1.0]
    return counts, aa, rng.dirichlet(np.ones(3), size=n)


def test_reader_reads_what_the_writers_write(tmp_path):
    """codon, first site, from, to, expected edges (the diagonal and the cells that are 0 left out); one line per codon in the
    other two; %.17g round-trips every double."""
    counts, aa, seed = _tables()
    text = host.lineage_replacements_write(counts, aa, seed, frame=2)
    rep, chg, sd = text.split("\n\n")
    lines = rep.split("\n")
    assert lines[0].split("\t") == ["codon", "first_site", "from", "to", "expected_edges"]
    assert [ln.split("\t")[:4] for ln in lines[1:3]] == [["0", "2", "K", "R"], ["0", "2", "R", "*"]]
    assert "0.33333333333333331" in lines[1]
    assert lines[3].split("\t")[:2] == ["1", "5"]
    assert chg.split("\n")[0].split("\t") == ["codon", "unchanged", "synonymous", "replacement", "undetermined"]
    assert sd.split("\n")[0].split("\t") == ["codon", "unchanged", "synonymous", "replacement"]
    got = host.parse_lineage_replacements(text)
    off = aa * (1.0 - np.eye(21))
    assert np.array_equal(got["aa_counts"], off) and np.array_equal(got["codon_counts"], counts)
    assert np.array_equal(got["seed_change"], seed)
    prefix = str(tmp_path / "out")
    for ext, part in ((".replacements.tsv", rep + "\n"), (".codon_changes.tsv", chg + "\n"), (".seed_edge.tsv", sd)):
        open(prefix + ext, "w").write(part)
    open(prefix + ".rows.tsv", "w").write("row\tweight\tchain_length\texpected_synonymous\texpected_replacement\n"
                                          "3\t1\t2\t0.5\t1.25\n4\t0.5\t3\t0\t2\n")
    open(prefix + ".summary.tsv", "w").write("key\tvalue\nrows_used\t2\nrows_skipped_nonfinite\t0\nkish_ess\t1.8\nframe\t2\n"
                                             "expected_synonymous\t0.25\nexpected_replacement\t1.5\n")
    res = host.read_lineage_replacements(prefix)
    assert np.array_equal(res["aa_counts"], off) and np.array_equal(res["codon_counts"], counts)
    assert res["rows"] == [(3, 1.0, 2, 0.5, 1.25), (4, 0.5, 3, 0.0, 2.0)]
    assert res["summary"] == dict(rows_used=2, rows_skipped_nonfinite=0, kish_ess=1.8, frame=2, expected_synonymous=0.25,
                                  expected_replacement=1.5)
    # a file in another layout is not read as if it were this one
    open(prefix + ".codon_changes.tsv", "w").write("codon\taa\tprobability\n")
    with pytest.raises(AssertionError):
        host.read_lineage_replacements(prefix)


def test_symbols_and_edge_classes_are_the_hosts_translation():
    sym, cls = lp.aa_symbols(), lp.edge_classes()
    assert sym.shape == (64,) and cls.shape == (64, 64) and sorted(set(sym)) == list(range(21))
    tri = ["ACGT"[x // 16] + "ACGT"[(x // 4) % 4] + "ACGT"[x % 4] for x in range(64)]
    for x in range(64):
        assert lp.AA_SYMBOLS[sym[x]] == host.translate(tri[x])
        for y in range(64):
            want = 0 if x == y else 1 if host.translate(tri[x]) == host.translate(tri[y]) else 2
            assert cls[x, y] == want, (tri[x], tri[y])
    assert (sym == 20).sum() == 3 and cls[tri.index("TAA"), tri.index("TGA")] == 1  # stop -> stop is silent
    assert (cls == 0).sum() == 64


def test_refusals_before_any_device_work(tmp_path):
    h = _phylo()
    with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
        h.lineage_replacements("anything", frame=3)
    with pytest.raises(RuntimeError, match="InitializePhyloParameters must be called first"):
        h.lineage_replacements("anything")
    out = str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
        h.run_lineage_replacements_pipeline("missing.tsv", "naive", out, 4, frame=-1)
    with pytest.raises(RuntimeError, match="burn-in fraction must be in"):
        h.run_lineage_replacements_pipeline("missing.tsv", "naive", out, 4, burnin_frac=1.0)
    with pytest.raises(RuntimeError, match="cannot be 'naive'"):
        h.run_lineage_replacements_pipeline("missing.tsv", "naive", out, 4)
    with pytest.raises(RuntimeError, match="is not a sequence of this clonal family"):
        h.run_lineage_replacements_pipeline("missing.tsv", "no-such-sequence", out, 4)
    assert not os.path.exists(out + ".replacements.tsv")


def test_cli_refuses_before_it_evaluates():
    """`linearham --lineage-replacements` with a bad --frame ends before the tree is read; the pipeline takes one device."""
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    fam = ["--yaml-path", os.path.join(D, "phylo_hmm_input.yaml"), "--cluster-ind", "0", "--hmm-param-dir",
           os.path.join(D, "hmm_params"), "--seed-seq", "x"]
    r = subprocess.run([exe, "--lineage-replacements"] + fam + ["--newick-path", "missing.tree", "--frame", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--frame must be 0, 1 or 2" in r.stderr
    r = subprocess.run([exe, "--lineage-replacements-pipeline", "--input-path", "x", "--output-path", "y", "--devices", "0,1"] + fam,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr
