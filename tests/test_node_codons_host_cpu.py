"""The host side of a lineage node's codon marginals, no GPU: the three writers and host.read_node_codons on files in the
pipeline's format, posterior.node_aa_table and posterior.change_classes, and the refusals that come before any device work."""
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
    codons = rng.dirichlet(np.ones(64) * 0.1, size=n)
    codons[codons < 1e-4] = 0.0
    codons[0] = 0.0
    codons[0, [0, 2, 63]] = [1.0 / 3.0, 0.5, 1e-300]   # AAA and AAG (both K), TTT
    change = rng.dirichlet(np.ones(4), size=n)
    change[1] = [0.0, 0.0, 0.0, 1.0]
    return codons, change


def test_reader_reads_what_the_writers_write(tmp_path):
    """codon, first site, node triple, probability (entries of probability 0 left out); the 64-codon amino-acid fold; one
    changes line per codon; %.17g round-trips every double."""
    codons, change = _tables()
    text = host.node_codons_write(codons, change, frame=2)
    cod, aa, chg = text.split("\n\n")
    lines = cod.split("\n")
    assert lines[0].split("\t") == ["codon", "first_site", "bases", "probability"]
    assert [ln.split("\t")[:3] for ln in lines[1:4]] == [["0", "2", "AAA"], ["0", "2", "AAG"], ["0", "2", "TTT"]]
    assert "0.33333333333333331" in lines[1]
    assert lines[4].split("\t")[:2] == ["1", "5"]
    assert aa.split("\n")[0].split("\t") == ["codon", "aa", "probability"]
    assert [ln.split("\t")[:2] for ln in aa.split("\n")[1:3]] == [["0", "F"], ["0", "K"]]
    assert chg.split("\n")[0].split("\t") == ["codon", "identical", "synonymous", "replacement", "undetermined"]
    got = host.parse_node_codons(text)
    assert np.array_equal(got["codons"], codons) and np.array_equal(got["change"], change)
    want = lp.node_aa_table(codons)
    assert len(got["aa"]) == len(want)
    for c in range(len(want)):
        assert set(got["aa"][c]) == set(want[c])
        assert max(abs(got["aa"][c][a] - want[c][a]) for a in want[c]) < 1e-15
    assert abs(got["aa"][0]["K"] - (1.0 / 3.0 + 0.5)) < 1e-15
    prefix = str(tmp_path / "out")
    for ext, part in ((".codons.tsv", cod + "\n"), (".aa.tsv", aa + "\n"), (".changes.tsv", chg)):
        open(prefix + ext, "w").write(part)
    open(prefix + ".rows.tsv", "w").write("row\tweight\tchain_length\n3\t1\t2\n4\t0.5\t3\n")
    open(prefix + ".summary.tsv", "w").write("key\tvalue\nrows_used\t2\nrows_skipped_nonfinite\t0\nkish_ess\t1.8\nframe\t2\n"
                                             "node\tmrca\nexpected_synonymous\t0.25\nexpected_replacement\t1.5\n")
    res = host.read_node_codons(prefix)
    assert np.array_equal(res["codons"], codons) and np.array_equal(res["change"], change)
    assert res["rows"] == [(3, 1.0, 2), (4, 0.5, 3)]
    assert res["summary"] == dict(rows_used=2, rows_skipped_nonfinite=0, kish_ess=1.8, frame=2, node="mrca",
                                  expected_synonymous=0.25, expected_replacement=1.5)
    # a file in another layout is not read as if it were this one
    open(prefix + ".changes.tsv", "w").write("codon\taa\tprobability\n")
    with pytest.raises(AssertionError):
        host.read_node_codons(prefix)


def test_change_classes_and_the_fold():
    """The class table against the host's translation codon by codon; the stop codons are a symbol of their own; node
    triples never hold an N, so the fold has no N rule."""
    cls = lp.change_classes()
    aa = lp.node_codon_amino_acids()
    assert cls.shape == (125, 64) and aa.count("*") == 3 and "X" not in aa
    b = "ACGTN"
    for i in (0, 2, 7, 48, 50, 124, 24, 4):  # AAA, AAG, ACT, TAA, TAG, NNN, ANN, AAN
        t = b[i // 25] + b[(i // 5) % 5] + b[i % 5]
        for x in range(64):
            u = "ACGT"[x // 16] + "ACGT"[(x // 4) % 4] + "ACGT"[x % 4]
            want = 3 if "N" in t else 0 if t == u else 1 if host.translate(t) == host.translate(u) else 2
            assert cls[i, x] == want, (t, u)
    taa, tag, tga = 25 * 3, 25 * 3 + 2, 25 * 3 + 5 * 2
    assert cls[taa, 16 * 3 + 2] == 1 and cls[taa, 16 * 3 + 4 * 2] == 1 and cls[tag, 16 * 3 + 4 * 2] == 1  # stop -> stop
    assert (cls == 0).sum() == 64 and (cls == 3).sum() == 61 * 64
    assert lp.node_aa_table(np.eye(64)[[48]]) == [{"*": 1.0}]


def test_refusals_before_any_device_work(tmp_path):
    h = _phylo()
    with pytest.raises(RuntimeError, match="node must be 0"):
        h.node_codon_marginals("anything", 2)
    with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
        h.node_codon_marginals("anything", "mrca", frame=3)
    with pytest.raises(RuntimeError, match="InitializePhyloParameters must be called first"):
        h.node_codon_marginals("anything", "mrca")
    out = str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="--node must be 'parent'"):
        h.run_node_codons_pipeline("missing.tsv", "naive", "root", out, 4)
    with pytest.raises(RuntimeError, match="node must be 0"):
        h.run_node_codons_pipeline("missing.tsv", "naive", 2, out, 4)
    with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
        h.run_node_codons_pipeline("missing.tsv", "naive", "mrca", out, 4, frame=-1)
    with pytest.raises(RuntimeError, match="burn-in fraction must be in"):
        h.run_node_codons_pipeline("missing.tsv", "naive", "mrca", out, 4, burnin_frac=1.0)
    with pytest.raises(RuntimeError, match="cannot be 'naive'"):
        h.run_node_codons_pipeline("missing.tsv", "naive", "parent", out, 4)
    with pytest.raises(RuntimeError, match="is not a sequence of this clonal family"):
        h.run_node_codons_pipeline("missing.tsv", "no-such-sequence", "parent", out, 4)
    assert not os.path.exists(out + ".codons.tsv")


def test_cli_refuses_before_it_evaluates():
    """`linearham --node-codons` with a bad --node or --frame ends before the tree is read; the pipeline takes one device."""
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    fam = ["--yaml-path", os.path.join(D, "phylo_hmm_input.yaml"), "--cluster-ind", "0", "--hmm-param-dir",
           os.path.join(D, "hmm_params"), "--seed-seq", "x"]
    common = [exe, "--node-codons"] + fam + ["--newick-path", "missing.tree"]
    r = subprocess.run(common + ["--node", "root"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--node must be 'parent'" in r.stderr
    r = subprocess.run(common + ["--node", "mrca", "--frame", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--frame must be 0, 1 or 2" in r.stderr
    r = subprocess.run([exe, "--node-codons-pipeline", "--input-path", "x", "--output-path", "y", "--node", "mrca", "--devices",
                        "0,1"] + fam, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr
