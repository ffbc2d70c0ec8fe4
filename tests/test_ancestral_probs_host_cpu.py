"""The host side of the candidate ancestral sequences' probabilities, no GPU: WriteAncestralProbsTable and
host.read_ancestral_probs on files in the pipeline's format, the named candidate file, --node, and the refusals that come
before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import host

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
L = 15   # the toy family's alignment


def _text(names, seqs, prob):
    lib = host.load_host()
    f = lib.lhh_write_ancestral_probs_table
    f.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double)]
    out, covered = C.c_char_p(), C.c_double()
    prob = np.ascontiguousarray(prob, dtype=np.float64)
    assert f("\n".join(names).encode(), "\n".join(seqs).encode(), prob.ctypes.data, len(names), C.byref(out), C.byref(covered)) == 0
    return out.value.decode(), covered.value


def _phylo():
    return host.PhyloHMM(os.path.join(D, "phylo_hmm_input.yaml"), 0, os.path.join(D, "hmm_params"), 0)


def test_reader_reads_what_the_writer_writes(tmp_path):
    """name, sequence, probability; ranked by probability, ties in file order; %.17g round-trips every double; the covered
    mass counts the candidates without an open site."""
    names = ["a", "b", "c", "d"]
    seqs = ["ACGTACGTACGTACG", "ACGTACGTACGTACN", "CCGTACGTACGTACG", "GCGTACGTACGTACG"]
    prob = [0.25, 1.0 / 3.0, 0.25, 1e-300]
    text, covered = _text(names, seqs, prob)
    lines = text.strip("\n").split("\n")
    assert lines[0].split("\t") == ["name", "sequence", "probability"]
    assert [ln.split("\t")[0] for ln in lines[1:]] == ["b", "a", "c", "d"]
    assert "0.33333333333333331" in lines[1]
    assert covered == 0.25 + 0.25 + 1e-300
    prefix = str(tmp_path / "out")
    open(prefix + ".probs.tsv", "w").write(text)
    open(prefix + ".rows.tsv", "w").write("row\tweight\tchain_length\n3\t1\t2\n4\t0.5\t3\n")
    open(prefix + ".summary.tsv", "w").write("key\tvalue\nrows_used\t2\nrows_skipped_nonfinite\t0\nkish_ess\t1.8\ncandidates\t4\n"
                                             "candidates_constrained\t3\ncovered_mass\t0.5\n")
    res = host.read_ancestral_probs(prefix)
    assert res["names"] == ["b", "a", "c", "d"] and res["seqs"] == [seqs[1], seqs[0], seqs[2], seqs[3]]
    assert np.array_equal(res["prob"], [prob[1], prob[0], prob[2], prob[3]])
    assert res["rows"] == [(3, 1.0, 2), (4, 0.5, 3)]
    assert res["summary"] == dict(rows_used=2, rows_skipped_nonfinite=0, kish_ess=1.8, candidates=4, candidates_constrained=3,
                                  covered_mass=0.5)
    # a file in another layout is not read as if it were this one
    open(prefix + ".probs.tsv", "w").write("rank\tNaiveSequence\tprobability\n")
    with pytest.raises(AssertionError):
        host.read_ancestral_probs(prefix)


def _file(tmp_path, text):
    p = str(tmp_path / "cands.fa")
    open(p, "w").write(text)
    return p


def test_named_candidate_file(tmp_path):
    a, b = "ACGTACGTACGTACG", "acgtnnnnnnnnnnn"
    got = host.read_named_candidates(_file(tmp_path, ">first the rest of the header\n%s\n\n>second\n%s\n%s\n" % (a, b[:7], b[7:])), L)
    assert got == [("first", a), ("second", b.upper())]
    assert host.read_named_candidates(_file(tmp_path, a + "\n" + b + "\n"), L) == [("candidate_1", a), ("candidate_2", b.upper())]
    for text, message in ((">x\n" + a[:-1] + "\n", r"line 2: sequence of 14 sites, the alignment has 15"),
                          (">x\n" + a[:-1] + "U\n", r"line 2: character 'U' is not one of ACGTN"),
                          (">x\n" + a + "\n>y\n" + a + "\n", r"line 4: repeats the sequence of line 2"),
                          (">x\n>y\n" + a + "\n", r"line 1: FASTA header without a sequence"),
                          ("\n\n", r"no candidate sequences")):
        with pytest.raises(RuntimeError, match=message):
            host.read_named_candidates(_file(tmp_path, text), L)
    with pytest.raises(RuntimeError, match="more than 65536 candidates"):
        host.read_named_candidates(_file(tmp_path, "".join("ACGTACG" + "".join("ACGT"[(k >> (2 * i)) & 3] for i in range(8)) + "\n"
                                                           for k in range(65537))), L)
    with pytest.raises(RuntimeError, match="Can't read candidate file"):
        host.read_named_candidates(str(tmp_path / "missing.fa"), L)


def test_node_names():
    assert host.parse_lineage_node("parent") == 0 and host.parse_lineage_node("mrca") == 1
    for bad in ("root", "MRCA", ""):
        with pytest.raises(RuntimeError, match="--node must be 'parent'"):
            host.parse_lineage_node(bad)


def test_refusals_before_any_device_work(tmp_path):
    h = _phylo()
    good = _file(tmp_path, ">x\nACGTACGTACGTACG\n")
    with pytest.raises(RuntimeError, match="InitializePhyloParameters must be called first"):
        h.ancestral_candidate_posterior("anything", "mrca", ["ACGTACGTACGTACG"])
    with pytest.raises(RuntimeError, match="does not have the alignment's length"):
        h.ancestral_candidate_posterior("anything", 1, ["ACGT"])
    with pytest.raises(RuntimeError, match="node must be 0"):
        h.ancestral_candidate_posterior("anything", 2, ["ACGTACGTACGTACG"])
    out = str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="--node must be 'parent'"):
        h.run_ancestral_probs_pipeline("missing.tsv", "naive", "root", good, out, 4)
    with pytest.raises(RuntimeError, match="Can't read candidate file"):
        h.run_ancestral_probs_pipeline("missing.tsv", "naive", "mrca", str(tmp_path / "none.fa"), out, 4)
    bad = str(tmp_path / "bad.fa")
    open(bad, "w").write(">x\nACGT\n")
    with pytest.raises(RuntimeError, match="line 2: sequence of 4 sites"):
        h.run_ancestral_probs_pipeline("missing.tsv", "naive", "mrca", bad, out, 4)
    with pytest.raises(RuntimeError, match="burn-in fraction must be in"):
        h.run_ancestral_probs_pipeline("missing.tsv", "naive", "mrca", good, out, 4, burnin_frac=1.0)
    with pytest.raises(RuntimeError, match="cannot be 'naive'"):
        h.run_ancestral_probs_pipeline("missing.tsv", "naive", "parent", good, out, 4)
    with pytest.raises(RuntimeError, match="is not a sequence of this clonal family"):
        h.run_ancestral_probs_pipeline("missing.tsv", "no-such-sequence", "parent", good, out, 4)
    assert not os.path.exists(out + ".probs.tsv")


def test_cli_refuses_before_it_evaluates(tmp_path):
    """`linearham --ancestral-probs` with a bad --node or candidate file ends before the tree is read."""
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    common = [exe, "--ancestral-probs", "--yaml-path", os.path.join(D, "phylo_hmm_input.yaml"), "--cluster-ind", "0",
              "--hmm-param-dir", os.path.join(D, "hmm_params"), "--seed-seq", "x", "--newick-path", "missing.tree"]
    good = _file(tmp_path, ">x\nACGTACGTACGTACG\n")
    r = subprocess.run(common + ["--node", "root", "--candidates", good], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--node must be 'parent'" in r.stderr
    r = subprocess.run(common + ["--node", "mrca", "--candidates", str(tmp_path / "none.fa")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "Can't read candidate file" in r.stderr
