"""The host side of the naive-probability tables, no GPU: translation, repr-style numbers, the writers of .naive.tsv /
.aa.fasta / .dnamap and the candidate-file reader (linearham_amd/csrc/host/NaiveProbs.cpp through the host library)."""
import itertools
import math
import random
import struct

import pytest

from linearham_amd import host

CODE = dict(zip(("".join(c) for c in itertools.product("TCAG", repeat=3)),
                "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"))


def test_translation_table():
    for codon, aa in CODE.items():
        assert host.translate(codon) == aa
    # reading frame 0, truncated to a multiple of 3
    assert host.translate("ATGGC") == "M"
    assert host.translate("AT") == ""
    assert host.translate("ATGTGGTAA") == "MW*"


@pytest.mark.parametrize("codon,aa", [
    ("CTN", "L"), ("GTN", "V"), ("GCN", "A"), ("GGN", "G"), ("CCN", "P"), ("ACN", "T"), ("TCN", "S"), ("CGN", "R"),
    ("TTN", "X"),   # F / L
    ("TAN", "X"),   # Y / stop: mixed stop and sense resolutions give X
    ("TGN", "X"),   # C / stop / W
    ("TNA", "X"),   # L / S / stop
    ("AGN", "X"),   # S / R
    ("NNN", "X"),
    ("TRA", "X"),   # a character outside ACGTN
])
def test_n_codons(codon, aa):
    assert host.translate(codon) == aa


def test_n_codon_rule_is_unanimity():
    for codon in ("".join(c) for c in itertools.product("ACGTN", repeat=3)):
        res = {CODE["".join(r)] for r in itertools.product(*[("TCAG" if ch == "N" else ch) for ch in codon])}
        assert host.translate(codon) == (res.pop() if len(res) == 1 else "X"), codon


def test_repr_double():
    rng = random.Random(7)
    vals = [0.0, 1.0, 0.5, 0.1, 1 / 3, 2 / 3, 1e-4, 1e-5, 1.5e-5, 9.999e-5, 0.00012345, 1e15, 1e16, 123456789012345678.0,
            5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.30000000000000004, 2 ** -20, 2 ** -1074]
    vals += [rng.random() for _ in range(2000)]
    vals += [rng.random() * 10 ** rng.randint(-30, 5) for _ in range(2000)]
    vals += [struct.unpack("<d", struct.pack("<Q", rng.getrandbits(62)))[0] for _ in range(2000)]
    vals += [-v for v in vals[:50]]
    vals += [math.inf, -math.inf]
    for v in vals:
        assert host.repr_double(v) == repr(v), v
        if math.isfinite(v):
            assert float(host.repr_double(v)) == v


def test_writers_group_and_order():
    # three DNA candidates translate to MK (two of them) and MR; one with an N codon translates to X
    seqs = ["ATGAAA", "ATGAGA", "ATGAAG", "ATGNNN"]
    prob = [0.25, 0.375, 0.125, 0.0625]
    log_prior = [-1.0, -2.0, -3.0, -math.inf]
    tsv, aa, dnamap = host.naive_probs_write(seqs, prob, log_prior, count=[3, 1, 2, 0], freq=[0.5, 0.125, 0.375, 0.0])
    rows = host.parse_naive_table(tsv)
    assert [r["seq"] for r in rows] == ["ATGAGA", "ATGAAA", "ATGAAG", "ATGNNN"]
    assert [r["rank"] for r in rows] == [1, 2, 3, 4]
    assert rows[3]["log_prior"] == -math.inf and "\t-inf\t" in tsv
    assert [r["sampled_count"] for r in rows] == [1, 3, 2, 0]
    assert tsv.split("\n")[0] == "rank\tNaiveSequence\tprobability\tlog_prior\tsampled_count\tsampled_frequency"
    assert aa == ">naive_0_0.375\nMK\n>naive_1_0.375\nMR\n>naive_2_0.0625\nMX\n"  # ties: first appearance
    assert dnamap == (">naive_0_0.375\n0.25,ATGAAA\n0.125,ATGAAG\n>naive_1_0.375\n0.375,ATGAGA\n"
                      ">naive_2_0.0625\n0.0625,ATGNNN\n")
    for name, p, _ in host._parse_aa(aa):
        assert float(name.split("_")[2]) == p
    # candidates from a file: NA in the sampled columns
    tsv2, _, _ = host.naive_probs_write(seqs, prob, log_prior)
    assert all(r["sampled_count"] is None and r["sampled_frequency"] is None for r in host.parse_naive_table(tsv2))
    assert tsv2.split("\n")[1].endswith("\tNA\tNA")


def test_writer_numbers_are_exact():
    rng = random.Random(3)
    prob = [rng.random() * 1e-3 for _ in range(20)]
    seqs = ["".join(rng.choice("ACGT") for _ in range(9)) for _ in range(20)]
    tsv, aa, dnamap = host.naive_probs_write(seqs, prob, [-1.0] * 20)
    got = {r["seq"]: r["probability"] for r in host.parse_naive_table(tsv)}
    assert got == dict(zip(seqs, prob))
    for lst in host._parse_dnamap(dnamap).values():
        for p, dna in lst:
            assert p == got[dna]


def test_candidate_file(tmp_path):
    p = tmp_path / "c.txt"
    p.write_text("ACGTN\nacgta\n\n")
    assert host.read_candidates(str(p), 5) == ["ACGTN", "ACGTA"]
    p.write_text(">a\nACG\nTN\n>b\nAAAAA\n")
    assert host.read_candidates(str(p), 5) == ["ACGTN", "AAAAA"]
    p.write_text("ACGTN\nACGT\n")
    with pytest.raises(RuntimeError, match="line 2: sequence of 4 sites, the alignment has 5"):
        host.read_candidates(str(p), 5)
    p.write_text("ACGTN\nACGXN\n")
    with pytest.raises(RuntimeError, match="line 2: character 'X'"):
        host.read_candidates(str(p), 5)
    p.write_text("")
    with pytest.raises(RuntimeError, match="no candidate sequences"):
        host.read_candidates(str(p), 5)
    p.write_text("\n>only a header\n")
    with pytest.raises(RuntimeError, match="line 2: FASTA header without a sequence"):
        host.read_candidates(str(p), 5)
    p.write_text(">a\n>b\nACGTN\n")
    with pytest.raises(RuntimeError, match="line 1: FASTA header without a sequence"):
        host.read_candidates(str(p), 5)
    p.write_text(">a\nACGTN\n\n>b\n")
    with pytest.raises(RuntimeError, match="line 4: FASTA header without a sequence"):
        host.read_candidates(str(p), 5)
    p.write_text("ACGTN\nACGTN\n")
    with pytest.raises(RuntimeError, match="line 2: repeats the sequence of line 1"):
        host.read_candidates(str(p), 5)
