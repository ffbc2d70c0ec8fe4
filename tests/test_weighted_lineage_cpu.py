"""Weighted lineage tables without a GPU: the weighted oracle (tests/weighted_lineage_oracle.py) on a hand-worked
four-tree file, then the host's tabulator with a weights file (Lineage.cpp through host.tabulate_lineage_trees and
`linearham --lineage-trees --weights-path`) against the oracle, and what a weights file can get wrong."""
import math
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import host
from tests import lineage_oracle as lo
from tests import weighted_lineage_oracle as wlo
from tests.test_lineage_cpu import FILES, HAND, SEED_NT, _chain_tree, _oracle_trees

# HAND's three trees and one whose added root and naive's neighbour both read MR
HAND4 = HAND + [_chain_tree("ATGAAA", ["ATGAGA"], SEED_NT)]


def test_oracle_on_four_hand_written_trees():
    """Weights 1, 1/2, 1/4, 1/4 (total 2; every sum below is exact in binary).  Lineage translations naive -> seed:
        tree 1 (1)    MK MK MK MR MK MT    bases ATGAAA ATGAAA ATGAAA ATGAGA ATGAAG ATGACA
        tree 2 (1/2)  MK MK MK MK MT             ATGAAG ATGAAA ATGAAA ATGAAA ATGACA
        tree 3 (1/4)  MT MT MT MR MT             ATGACA ATGACC ATGACC ATGAGA ATGACA
        tree 4 (1/4)  MK MR MR MT                ATGAAA ATGAGA ATGAGA ATGACA
    node_c: MK 1 + 1/2 + 1/4 = 1.75, MR 1 + 1/4 + 1/4 = 1.5, MT 2 -> MT, MK, MR.
    naive translations: MK 1.75 -> naive_0_0.875 (MT, 0.25, is the seed's and keeps the seed's name); MR is
    intermediate_0_0.75.
    node_dt: MK: ATGAAA 1 (tree 1, first run) + 1/2 + 1/4 = 1.75, ATGAAG 1 (tree 1, second run) + 1/2 = 1.5;
             MR: ATGAGA 1 + 1/4 + 1/4 = 1.5; MT: ATGACA 1 + 1/2 + 1/4 + 1/4 (both runs of tree 3) + 1/4 = 2.25, ATGACC 1/4.
    edge_c: MK>MR 1 + 1/4, MR>MK 1, MK>MT 1 + 1/2, MT>MR 1/4, MR>MT 1/4 + 1/4 -> MK>MT 1.5, MK>MR 1.25, MR>MK 1, MR>MT 0.5,
    MT>MR 0.25 (unweighted, MK>MR and MR>MT would tie at 2 behind MK>MT: the weights decide the order here)."""
    lineages = [list(reversed(lo.seqs_of_tree(ln, "seed"))) for ln in HAND4]
    t = wlo.tabulate(lineages, "seed", [1.0, 0.5, 0.25, 0.25])
    n0, i0 = "naive_0_0.875", "intermediate_0_0.75"
    assert t["total"] == 2.0
    assert t["nodes"] == [("seed", "seed", 2.0), (n0, "naive", 1.75), (i0, "intermediate", 1.5)]
    assert t["fasta"] == ">seed\nMT\n>%s\nMK\n>%s\nMR\n" % (n0, i0)
    assert t["dnamap"] == (">seed\n1.125,ATGACA\n0.125,ATGACC\n>%s\n0.875,ATGAAA\n0.75,ATGAAG\n>%s\n0.75,ATGAGA\n" % (n0, i0))
    assert t["edges"] == [(n0, "seed", 1.5, ["K2T"]), (n0, i0, 1.25, ["K2R"]), (i0, n0, 1.0, ["R2K"]),
                          (i0, "seed", 0.5, ["R2T"]), ("seed", i0, 0.25, ["T2R"])]
    # all weights 1: the parent oracle's tables
    u, p = wlo.tabulate(lineages, "seed", [1.0] * 4), lo.tabulate(lineages, "seed")
    assert (u["fasta"], u["dnamap"], u["nodes"], u["edges"]) == (p["fasta"], p["dnamap"], p["nodes"], p["edges"])
    w, ess = wlo.weights_of([math.log(4.0), math.log(2.0), 0.0, float("-inf"), 0.0])
    assert w[3] is None and np.allclose([x for x in w if x is not None], [1.0, 0.5, 0.25, 0.25], rtol=1e-15)
    assert abs(ess - 4.0 / 1.375) < 1e-14


def split_name(name):
    """('naive_0_', 0.875) of 'naive_0_0.875': the fraction inside a name apart from the rest (None: the seed's)."""
    head, _, tail = name.rpartition("_")
    if name.startswith(("naive_", "intermediate_")) and head:
        return head + "_", float(tail)
    return name, None


def close(a, b, rtol):
    return a == b or abs(a - b) <= rtol * abs(b)


def same_name(a, b, rtol):
    (ha, fa), (hb, fb) = split_name(a), split_name(b)
    return ha == hb and ((fa is None and fb is None) or close(fa, fb, rtol))


def compare_weighted(prefix, want, rtol):
    """The files under `prefix` against the weighted oracle's tables: names (the fraction inside parsed out), kinds,
    sequences, mutations and every order exactly; sums and fractions to `rtol`."""
    got = host.read_lineage(prefix)
    total = want["total"]
    assert len(got["fasta"]) == len(want["order"])
    for (name, aa), s in zip(got["fasta"], want["order"]):
        assert aa == s and same_name(name, want["names"][s], rtol), (name, want["names"][s])
    assert len(got["nodes"]) == len(want["nodes"])
    for g, (name, kind, c) in zip(got["nodes"], want["nodes"]):
        assert same_name(g["name"], name, rtol) and g["kind"] == kind, (g, name)
        assert close(g["count"], c, rtol) and close(g["fraction"], c / total, rtol), (g, c)
    for (gname, rows), s in zip(got["dnamap"].items(), want["order"]):
        assert same_name(gname, want["names"][s], rtol)
        ref = wlo.most_common(want["node_dt"][s])
        assert [dna for _, dna in rows] == [dna for dna, _ in ref], gname
        assert all(close(f, c / total, rtol) for (f, _), (_, c) in zip(rows, ref)), gname
    assert len(got["edges"]) == len(want["edges"])
    count_of = {name: c for name, _, c in want["nodes"]}
    for g, (a, b, c, muts) in zip(got["edges"], want["edges"]):
        assert same_name(g["parent"], a, rtol) and same_name(g["child"], b, rtol) and g["mutations"] == muts, (g, a, b)
        assert close(g["count"], c, rtol) and close(g["fraction"], c / total, rtol), (g, c)
        assert close(g["parent_fraction"], c / count_of[a], rtol), (g, c)
    return got


def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _write(tmp_path, name, lines):
    p = str(tmp_path / name)
    open(p, "w").write("\n".join(str(x) for x in lines) + "\n")
    return p


def test_host_tabulator_with_weights_on_hand_written_trees(tmp_path):
    """Fractions to 1e-12: the sums are the same doubles added in the same order; the margin covers exp alone."""
    trees = _write(tmp_path, "hand.trees", HAND4)
    lw = [0.3, -0.4, -1.1, -2.0]
    weights = _write(tmp_path, "hand.lw", ["%.17g" % x for x in lw])
    prefix = str(tmp_path / "hand")
    host.tabulate_lineage_trees(trees, "seed", prefix, weights)
    want, ess, skipped = wlo.tabulate_trees(HAND4, "seed", lw)
    got = compare_weighted(prefix, want, 1e-12)
    assert skipped == 0
    s = got["summary"]
    assert abs(s.pop("kish_ess") - ess) <= 1e-12 * ess
    assert s == dict(rows=4, distinct_nt=5, distinct_aa=3, longest_path=3, hash_collisions_resolved=0, rows_used=4,
                     rows_skipped_nonfinite=0, draws_per_row=1)
    # counts print as floats here, as integers without weights
    assert "." in open(prefix + ".nodes.tsv").read().split("\n")[1].split("\t")[2]
    r = subprocess.run([_exe(), "--lineage-trees", "--input-path", trees, "--output-path", prefix + "_cli", "--seed-seq",
                        "seed", "--weights-path", weights], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for ext in FILES:
        assert open(prefix + "_cli" + ext, "rb").read() == open(prefix + ext, "rb").read(), ext


def test_host_tabulator_with_weights_on_oracle_draws(tmp_path):
    labels, lines = _oracle_trees(tmp_path, 40, n_leaves=8)
    seed_name = labels[-1]
    lw = (1.5 * np.random.default_rng(11).standard_normal(len(lines)) - 300.0).tolist()
    trees = _write(tmp_path, "asr.trees", lines)
    weights = _write(tmp_path, "asr.lw", ["%.17g" % x for x in lw])
    prefix = str(tmp_path / "lin")
    got = host.tabulate_lineage_trees(trees, seed_name, prefix, weights)
    want, ess, _ = wlo.tabulate_trees(lines, seed_name, lw)
    assert 0.15 * len(lines) < ess < 0.85 * len(lines)      # the weights matter and do not degenerate
    assert len(want["order"]) >= 3 and len(want["edges"]) >= 2
    compare_weighted(prefix, want, 1e-12)
    assert abs(got["summary"]["kish_ess"] - ess) <= 1e-12 * ess
    # the weights change the tables: the unweighted fractions are others
    plain = host.tabulate_lineage_trees(trees, seed_name, str(tmp_path / "plain"))
    assert [n["fraction"] for n in plain["nodes"]] != [n["fraction"] for n in got["nodes"]]


def test_equal_log_weights_give_the_unweighted_files(tmp_path):
    trees = _write(tmp_path, "hand.trees", HAND4)
    weights = _write(tmp_path, "hand.lw", ["-1234.5"] * 4)
    a, b = str(tmp_path / "w"), str(tmp_path / "u")
    host.tabulate_lineage_trees(trees, "seed", a, weights)
    host.tabulate_lineage_trees(trees, "seed", b)
    for ext in (".fasta", ".dnamap"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert host.read_lineage(a)["summary"]["kish_ess"] == 4.0


def test_non_finite_weight_lines_are_skipped_and_counted(tmp_path):
    trees = _write(tmp_path, "hand.trees", [HAND4[0], HAND4[3], HAND4[1], HAND4[3], HAND4[2], HAND4[3]])
    weights = _write(tmp_path, "hand.lw", ["0.3", "-inf", "-0.4", "nan", "-1.1", "-2.0"])
    a = str(tmp_path / "w")
    got = host.tabulate_lineage_trees(trees, "seed", a, weights)
    assert got["summary"]["rows_skipped_nonfinite"] == 2 and got["summary"]["rows_used"] == 4
    assert got["summary"]["rows"] == 4
    b = str(tmp_path / "kept")
    host.tabulate_lineage_trees(_write(tmp_path, "kept.trees", HAND4), "seed", b,
                                _write(tmp_path, "kept.lw", ["0.3", "-0.4", "-1.1", "-2.0"]))
    for ext in FILES:
        assert open(a + ext, "rb").read().replace(b"nonfinite\t2", b"nonfinite\t0") == open(b + ext, "rb").read(), ext


def test_weights_file_errors(tmp_path):
    trees = _write(tmp_path, "hand.trees", HAND4)
    prefix = str(tmp_path / "e")
    with pytest.raises(RuntimeError, match="finite"):
        host.tabulate_lineage_trees(trees, "seed", prefix, _write(tmp_path, "a.lw", ["-inf", "nan", "inf", "-inf"]))
    with pytest.raises(RuntimeError, match=r"\b3 lines.*\b4 trees"):
        host.tabulate_lineage_trees(trees, "seed", prefix, _write(tmp_path, "b.lw", ["0", "0", "0"]))
    with pytest.raises(RuntimeError, match=r"\b5 lines.*\b4 trees"):
        host.tabulate_lineage_trees(trees, "seed", prefix, _write(tmp_path, "c.lw", ["0"] * 5))
    with pytest.raises(RuntimeError, match="not a number"):
        host.tabulate_lineage_trees(trees, "seed", prefix, _write(tmp_path, "d.lw", ["0", "zero", "0", "0"]))
    with pytest.raises(RuntimeError, match="open"):
        host.tabulate_lineage_trees(trees, "seed", prefix, str(tmp_path / "missing.lw"))


def test_weighted_pipeline_refuses_bad_arguments_before_it_needs_a_device(tmp_path, data_dir):
    h = host.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    none, x = str(tmp_path / "none.tsv"), str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="naive"):
        h.run_weighted_lineage_pipeline(none, "naive", x, 4)
    with pytest.raises(RuntimeError, match="not_a_tip"):
        h.run_weighted_lineage_pipeline(none, "not_a_tip", x, 4)
    for d in (0, 65):
        with pytest.raises(RuntimeError, match="draws-per-row must be in 1 .. 64"):
            h.run_weighted_lineage_pipeline(none, "not_a_tip", x, 4, draws_per_row=d)
    with pytest.raises(RuntimeError, match="burn-in"):
        h.run_weighted_lineage_pipeline(none, "not_a_tip", x, 4, burnin_frac=1.0)
