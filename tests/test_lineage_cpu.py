"""The lineage tables without a GPU: the oracle (tests/lineage_oracle.py) on a hand-worked file, then the host's
tabulator (Lineage.cpp through host.tabulate_lineage_trees and `linearham --lineage-trees`) against the oracle on that
file and on annotated trees of oracle/asr_oracle.py draws, and the errors that need no device."""
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import host
from tests import lineage_oracle as lo

# codons used below: ATG = M, AAA = AAG = K, AGA = R, ACA = ACC = T
SEED_NT = "ATGACA"


def _chain_tree(naive, inner, seed, seed_name="seed"):
    """An annotated tree as PhyloHMM::RunAsr writes it whose seed lineage is naive, inner[0] (naive's neighbour, and
    the root added above it), inner[1], ..., inner[-1] (the seed's parent), seed; every inner node has one more tip."""
    def c(s):
        return '[&ancestral="%s"]' % s
    sub = "%s%s:0.1" % (seed_name, c(seed))
    for k in range(len(inner) - 1, -1, -1):
        sub = "(x%d%s:0.1,%s)%s:%s" % (k, c("GGGGGG"), sub, c(inner[k]), "0" if k == 0 else "0.1")
    return "(naive%s:0.1,%s)%s;" % (c(naive), sub, c(inner[0]))


HAND = [
    _chain_tree("ATGAAA", ["ATGAAA", "ATGAGA", "ATGAAG"], SEED_NT),
    _chain_tree("ATGAAG", ["ATGAAA", "ATGAAA"], SEED_NT),
    _chain_tree("ATGACA", ["ATGACC", "ATGAGA"], SEED_NT),
]
F23, F13, F43 = repr(2 / 3), repr(1 / 3), repr(4 / 3)


def test_oracle_on_hand_written_trees():
    """Three trees, lineage translations naive -> seed (the root RunAsr adds repeats naive's neighbour):
        tree 1   MK MK MK MR MK MT    bases ATGAAA ATGAAA ATGAAA ATGAGA ATGAAG ATGACA
        tree 2   MK MK MK MK MT             ATGAAG ATGAAA ATGAAA ATGAAA ATGACA
        tree 3   MT MT MT MR MT             ATGACA ATGACC ATGACC ATGAGA ATGACA
    node_c (once per tree): MK 2, MR 2, MT 3 -> most_common MT, MK, MR: MK and MR tie, MK appeared first.
    node_dt (once per run of equal translations):
        MK: tree 1 has two runs, ATGAAA in the first and ATGAAG in the second (MK returns after MR); tree 2 has one run
            with both (a synonymous change inside a run) -> ATGAAA 2, ATGAAG 2, ATGAAA first.
        MT: ATGACA once in trees 1 and 2, and in BOTH runs of tree 3 -> 4 (more than there are trees: the script's
            groupby rule); ATGACC 1.
        MR: ATGAGA 2.
    edge_c without equal ends: MK>MR 1, MR>MK 1, MK>MT 2, MT>MR 1, MR>MT 1 -> MK>MT first, the rest in that order.
    Names: MT is the seed's translation (and tree 3's naive translation: the seed's name wins); naive translations are
    MK, MK, MT -> MK = naive_0_0.666..; MR = intermediate_0_0.666.. ."""
    t = lo.tabulate_trees(HAND, "seed")
    assert t["num_trees"] == 3
    assert t["nodes"] == [("seed", "seed", 3), ("naive_0_" + F23, "naive", 2), ("intermediate_0_" + F23, "intermediate", 2)]
    assert t["fasta"] == ">seed\nMT\n>naive_0_%s\nMK\n>intermediate_0_%s\nMR\n" % (F23, F23)
    assert t["dnamap"] == (">seed\n%s,ATGACA\n%s,ATGACC\n>naive_0_%s\n%s,ATGAAA\n%s,ATGAAG\n>intermediate_0_%s\n%s,ATGAGA\n"
                           % (F43, F13, F23, F23, F23, F23, F23))
    n0, i0 = "naive_0_" + F23, "intermediate_0_" + F23
    assert t["edges"] == [(n0, "seed", 2, ["K2T"]), (n0, i0, 1, ["K2R"]), (i0, n0, 1, ["R2K"]), ("seed", i0, 1, ["T2R"]),
                          (i0, "seed", 1, ["R2T"])]
    # the added root contributes only a pair with equal ends: the lineage without it counts the same
    direct = [["ATGAAA", "ATGAAA", "ATGAGA", "ATGAAG", SEED_NT], ["ATGAAG", "ATGAAA", "ATGAAA", SEED_NT],
              ["ATGACA", "ATGACC", "ATGAGA", SEED_NT]]
    d = lo.tabulate(direct, "seed")
    assert (d["fasta"], d["dnamap"], d["edges"]) == (t["fasta"], t["dnamap"], t["edges"])


def test_oracle_translation_is_its_own():
    assert lo.translate("ATGTGGTAAGC") == "MW*"
    assert [lo.translate(c) for c in ("CTN", "TTN", "TAN", "NNN", "TRA")] == ["L", "X", "X", "X", "X"]


def _compare(prefix, want):
    """The five files under `prefix` against the oracle's tables `want`."""
    assert open(prefix + ".fasta").read() == want["fasta"]
    assert open(prefix + ".dnamap").read() == want["dnamap"]
    got = host.read_lineage(prefix)
    N = want["num_trees"]
    assert [(n["name"], n["kind"], n["count"]) for n in got["nodes"]] == want["nodes"]
    assert [n["fraction"] for n in got["nodes"]] == [c / N for _, _, c in want["nodes"]]
    assert [(e["parent"], e["child"], e["count"], e["mutations"]) for e in got["edges"]] == want["edges"]
    count_of = {name: c for name, _, c in want["nodes"]}
    assert [e["fraction"] for e in got["edges"]] == [c / N for _, _, c, _ in want["edges"]]
    assert [e["parent_fraction"] for e in got["edges"]] == [c / count_of[a] for a, _, c, _ in want["edges"]]
    assert got["summary"]["rows"] == N
    assert got["summary"]["distinct_aa"] == len(want["node_c"])
    return got


def _exe():
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    if not os.path.exists(exe):
        from linearham_amd import build as lb
        lb.build_host(verbose=False)
    return exe


FILES = (".fasta", ".dnamap", ".nodes.tsv", ".edges.tsv", ".summary.tsv")


def _cli_trees(trees, seed_name, prefix):
    return subprocess.run([_exe(), "--lineage-trees", "--input-path", trees, "--output-path", prefix, "--seed-seq",
                           seed_name], capture_output=True, text=True, timeout=300)


def test_host_tabulator_on_hand_written_trees(tmp_path):
    trees = str(tmp_path / "hand.trees")
    open(trees, "w").write("\n".join(HAND) + "\n")
    prefix = str(tmp_path / "hand")
    host.tabulate_lineage_trees(trees, "seed", prefix)
    got = _compare(prefix, lo.tabulate_trees(HAND, "seed"))
    assert got["summary"] == dict(rows=3, distinct_nt=5, distinct_aa=3, longest_path=3, hash_collisions_resolved=0)
    assert open(prefix + ".edges.tsv").read().split("\n")[1].split("\t") == ["naive_0_" + F23, "seed", "2", F23, "1.0", "K2T"]
    r = _cli_trees(trees, "seed", prefix + "_cli")
    assert r.returncode == 0, r.stderr
    for ext in FILES:
        assert open(prefix + "_cli" + ext, "rb").read() == open(prefix + ext, "rb").read(), ext


def _annotated(children, root, brlen, labels, naive_seq, msa, anc, alphabet="ACGTN"):
    """The line PhyloHMM::RunAsr writes (scripts/run_bootstrap_asr_ess.R:86-101), rebuilt from oracle states."""
    T = len(labels)

    def comment(v):
        if v == 0:
            s = naive_seq
        elif v < T:
            s = "".join(alphabet[b] for b in msa[v - 1])
        else:
            s = "".join(alphabet[b] for b in anc[v - T])
        return '[&ancestral="%s"]' % s

    def go(v):
        if v < T:
            return labels[v] + comment(v) + ":%.10g" % brlen[v]
        a, b = children[2 * (v - T)], children[2 * (v - T) + 1]
        return "(" + go(a) + "," + go(b) + ")" + comment(v) + ":%.10g" % (0.0 if v == root else brlen[v])

    return "(" + labels[0] + comment(0) + ":%.10g" % brlen[0] + "," + go(root) + ")" + comment(root) + ";"


def _oracle_trees(tmp_path, n_rows, **kw):
    """Annotated trees as `--pipeline` then `--asr` would write them, made by the oracles alone: per row of a synthetic
    family's tree table the oracle's naive-sequence draw (pipeline seed 3), then asr_oracle's draws (Philox seed 77,
    rates = the 6-digit sr[] columns)."""
    from oracle import asr_oracle as ao
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=n_rows, divergence=0.03, brlen_mean=0.003, **kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    o = orc.PhyloHMM(yaml_path, 0, pdir, 3)
    labels = list(o.xmsa_labels)
    lines = []
    for i, r in enumerate(sf.read_trees_tsv(tsv)):
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        naive_seq = o.sample_naive_sequence()
        children, root, brlen = host.newick_arrays(r["tree"], labels)
        naive = np.array(["ACGTN".index(c) for c in naive_seq])
        sr = [float("%.6g" % x) for x in o.sr]
        _, anc, _ = ao.asr_sample(children, root, brlen, len(labels), o.msa, naive, r["er"], np.asarray(r["pi"]), sr, 77, i)
        lines.append(_annotated(children, root, brlen, labels, naive_seq, o.msa, anc))
    return labels, lines


def something_to_count(want, path_lengths):
    """The conditions a family must meet for the counting rules to be exercised, on the ORACLE's tables."""
    assert sum(1 for _, kind, c in want["nodes"] if kind == "intermediate" and c >= 2) >= 1
    assert max(len(c) for c in want["node_dt"].values()) >= 2
    assert any(c >= 2 for (a, b), c in want["edge_c"].items() if a != b)
    assert len(set(path_lengths)) >= 3


@pytest.mark.parametrize("kw", [dict(n_leaves=8), dict(n_leaves=20, seed=42, ragged=6, ambiguous=0.02)],
                         ids=["plain", "ragged"])
def test_host_tabulator_on_oracle_draws(tmp_path, kw):
    labels, lines = _oracle_trees(tmp_path, 120, **kw)
    seed_name = labels[-1]
    want = lo.tabulate_trees(lines, seed_name)
    lengths = [len(lo.seqs_of_tree(ln, seed_name)) - 3 for ln in lines]  # without seed, naive and the added root
    something_to_count(want, lengths)
    trees = str(tmp_path / "asr.trees")
    open(trees, "w").write("\n".join(lines) + "\n")
    prefix = str(tmp_path / "lin")
    host.tabulate_lineage_trees(trees, seed_name, prefix)
    got = _compare(prefix, want)
    nts = {s for ln in lines for s in lo.seqs_of_tree(ln, seed_name)}
    assert got["summary"]["distinct_nt"] == len(nts)
    assert got["summary"]["longest_path"] == max(lengths)
    r = _cli_trees(trees, seed_name, prefix + "_cli")
    assert r.returncode == 0, r.stderr
    for ext in FILES:
        assert open(prefix + "_cli" + ext, "rb").read() == open(prefix + ext, "rb").read(), ext


def test_errors_without_a_device(tmp_path):
    trees = str(tmp_path / "hand.trees")
    open(trees, "w").write("\n".join(HAND) + "\n")
    prefix = str(tmp_path / "e")
    with pytest.raises(RuntimeError, match="nosuch"):
        host.tabulate_lineage_trees(trees, "nosuch", prefix)   # a tree without the seed
    with pytest.raises(RuntimeError, match="naive"):
        host.tabulate_lineage_trees(trees, "naive", prefix)
    # a tree without the seed further down the file: the line is named
    open(trees, "a").write(_chain_tree("ATGAAA", ["ATGAAA"], SEED_NT, seed_name="other") + "\n")
    with pytest.raises(RuntimeError, match="line 4.*'seed'"):
        host.tabulate_lineage_trees(trees, "seed", prefix)
    # seeds whose translations differ over the trees (the script's assert len(seed_s) == 1)
    two = str(tmp_path / "two.trees")
    open(two, "w").write(HAND[0] + "\n" + _chain_tree("ATGAAA", ["ATGAAA"], "ATGAAA") + "\n")
    with pytest.raises(RuntimeError, match="seed"):
        host.tabulate_lineage_trees(two, "seed", prefix)
    with pytest.raises(RuntimeError, match="open"):
        host.tabulate_lineage_trees(str(tmp_path / "missing"), "seed", prefix)
    r = _cli_trees(trees, "nosuch", prefix)
    assert r.returncode != 0 and "ERROR:" in r.stderr and "nosuch" in r.stderr


def test_pipeline_refuses_a_bad_seed_before_it_needs_a_device(tmp_path, data_dir):
    """RunLineagePipeline checks the seed's name against the family's sequences first: the seed `naive` and a name that
    is no tip of the family are refused with the name in the message (no table is read, no device touched)."""
    h = host.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    with pytest.raises(RuntimeError, match="naive"):
        h.run_lineage_pipeline(str(tmp_path / "none.tsv"), "naive", str(tmp_path / "x"), 1)
    with pytest.raises(RuntimeError, match="not_a_tip"):
        h.run_lineage_pipeline(str(tmp_path / "none.tsv"), "not_a_tip", str(tmp_path / "x"), 1)
