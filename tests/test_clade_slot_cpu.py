"""The host side of K13 and K14 at the common ancestor of the seed and other sequences, no GPU: linearham::CladeSlot
(host.clade_slot, capi.clade_slot) against descendant sets, --node's text, and the refusals that come before any device
work, through the library and through the linearham program."""
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import capi, host
from tests.clade_slot_cases import brute_clade_slot, descendants, random_tree

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def test_clade_slot_against_descendant_sets():
    """200 random binary trees of 5 to 12 tips: every seed with one partner and with random sets of two to four; among them
    the seed's sibling tip (slot 0), a partner across the root (the last slot) and several partners (the largest of their
    slots); the path is seed_path's.  Both routes, host and capi, give the same."""
    rng = np.random.default_rng(20)
    seen = {"sibling": 0, "across_root": 0, "several_max": 0, "interior": 0}
    for _ in range(200):
        T = int(rng.integers(5, 13)) + 1          # tips 1 .. T-1 and naive
        children, root = random_tree(rng, T)
        below = descendants(children, T)
        for seed in range(1, T):
            want_path = host.seed_path(T, children, root, seed)
            single = {}
            for u in range(1, T):
                if u == seed:
                    continue
                path, slot = host.clade_slot(T, children, root, seed, [u])
                bpath, bslot = brute_clade_slot(children, root, T, seed, [u])
                assert path == want_path == bpath and slot == bslot, (children, root, seed, u)
                assert capi.clade_slot(T, children, root, seed, [u]) == (path, slot)
                single[u] = slot
                parent = path[0]
                if u in (int(x) for x in np.asarray(children).reshape(-1, 2)[parent - T]):
                    assert slot == 0
                    seen["sibling"] += 1
                if len(path) > 1 and u not in below[path[-2]]:
                    assert slot == len(path) - 1
                    seen["across_root"] += 1
                seen["interior"] += 0 < slot < len(path) - 1
            k = int(rng.integers(2, 5))
            others = [int(u) for u in rng.permutation([u for u in range(1, T) if u != seed])[:k]]
            path, slot = host.clade_slot(T, children, root, seed, others)
            assert (path, slot) == brute_clade_slot(children, root, T, seed, others)
            assert slot == max(single[u] for u in others)
            seen["several_max"] += len({single[u] for u in others}) > 1
    print(seen)
    assert all(v > 100 for v in seen.values()), seen


def test_clade_slot_refusals():
    rng = np.random.default_rng(3)
    T = 8
    children, root = random_tree(rng, T)
    for tips, message in (([3], "tip 3 is the seed itself"), ([0], "tip 0 is naive"), ([T], "tip 8 is not one of the tips 1 .. 7"),
                          ([-1], "tip -1 is not one of the tips"), ([], "empty list"), ([2, 5, 2], "tip 2 is listed twice")):
        for f in (host.clade_slot, capi.clade_slot):
            with pytest.raises(ValueError, match=message):
                f(T, children, root, 3, tips)
    with pytest.raises(ValueError, match="seed tip 0 is not a tip"):
        host.clade_slot(T, children, root, 0, [2])
    with pytest.raises(ValueError, match="children must hold"):
        host.clade_slot(T, children[:-2], root, 3, [2])


def test_node_text():
    """The two old words keep their values and every string refused before stays refused, with the message's old beginning;
    the new spelling gives its names."""
    assert host.parse_lineage_node("parent") == 0 and host.parse_lineage_node("mrca") == 1
    assert host.parse_lineage_node_text("parent") == (0, []) and host.parse_lineage_node_text("mrca") == (1, [])
    assert host.parse_lineage_node("mrca-with:a") == host.NODE_MRCA_WITH == 2
    assert host.parse_lineage_node_text("mrca-with:a") == (2, ["a"])
    assert host.parse_lineage_node_text("mrca-with:seq 1,b|2,c") == (2, ["seq 1", "b|2", "c"])
    for bad in ("root", "MRCA", "", "mrca-with", "mrca-with:", "mrca-with:a,", "mrca-with:,a", "mrca-with:a,,b", "mrca-with:a,b,a",
                "MRCA-with:a", "mrca_with:a", " mrca"):
        for f in (host.parse_lineage_node, host.parse_lineage_node_text):
            with pytest.raises(RuntimeError, match="--node must be 'parent'") as e:
                f(bad)
            assert "mrca-with:<name>" in str(e.value) and ("'" + bad + "'") in str(e.value)


def _phylo():
    return host.PhyloHMM(os.path.join(D, "phylo_hmm_input.yaml"), 0, os.path.join(D, "hmm_params"), 0)


def _labels():
    from oracle import linearham_oracle as orc
    o = orc.PhyloHMM(os.path.join(D, "phylo_hmm_input.yaml"), 0, os.path.join(D, "hmm_params"), 0)
    return [n for n in o.xmsa_labels if n != "naive"]


def test_refusals_before_any_device_work(tmp_path):
    """An unknown name, the seed itself and 'naive' are refused, by name, before the family is created: the calls below
    run where no device is visible, on a table that does not exist."""
    h = _phylo()
    seed, other = _labels()[:2]
    fasta = str(tmp_path / "c.fa")
    open(fasta, "w").write(">x\nACGTACGTACGTACG\n")
    out = str(tmp_path / "x")
    for node, message in (("mrca-with:no-such-seq", "'no-such-seq' is not a sequence of this clonal family"),
                          ("mrca-with:%s,%s" % (other, seed), "'%s' is the seed sequence itself" % seed),
                          ("mrca-with:naive", "cannot be 'naive'"),
                          ("mrca-with:", "--node must be 'parent'"), ("root", "--node must be 'parent'")):
        with pytest.raises(RuntimeError, match=message):
            h.run_ancestral_probs_pipeline("missing.tsv", seed, node, fasta, out, 4)
        with pytest.raises(RuntimeError, match=message):
            h.run_node_codons_pipeline("missing.tsv", seed, node, out, 4)
    with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
        h.run_node_codons_pipeline("missing.tsv", seed, "mrca-with:" + other, out, 4, frame=3)
    with pytest.raises(RuntimeError, match="Can't read candidate file"):
        h.run_ancestral_probs_pipeline("missing.tsv", seed, "mrca-with:" + other, str(tmp_path / "none.fa"), out, 4)
    with pytest.raises(RuntimeError, match="is not a sequence of this clonal family"):
        h.run_node_codons_pipeline("missing.tsv", "no-such-seed", "mrca-with:" + other, out, 4)
    with pytest.raises(RuntimeError, match="burn-in fraction must be in"):
        h.run_node_codons_pipeline("missing.tsv", seed, "mrca-with:" + other, out, 4, burnin_frac=1.0)
    # the single-tree calls: the node's text first, then the tree
    with pytest.raises(RuntimeError, match="--node must be 'parent'"):
        h.ancestral_candidate_posterior(seed, "mrca-with:", ["ACGTACGTACGTACG"])
    with pytest.raises(RuntimeError, match="--node must be 'parent'"):
        h.node_codon_marginals(seed, "mrca-with:a,a")
    # integers keep their own refusal
    with pytest.raises(RuntimeError, match="node must be 0"):
        h.ancestral_candidate_posterior(seed, 2, ["ACGTACGTACGTACG"])
    with pytest.raises(RuntimeError, match="node must be 0"):
        h.run_node_codons_pipeline("missing.tsv", seed, 2, out, 4)
    assert not os.path.exists(out + ".probs.tsv") and not os.path.exists(out + ".codons.tsv")


def test_cli_refuses_before_it_reads_the_tree(tmp_path):
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    seed, other = _labels()[:2]
    fasta = str(tmp_path / "c.fa")
    open(fasta, "w").write(">x\nACGTACGTACGTACG\n")
    common = ["--yaml-path", os.path.join(D, "phylo_hmm_input.yaml"), "--cluster-ind", "0", "--hmm-param-dir",
              os.path.join(D, "hmm_params"), "--seed-seq", seed]

    def run(sub, node, extra):
        return subprocess.run([exe, sub, "--node", node] + common + extra, capture_output=True, text=True, timeout=120)
    single = ["--newick-path", "missing.tree"]
    table = ["--input-path", "missing.tsv", "--output-path", str(tmp_path / "o")]
    for sub, extra in (("--ancestral-probs", single + ["--candidates", fasta]), ("--node-codons", single),
                       ("--ancestral-probs-pipeline", table + ["--candidates", fasta]), ("--node-codons-pipeline", table)):
        for node in ("mrca-with:", "mrca-with:a,,b", "root"):
            r = run(sub, node, extra)
            assert r.returncode != 0 and "--node must be 'parent'" in r.stderr and "mrca-with:<name>" in r.stderr, (sub, node)
    for sub, extra in (("--ancestral-probs-pipeline", table + ["--candidates", fasta]), ("--node-codons-pipeline", table)):
        r = run(sub, "mrca-with:nobody", extra)
        assert r.returncode != 0 and "'nobody' is not a sequence of this clonal family" in r.stderr
        r = run(sub, "mrca-with:naive", extra)
        assert r.returncode != 0 and "cannot be 'naive'" in r.stderr
        r = run(sub, "mrca-with:" + seed, extra)
        assert r.returncode != 0 and "is the seed sequence itself" in r.stderr
    assert not os.path.exists(str(tmp_path / "o") + ".rows.tsv")
