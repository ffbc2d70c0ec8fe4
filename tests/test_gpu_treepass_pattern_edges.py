"""The tree-pass kernels at their pattern- and site-count edges, against the oracles of their own modules.

tree_upward (under K3b, K11b, K12b), cond_kernel (K13b in its three forms, and through it K14) and K15b loop with a lane per
pattern over NP = n_prune + 1 in four waves -- a second trip starts at NP = 257 --, K11b's and K12b's down passes with a lane
per site.  tests/pattern_edge_cases.TREEPASS holds the crafted families: NP 64, 65, 256, 257, 258, 512, 513 and 1 026, each
without and with an all-N site; 256, 257 and 1 100 sites; one case with N inside patterns; R = 1 once.  Per case two seed tips
with paths of different length on both tree samples: K11 and K12 (full and lean) against ancestral_marginal_oracle /
edge_oracle, K13b's cond at the parent, the MRCA and an interior slot against clade_slot_cases.AtCase.tables_at (1e-10) and
five one-hot K11 calls (1e-12), K13's log_cand for one-site candidates at the first and last site of every block of 64 sites
(2.5e-11; the all-open candidate exactly 0), K14's and K15's given-rates forms in frame 1 against node_codon_oracle /
codon_edge_oracle (1e-10), K3 against oracle/asr_oracle.py on the 256- and 257-pattern cases (drawn strings equal); tables sum
to 1 within 1e-12, padding slots are 0, sites of one pattern carry the same bits, rows are bit-identical alone and in the batch.

Children (tests/treepass_pattern_edges_worker.py) run one at a time under their own time limit; nothing is started after one
that did not end cleanly."""
import json
import os
import subprocess
import sys

import pytest

from tests.pattern_edge_cases import K3_L, TREEPASS, TREEPASS_L
from tests.treepass_pattern_edges_worker import block_edge_sites

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "treepass_pattern_edges_worker.py")
PER_CHILD = 4
CHILD_TIMEOUT = 120        # (four cases of some 2 s each)
_stopped = []
# the figures every case reports (K3's on its own cases)
FIGURES = {"k11_marg", "k11_rate_post", "k11_sum_to_one", "k12_edge", "k12_naive_edge", "k12_chain_counts", "k12_rate_post",
           "k12_edge_load", "k12lean_naive_edge", "k12lean_chain_counts", "k12lean_rate_post", "k12lean_edge_load", "k12_cells",
           "k13_cond_parent", "k13_cond_mrca", "k13_cond_slot", "k13_cond_vs_k11", "k13_cond_sum_to_one", "k13_log_cand",
           "k14_codons_parent", "k14_change_parent", "k14_codons_mrca", "k14_change_mrca", "k14_codons_slot", "k14_change_slot",
           "k14_sum_to_one", "k15b_cond_edge", "k15_codon_counts", "k15_aa_counts", "k15_seed_change", "k15_edge_change",
           "k15_edge_load"}


def test_the_case_list_holds_every_edge():
    plain = [(c, R) for c, R in TREEPASS if c.base == "s1100" and not c.mixed and R == 4]
    assert sorted({c.L + 1 for c, _ in plain}) == [64, 65, 256, 257, 258, 512, 513, 1026]
    assert all({c.all_n for c, _ in plain if c.L == L} == {False, True} for L in TREEPASS_L)
    assert {(c.base, c.all_n) for c, _ in TREEPASS if c.base != "s1100"} == {(b, p) for b in ("s256", "s257") for p in (False, True)}
    assert sum(c.mixed for c, _ in TREEPASS) == 1 and [R for _, R in TREEPASS].count(1) == 1
    assert len(TREEPASS) == 22


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("treepass_edges"))


@pytest.mark.parametrize("first", range(0, len(TREEPASS), PER_CHILD))
def test_tree_pass_kernels_match_their_oracles(workdir, first):
    assert not _stopped, "not started: an earlier child did not end cleanly (%s)" % _stopped[0]
    last = min(first + PER_CHILD, len(TREEPASS))
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, str(first), str(last), workdir]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        _stopped.append("cases %d to %d: exit status %d" % (first, last, r.returncode))
        raise AssertionError("cases %d to %d: exit status %d\n%s\n%s" % (first, last, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x["key"] for x in res["cases"]] == ["%s_R%d" % (c.name, R) for c, R in TREEPASS[first:last]]
    bad = []
    for x, (c, R) in zip(res["cases"], TREEPASS[first:last]):
        print(x["key"], json.dumps(x["premises"]), json.dumps(x["figures"]))
        p = x["premises"]
        want = FIGURES | ({"k3_mismatches"} if c.L in K3_L and not c.mixed and R == 4 else set())
        assert set(x["figures"]) == want, (x["key"], sorted(set(x["figures"]) ^ want))
        assert p["lengths"][0] != p["lengths"][2] and p["n_pat"] == c.L + 1 + int(c.all_n)
        assert p["candidates"] == 1 + 4 * len(block_edge_sites(p["sites"])) and p["sites"] == {"s1100": 1100, "s256": 256, "s257": 257}[c.base]
        bad += ["%s: %s" % (x["key"], f) for f in x["failures"]]
    assert not bad, "\n".join(bad)
