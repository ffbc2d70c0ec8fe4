"""K13 and K14 at a slot per row -- lh_eval_ancestral_candidates_at_batch, lh_eval_node_codons_at_batch,
lh_asr_node_codons_at_batch and their _device forms, the third form of K13b (lh_ancestral_probs.hip) -- on the device: the node
is the most recent common ancestor of the seed and another tip, which lies on the seed's path at a slot that differs from
tree sample to tree sample.

Every case runs in a child process (tests/clade_slot_worker.py) under its own time limit, and nothing more is started after a
child that did not end cleanly.  Families: Spec.small(n_samples=5, seed=45) (8 leaves, 62 sites, paths of 3 to 6 nodes) and
the 17-leaf family (n_leaves=17, n_samples=2, seed=9); the tests assert what they claim about the slots they cover.

Bounds, those of the tests of K13 and K14 at the two fixed nodes: 1e-10 (ancestral_cases.BOUND) against the double-precision
oracles; 1e-12 between two device results of the same quantity and for sums to 1; log_cand against the oracle 2.5e-11
(tests/test_gpu_ancestral_probs.py's LOG_CAND_BOUND); weighted sums against numpy over all rows 1e-12 relative, two batches
combined by posterior.combine against the single call 1e-13; device draws within 5 sigma + 1/N of the exact tables.  What
is said to have the same bits is compared bit for bit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "clade_slot_worker.py")
CHILD_TIMEOUT = 240
_stopped = []


def _child(mode, env=None, args=()):
    assert not _stopped, "not started: an earlier child did not end cleanly (%s)" % _stopped[0]
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, WORKER, mode] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        _stopped.append("%s: exit status %d" % (mode, r.returncode))
        raise AssertionError("%s: exit status %d\n%s\n%s" % (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(mode, json.dumps({k: res[k] for k in ("figures", "premises") if k in res}))
    return res


def test_tables_at_interior_slots():
    """cond at the slot against the oracle's tables, against five one-hot lh_asr_marginals_batch calls read at marg[slot]
    and summing to 1, on both families; log_cand against the oracle with the slot's G for one-site candidates at a V, a
    junction and a J site, the 64 candidates of three neighbouring junction sites (they sum to 1), the seed's whole
    sequence, the same half open, and the all-open candidate (exactly 0); one-site candidates against K11's marg at the
    slot; K14's codons against K13's 64 three-site candidates, against the oracle's contraction and, as site marginals,
    against K11; change sums to 1; the given-rates form on the evaluation's own rates and K9 table gives its bits."""
    res = _child("tables")
    p = res["premises"]
    assert p["f8"]["n"] == 5 and all(0 < s < n - 1 for s, n in zip(p["f8"]["slots"], p["f8"]["lengths"]))
    assert p["f17"]["n"] >= 20 and p["f17"]["longest"] >= 6 and len(p["f17"]["slots"]) >= 3 and min(p["f17"]["slots"]) >= 1
    assert res["failures"] == []


@pytest.fixture(scope="module")
def identity():
    return _child("identity")


def test_end_slots_are_the_fixed_nodes_and_rows_stand_alone(identity):
    """slot 0 in every row gives the bits of node 0, the last slot those of node 1, every table and weighted sum of K13 and
    K14; a row gives the same bits alone, in a batch whose rows have unlike slots, and second in a batch of two; weighted
    sums and weight_stats with log_offset against numpy; two batches combined against the single call."""
    p = identity["premises"]
    slots, lens = p["mixed_slots"], p["mixed_lengths"]
    assert len(set(slots)) >= 3 and slots[0] == 0 and slots[1] == lens[1] - 1
    assert any(0 < s < n - 1 for s, n in zip(slots, lens))
    assert len(p["weighted_slots"]) >= 3
    assert identity["failures"] == []


def test_rows_across_launch_group_and_pair_group_cuts(identity):
    """259 rows under LH_CHUNK=256 and LH_ANC_PAIRS=7 (read once per process): two launch groups, groups of pairs that cut
    a row's candidates; rows on either side of each cut carry the bits they have alone in a process without the hooks."""
    res = _child("cut", {"LH_CHUNK": "256", "LH_ANC_PAIRS": "7"})
    assert res["n"] == 259 and res["groups"] == 2 and len(res["distinct_slots"]) >= 3
    assert sorted(res["rows"]) == sorted(identity["alone"])
    assert res["rows"] == identity["alone"]


def test_device_draws_lie_on_the_tables():
    res = _child("draws")
    assert 0 < res["premises"]["slot"] < res["premises"]["length"] - 1
    assert res["failures"] == []


def test_pipelines_at_the_common_ancestor():
    """`linearham --ancestral-probs-pipeline` and `--node-codons-pipeline --node mrca-with:<name>` on the five-row table:
    files byte-identical for LH_PIPELINE_BATCH 2 and 4 and through the library; the tables equal the Python route's rows
    weighted on the host (1e-12), rows.tsv carries every row's slot and summary.tsv node, slot_min and slot_max; with
    partners whose common ancestor with the seed is the root in every row the tables are byte for byte --node mrca's, whose
    own files keep their columns; the single-tree commands give the numbers of the pipeline on a one-row table."""
    res = _child("pipeline")
    p = res["premises"]
    assert len(p["slots"]) == 5 and all(0 < s < n - 1 for s, n in zip(p["slots"], p["lengths"]))
    assert res["failures"] == []


def test_k14_at_an_interior_slot_in_extended_range(tmp_path):
    """lh_eval_node_codons_at_batch on an extended-range handle, a control row and a spread row of tests/ext_deep_cases.py
    (cad190) in one batch at an interior slot: codons and change against node_codon_oracle's contraction of the reference Q
    with the exact cond[slot] (mpmath) within ext_deep_cases.bound(d_ref), d_ref measured on the CPU at that slot between the
    double-precision oracle and the exact tables (tests/clade_slot_ext_cases.py); rows sum to 1; the end slots give the
    fixed nodes' bits in this mode too.  The spread row has no finite log-likelihood in the default mode."""
    from tests import clade_slot_ext_cases as xe
    out = str(tmp_path / "ext")
    meta = xe.build(out, jobs=max(1, min(2, len(os.sched_getaffinity(0)))))
    print("extended range:", json.dumps(meta))
    assert [meta["kinds"][n] for n in meta["rows"]] == ["control", "spread"]
    assert meta["numpy_finite"]["control_b"] and not meta["numpy_finite"]["spread_a10"]
    assert all(0 < s < n - 1 for s, n in zip(meta["slots"], (meta["path_len"][r] for r in meta["rows"])))
    res = _child("ext", args=[out])
    assert res["premises"]["default_finite"] == [True, False]
    assert res["failures"] == []


def test_slots_outside_the_path():
    """-1, the path's length and P: the host forms refuse, naming the row; the device forms give that row NaN and no weight,
    raise the handle's error word with the slot's own message once, and leave the other rows' bits alone."""
    res = _child("badslot")
    assert res["failures"] == []
