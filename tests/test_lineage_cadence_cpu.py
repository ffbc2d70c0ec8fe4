"""tests/lineage_cadence_worker.py without a GPU: the exact reference that tests/test_gpu_lineage_cadence.py holds K15b's
conditional edge tables to tells the arithmetic before the fix of the tree joins from the one after it, and the codon-level
naive distributions are what the module says they are.  Figures: profiles/r26_codon_cadence_cpu.txt (python
tests/lineage_cadence_worker.py --cpu DIR)."""
import os

import numpy as np

from tests import lineage_cadence_worker as lw


def test_one_rescaling_per_node_misses_the_exact_conditional_edge_tables():
    """codon_edge_oracle.cond_edges fed an upward pass with ONE 2^256 rescaling per node (upward_until(until=False)), on
    cmp180's first seed tip (44, inside the block).  compound_zeroed: the live category's vector is 0 after the block's
    joins and H misses the exact cond_edge by 1, a whole table -- beyond the row's bound max(1e-10, 8 d_ref).
    compound_lossy: the last join's product is subnormal and loses bits, yet H, normalised per rate, stays at d_ref from
    the exact tables: that row proves nothing for K15b (the per-rate likelihoods it spoils are
    tests/test_cadence_cases_cpu.py's subject); only finiteness is asserted on it."""
    jobs = max(1, min(2, len(os.sched_getaffinity(0))))
    got = {name: (far, ref) for name, far, ref in lw.one_rescale_rows(jobs)}
    assert set(got) == {"compound_lossy", "compound_zeroed"}
    for name, (far, ref) in got.items():
        print("%s: one rescaling per node %.3g from the exact cond_edge; rescale-until (d_ref) %.3g" % (name, far, ref))
        assert np.isfinite(far) and ref <= 1e-12, (name, far, ref)
    far, ref = got["compound_zeroed"]
    assert far > max(lw.FLOOR, 8.0 * ref), (far, ref)


def test_codon_level_naive_distributions(tmp_path):
    from tests import cadence_cases as cc
    h = cc.load_family("cmp180", tmp_path)
    L = h.msa.shape[1]
    naive = lw.naive_rows(h)
    for frame in (0, 1, 2):
        C = (L - frame) // 3
        for kind in lw.Q_KINDS:
            Q = lw.codon_q_of(kind, h, frame)
            assert Q.shape == (C, 125) and (Q >= 0).all() and np.abs(Q.sum(axis=1) - 1).max() < 1e-15
            assert np.array_equal(Q, lw.codon_q_of(kind, h, frame))
        hot = lw.codon_q_of("one_hot", h, frame).argmax(axis=1)
        assert np.array_equal(np.stack([hot // 25, (hot // 5) % 5, hot % 5], axis=1), naive[frame:frame + 3 * C].reshape(C, 3))
        assert (lw.codon_q_of("all_n", h, frame)[:, 124] == 1).all()
        dq = lw.codon_q_of("dirichlet", h, frame)
        assert ((dq == 0) | (dq >= 1e-3)).all() and (dq == 0).any() and ((dq > 0).sum(axis=1) > 1).any()
    # every deep site takes every position of a codon over the three frames
    for site in cc.deep_sites("cmp180") + cc.deep_sites("cad190"):
        assert {(site - frame) % 3 for frame in (0, 1, 2) if frame <= site < frame + 3 * ((L - frame) // 3)} == {0, 1, 2}, site
