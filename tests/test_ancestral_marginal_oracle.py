"""The oracle of the exact ancestral-state marginals (tests/ancestral_marginal_oracle.py) against brute-force enumeration,
against the ancestral sampler's own distribution, and against consequences that need no oracle.  CPU only."""
import os

import numpy as np
import pytest

from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import desc_builder as db

# a 5-tip tree (tip 0 = naive, hanging off the root 7): 5 = (1, 2), 6 = (5, 3), 7 = (6, 4)
T5 = 5
CHILDREN5 = np.array([1, 2, 5, 3, 6, 4], dtype=np.int32)
ROOT5 = 7
BRLEN5 = np.array([0.03, 0.11, 0.02, 0.2, 0.07, 0.05, 0.13, 0.0])
ER = [1.1, 2.3, 0.7, 0.9, 3.1, 1.0]
PI = np.array([0.17, 0.19, 0.25, 0.39])


def _columns5():
    """12 columns over the four sequenced tips: random bases, one column with an N tip, one all-N column."""
    rng = np.random.default_rng(11)
    msa = rng.integers(0, 4, size=(4, 12))
    msa[2, 3] = 4          # an N tip inside a column
    msa[:, 7] = 4          # an all-N column
    q = rng.dirichlet(np.ones(5) * 0.7, size=12)
    q[0] = [0, 0, 1, 0, 0]             # one-hot
    q[1] = [0.5, 0, 0, 0, 0.5]         # mass on N
    q[3] = [0, 0.25, 0, 0.25, 0.5]
    q[7] = [0.1, 0.2, 0.3, 0.15, 0.25]
    return msa, q


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("seed_tip", [1, 3, 4])
def test_formulas_equal_enumeration(R, seed_tip):
    msa, q = _columns5()
    rates = orc.gamma_rates_mean(0.6, R)
    path = amo.seed_path(CHILDREN5, ROOT5, T5, seed_tip)
    assert len(path) == {1: 3, 3: 2, 4: 1}[seed_tip]
    marg, rp = amo.marginals(CHILDREN5, ROOT5, BRLEN5, T5, msa, q, ER, PI, rates, path)
    ref, rp_ref = amo.marginals_by_enumeration(CHILDREN5, ROOT5, BRLEN5, T5, msa, q, ER, PI, rates, path)
    assert np.abs(marg - ref).max() < 1e-13
    assert np.abs(rp - rp_ref).max() < 1e-13
    # the sum rule
    assert np.abs(marg.sum(axis=-1) - 1).max() < 1e-12
    assert np.abs(rp.sum(axis=-1) - 1).max() < 1e-12
    # the all-N column tells the rates nothing
    assert np.abs(rp[7] - 1.0 / R).max() < 1e-15


def _toy(data_dir):
    h = orc.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    tree = open(os.path.join(data_dir, "newton.tree")).read()
    children, root, brlen = db.tree_arrays(orc.parse_newick(tree), h.xmsa_labels)
    return h, children, root, brlen


def test_one_hot_equals_the_samplers_distribution(data_dir):
    """With a one-hot naive_prob the tables are the distributions asr_sample draws from: node frequencies over 4 000 sample
    numbers of the toy family (phylo_hmm_input.yaml + newton.tree), every cell within 5 sigma + 1/N."""
    h, children, root, brlen = _toy(data_dir)
    T, L = h.msa.shape[0] + 1, h.msa.shape[1]
    er, pi = [1.0] * 6, np.array([0.17, 0.19, 0.25, 0.39])
    rates = orc.gamma_rates_mean(1.0, 4)
    naive = (np.arange(L) % 5).astype(np.uint8)
    N = 4000
    counts = np.zeros((T - 2, L, 4))
    rate_counts = np.zeros((L, 4))
    sites = np.arange(L)
    for i in range(N):
        choice, anc, _ = ao.asr_sample(children, root, brlen, T, h.msa, naive, er, pi, rates, 77, i)
        for v in range(T - 2):
            counts[v, sites, anc[v]] += 1
        rate_counts[sites, choice] += 1
    q = np.eye(5)[naive]
    for seed_tip in range(1, T):
        path = amo.seed_path(children, root, T, seed_tip)
        marg, rp = amo.marginals(children, root, brlen, T, h.msa, q, er, pi, rates, path)
        for s, v in enumerate(path):
            p = marg[s]
            assert (np.abs(counts[v - T] / N - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all()
        assert (np.abs(rate_counts / N - rp) <= 5 * np.sqrt(rp * (1 - rp) / N) + 1.0 / N).all()
    assert {len(amo.seed_path(children, root, T, t)) for t in range(1, T)} == {1, 2}


def test_sum_rule_on_the_toy_family(data_dir):
    h, children, root, brlen = _toy(data_dir)
    T, L = h.msa.shape[0] + 1, h.msa.shape[1]
    q = np.random.default_rng(3).dirichlet(np.ones(5), size=L)
    for R in (1, 4, 8):
        for seed_tip in range(1, T):
            path = amo.seed_path(children, root, T, seed_tip)
            marg, rp = amo.marginals(children, root, brlen, T, h.msa, q, [1.0] * 6, PI, orc.gamma_rates_mean(0.3, R), path)
            assert np.abs(marg.sum(axis=-1) - 1).max() < 1e-12
            assert np.abs(rp.sum(axis=-1) - 1).max() < 1e-12


def test_a_tip_at_distance_1e6_fixes_its_parent():
    """No oracle needed: on the 5-tip tree above with tip 1 (the seed) at distance 1e-6 from its parent, node 5, slot 0 puts
    at least 0.99 on the seed's base at every site where the seed has one -- whatever the other tips and the naive
    distribution say (they sit at distances of 0.02 and more)."""
    msa, q = _columns5()
    brlen = BRLEN5.copy()
    brlen[1] = 1e-6
    path = amo.seed_path(CHILDREN5, ROOT5, T5, 1)
    marg, _ = amo.marginals(CHILDREN5, ROOT5, brlen, T5, msa, q, ER, PI, orc.gamma_rates_mean(0.6, 4), path)
    checked = 0
    for j in range(msa.shape[1]):
        if msa[0, j] < 4:
            assert marg[0, j, msa[0, j]] >= 0.99, (j, marg[0, j])
            checked += 1
    assert checked == 11


def test_host_seed_path(data_dir):
    """linearham::SeedPath -- the walk the lineage pipelines and the ancestral-marginals pipeline share, reached through
    host.seed_path and capi.seed_path -- against the oracle's Python walk on three trees: the 5-tip tree above, the toy
    family's tree and a 9-tip ladder.  Host logic: no device."""
    from linearham_amd import capi, host
    _, toy_children, toy_root, _ = _toy(data_dir)
    T9 = 9   # 9 = (1, 2), 10 = (9, 3), ..., 15 = (14, 8): the root, naive's neighbour
    ladder = np.array([1, 2] + sum(([T9 + i, 3 + i] for i in range(6)), []), dtype=np.int32)
    for T, children, root in ((T5, CHILDREN5, ROOT5), (4, toy_children, toy_root), (T9, ladder, 15)):
        for tip in range(1, T):
            want = amo.seed_path(children, root, T, tip)
            assert host.seed_path(T, children, root, tip) == want
            assert capi.seed_path(T, children, root, tip) == want
    assert len(host.seed_path(T9, ladder, 15, 1)) == 7 and host.seed_path(T9, ladder, 15, 8) == [15]
    assert capi.pad_paths([[5, 6, 7], [7]]).tolist() == [[5, 6, 7], [7, -1, -1]]
    with pytest.raises(ValueError):
        host.seed_path(T5, CHILDREN5, ROOT5, 0)
    with pytest.raises(ValueError):          # a tip that hangs below another node than the root
        host.seed_path(T5, CHILDREN5, 6, 4)
