"""The oracle of the exact substitution posteriors along a lineage's edges (tests/edge_oracle.py) against brute-force
enumeration, against its margins (the per-node tables of tests/ancestral_marginal_oracle.py and the naive distribution) and
against the ancestral sampler's own pair frequencies.  CPU only."""
import numpy as np
import pytest

from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import edge_oracle as eo
from tests.test_ancestral_marginal_oracle import BRLEN5, CHILDREN5, ER, PI, ROOT5, T5, _columns5, _toy

PATH_LEN5 = {1: 3, 2: 3, 3: 2, 4: 1}


@pytest.fixture(scope="module", params=[(R, tip) for R in (1, 4) for tip in (1, 2, 3, 4)], ids=lambda p: "R%d-tip%d" % p)
def five(request):
    """The 5-tip tree with its N tip (tip 3 in column 3: an N seed tip when tip 3 is the seed) and its all-N column."""
    R, tip = request.param
    msa, q = _columns5()
    rates = orc.gamma_rates_mean(0.6, R)
    path = amo.seed_path(CHILDREN5, ROOT5, T5, tip)
    assert len(path) == PATH_LEN5[tip]
    args = (CHILDREN5, ROOT5, BRLEN5, T5, msa, q, ER, PI, rates, path)
    return dict(R=R, tip=tip, q=q, path=path, got=eo.edges(*args, tip), ref=eo.edges_by_enumeration(*args, tip),
                marg=amo.marginals(*args)[0])


def test_formulas_equal_enumeration(five):
    for k in ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post"):
        assert np.abs(five["got"][k] - five["ref"][k]).max() < 1e-13, k


def test_margins(five):
    edge, ne, marg, q = five["got"]["edge"], five["got"]["naive_edge"], five["marg"], five["q"]
    assert np.abs(edge.sum(axis=-1) - marg).max() < 1e-13                  # sum_c edge[s] = marg[s]
    if len(five["path"]) > 1:
        assert np.abs(edge[1:].sum(axis=-2) - marg[:-1]).max() < 1e-13     # sum_a edge[s] = marg[s-1]
    assert np.abs(ne.sum(axis=-1) - q).max() < 1e-13                       # sum_i naive_edge = q
    assert np.abs(ne.sum(axis=-2) - marg[-1]).max() < 1e-13                # sum_b naive_edge = marg[len-1]


def test_chain_counts_sum_to_the_number_of_edges(five):
    cc = five["got"]["chain_counts"]
    assert np.abs(cc.sum(axis=(-1, -2)) - (len(five["path"]) + 1 - five["q"][:, 4])).max() < 1e-12
    load = five["got"]["edge_load"]
    assert abs(load.sum() - (cc * (1 - np.eye(4))).sum()) < 1e-12


def test_joint_is_not_the_product_of_its_margins(five):
    """What K11's tables cannot give: in some cell of an inner edge (the seed edge where there is none) the joint is
    further than 0.1 from the product of the two ends' marginals."""
    edge = five["got"]["edge"]
    s = 1 if len(five["path"]) > 1 else 0
    prod = edge[s].sum(axis=-1)[:, :, None] * edge[s].sum(axis=-2)[:, None, :]
    assert np.abs(edge[s] - prod).max() >= 0.1


def test_one_hot_equals_the_samplers_pair_frequencies(data_dir):
    """With a one-hot naive_prob the tables are the pair distributions of what asr_sample draws: over 4 000 sample numbers
    of the toy family, the frequencies of (root state), of (root, other inner node) and of (parent, seed tip) lie on the
    tables, every cell within 5 sigma + 1/N."""
    h, children, root, brlen = _toy(data_dir)
    T, L = h.msa.shape[0] + 1, h.msa.shape[1]
    er, pi = [1.0] * 6, np.array([0.17, 0.19, 0.25, 0.39])
    rates = orc.gamma_rates_mean(1.0, 4)
    naive = (np.arange(L) % 5).astype(np.uint8)
    N = 4000
    sites = np.arange(L)
    pair = np.zeros((T - 2, T - 2, L, 4, 4))       # [upper node][lower node]
    for i in range(N):
        _, anc, _ = ao.asr_sample(children, root, brlen, T, h.msa, naive, er, pi, rates, 77, i)
        for v in range(T - 2):
            for w in range(T - 2):
                pair[v, w, sites, anc[v], anc[w]] += 1
    q = np.eye(5)[naive]

    def close(freq, p):
        return (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all()

    lens = set()
    for tip in range(1, T):
        path = amo.seed_path(children, root, T, tip)
        lens.add(len(path))
        got = eo.edges(children, root, brlen, T, h.msa, q, er, pi, rates, path, tip)
        for s in range(1, len(path)):
            assert close(pair[path[s] - T, path[s - 1] - T] / N, got["edge"][s])
        # the naive edge: naive is fixed, so row naive_j holds the root's frequencies (all of the mass)
        root_freq = np.einsum("laa->la", pair[root - T, root - T]) / N
        assert close(root_freq, got["naive_edge"][sites, naive])
        assert np.abs(got["naive_edge"].sum(axis=(1, 2)) - 1).max() < 1e-12
        # the seed edge: an observed tip is fixed too, column msa_j holds its parent's frequencies
        v0 = path[0] - T
        par_freq = np.einsum("laa->la", pair[v0, v0]) / N
        seen = h.msa[tip - 1] < 4
        assert seen.any()
        assert close(par_freq[seen], got["edge"][0][sites[seen], :, h.msa[tip - 1][seen]])
    assert lens == {1, 2}
