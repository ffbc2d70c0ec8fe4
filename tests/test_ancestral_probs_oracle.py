"""The oracle of the candidate ancestral sequences' probabilities (tests/ancestral_probs_oracle.py) against K11's oracle,
against brute-force enumeration, against the ancestral sampler's draws and against consequences that need no oracle.  CPU
only.

Bounds: identities between two double-precision evaluations of the same quantity 1e-12 (they were measured at 7e-15);
frequencies of N draws within 5 sigma + 1/N of the exact probability."""
import os

import numpy as np
import pytest

from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import ancestral_probs_oracle as apo
from tests import desc_builder as db
from tests import posterior_oracle as po
from tests.ancestral_cases import toy
from tests.test_ancestral_marginal_oracle import BRLEN5, CHILDREN5, ER, PI, ROOT5, T5, _columns5

IDENTITY = 1e-12


class Fam:
    """An oracle family with one tree sample's parameters and emissions set."""

    def __init__(self, o, row, R):
        self.o, self.row, self.R = o, row, R
        self.T, self.L = o.msa.shape[0] + 1, o.msa.shape[1]
        self.children, self.root, self.brlen = db.tree_arrays(orc.parse_newick(row["tree"]), o.xmsa_labels)
        self.pi = np.asarray(row["pi"], dtype=float)
        self.rates = orc.gamma_rates_mean(row["alpha"], R)
        o.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        self.loglik = o.log_likelihood()
        self.pre = amo.prepare(self.children, self.root, self.brlen, self.T, o.msa, row["er"], self.pi, self.rates)

    def path(self, tip):
        return amo.seed_path(self.children, self.root, self.T, tip)

    def tables(self, path, node):
        return apo.cond_tables(self.children, self.root, self.brlen, self.T, self.o.msa, self.row["er"], self.pi, self.rates,
                               path, node, pre=self.pre)

    def k11(self, path):
        q = po.site_base(self.o, po.smoothing(self.o))
        marg, _ = amo.marginals(self.children, self.root, self.brlen, self.T, self.o.msa, q, self.row["er"], self.pi,
                                self.rates, path, pre=self.pre)
        return marg


def _golden(data_dir, case, row):
    o = orc.PhyloHMM(os.path.join(data_dir, case + ".yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    _, rows = toy(data_dir)
    return Fam(o, rows[row], 4)


def _light(tmp_path):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(locus="igk", n_samples=1, seed=5), out)
    o = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    return Fam(o, sf.read_trees_tsv(os.path.join(out, "trees.tsv"))[0], 4)


@pytest.fixture(params=["phylo_hmm_input", "phylo_hmm_input_extra", "igk"])
def fam(request, data_dir, tmp_path):
    return _light(tmp_path) if request.param == "igk" else _golden(data_dir, request.param, 1)


def test_one_site_candidates_are_k11s_marginals(fam):
    """A candidate constrained at one site asks for K11's marginal of that site, at both ends of the path."""
    path = fam.path(1)
    marg = fam.k11(path)
    sites = range(fam.L) if fam.L <= 20 else [0, 1, fam.L // 3, fam.L // 2, fam.L - 2, fam.L - 1]
    for node in (apo.PARENT, apo.MRCA):
        G = fam.tables(path, node)
        for j in sites:
            got = np.exp(apo.log_candidates(fam.o, G, apo.one_site(fam.L, j)))
            assert np.abs(got - marg[apo.slot_of(node, path), j]).max() < IDENTITY, (node, j)


def test_three_site_candidates_sum_to_one_and_open_is_zero(fam):
    path = fam.path(1)
    L = fam.L
    for node in (apo.PARENT, apo.MRCA):
        G = fam.tables(path, node)
        lc = apo.log_candidates(fam.o, G, apo.constrained(L, [0, L // 2, L - 1]))
        assert len(lc) == 64 and abs(np.exp(lc).sum() - 1) < IDENTITY
        assert apo.log_candidates(fam.o, G, np.full((1, L), apo.OPEN))[0] == 0.0


def test_joint_is_not_the_product_of_the_marginals(data_dir):
    """Why K11's tables cannot answer the question: at the MRCA of tip 1 on the toy family (row 1 of ancestral_cases.toy)
    the junction sites 5 and 6 are at least 0.005 away from the product of their marginals."""
    f = _golden(data_dir, "phylo_hmm_input", 1)
    path = f.path(1)
    G = f.tables(path, apo.MRCA)
    one = [np.exp(apo.log_candidates(f.o, G, apo.one_site(f.L, j))) for j in (5, 6)]
    two = np.exp(apo.log_candidates(f.o, G, apo.constrained(f.L, [5, 6]))).reshape(4, 4)
    assert abs(two.sum() - 1) < IDENTITY
    assert np.abs(two.sum(axis=1) - one[0]).max() < IDENTITY and np.abs(two.sum(axis=0) - one[1]).max() < IDENTITY
    assert np.abs(two - np.outer(one[0], one[1])).max() >= 0.005


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("seed_tip", [1, 3, 4])
def test_tables_equal_enumeration(R, seed_tip):
    """G against the enumeration of all inner states on the 5-tip tree, with an N tip and an all-N column."""
    msa, _ = _columns5()
    rates = orc.gamma_rates_mean(0.6, R)
    path = amo.seed_path(CHILDREN5, ROOT5, T5, seed_tip)
    for node in (apo.PARENT, apo.MRCA):
        G = apo.cond_tables(CHILDREN5, ROOT5, BRLEN5, T5, msa, ER, PI, rates, path, node)
        assert np.abs(G.sum(axis=-1) - 1).max() < IDENTITY
        for b in range(5):
            q = np.zeros((msa.shape[1], 5))
            q[:, b] = 1.0
            ref, _ = amo.marginals_by_enumeration(CHILDREN5, ROOT5, BRLEN5, T5, msa, q, ER, PI, rates, path)
            assert np.abs(G[:, b] - ref[apo.slot_of(node, path)]).max() < 1e-13


def test_two_site_probabilities_against_draws(data_dir):
    """What the probabilities are probabilities of: naive sequences drawn from the HMM's posterior, ancestral sequences
    drawn under each by asr_oracle.asr_sample, N = 4 000; the pair frequencies at two sites of the node against the exact
    two-site tables, every cell within 5 sigma + 1/N, at both nodes and for a junction pair and a distant pair."""
    f = _golden(data_dir, "phylo_hmm_input", 1)
    o, r = f.o, f.row
    path = f.path(1)
    assert len(path) == 2
    N = 4000
    draws = np.zeros((N, 2, f.L), dtype=np.int64)
    code = {c: i for i, c in enumerate(o.alphabet)}
    for i in range(N):
        naive = np.array([code[c] for c in o.sample_naive_sequence()], dtype=np.uint8)
        _, anc, _ = ao.asr_sample(f.children, f.root, f.brlen, f.T, o.msa, naive, r["er"], f.pi, f.rates, 91, i)
        draws[i, 0], draws[i, 1] = anc[path[0] - f.T], anc[path[-1] - f.T]
    for node in (apo.PARENT, apo.MRCA):
        G = f.tables(path, node)
        for a, b in ((5, 6), (1, f.L - 2)):
            p = np.exp(apo.log_candidates(o, G, apo.constrained(f.L, [a, b]))).reshape(4, 4)
            freq = np.zeros((4, 4))
            np.add.at(freq, (draws[:, node, a], draws[:, node, b]), 1.0 / N)
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (node, a, b)
