"""The exact lineage reference (tests/exact_lineage_oracle.py: mpmath, no rescaling) against the double-precision oracles of
K11, K12 and K13's tables on benign parameters, where those are themselves checked against enumeration
(tests/test_ancestral_marginal_oracle.py, tests/test_edge_oracle.py, tests/test_ancestral_probs_oracle.py).  CPU only.

Bounds: 1e-12 on the 5-tip enumeration tree (two evaluations of a probability, one of them in doubles through LAPACK's
eigen-decomposition); on the toy family the project's bound for these tables (ancestral_cases.BOUND, 1e-10)."""
import numpy as np
import pytest

from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import ancestral_probs_oracle as apo
from tests import edge_oracle as eo
from tests import exact_lineage_oracle as xl
from tests import exact_model_oracle as ex
from tests.ancestral_cases import BOUND
from tests.test_ancestral_marginal_oracle import BRLEN5, CHILDREN5, ER, PI, ROOT5, T5, _columns5, _toy

KEYS = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")


def _compare(children, root, brlen, T, msa, q, er, pi, rates, seed_tips, bound):
    model = ex.ExactModel(er, pi, [float(r) for r in rates])
    lin = xl.ExactLineage(model, T, children, root, brlen, msa)
    pre = amo.prepare(children, root, brlen, T, msa, er, pi, rates)
    worst = 0.0
    for tip in seed_tips:
        path = amo.seed_path(children, root, T, tip)
        tab = lin.tables(path, tip)
        got = xl.mix(tab, q)
        marg, rp = amo.marginals(children, root, brlen, T, msa, q, er, pi, rates, path, pre=pre)
        want = eo.edges(children, root, brlen, T, msa, q, er, pi, rates, path, tip, pre=pre)
        d = [np.abs(got["marg"] - marg).max(), np.abs(got["rate_post"] - rp).max()]
        d += [np.abs(got[k] - want[k]).max() for k in KEYS]
        for node in (apo.PARENT, apo.MRCA):
            G = apo.cond_tables(children, root, brlen, T, msa, er, pi, rates, path, node, pre=pre)
            d.append(np.abs(tab["cond"][apo.slot_of(node, path)] - G).max())
        worst = max(worst, max(d))
        assert max(d) < bound, (tip, d)
        # what needs no oracle: every table is a distribution, and the edge tables' margins are the node tables
        assert np.abs(got["marg"].sum(axis=-1) - 1).max() < 1e-14 and np.abs(got["rate_post"].sum(axis=-1) - 1).max() < 1e-14
        assert np.abs(got["edge"].sum(axis=-1) - got["marg"]).max() < 1e-14
        if len(path) > 1:
            assert np.abs(got["edge"][1:].sum(axis=-2) - got["marg"][:-1]).max() < 1e-14
        assert np.abs(got["naive_edge"].sum(axis=-1) - q).max() < 1e-14
    return worst


@pytest.mark.parametrize("R", [1, 4])
def test_equals_the_double_oracles_on_the_enumeration_tree(R):
    msa, q = _columns5()
    rates = orc.gamma_rates_mean(0.6, R)
    worst = _compare(CHILDREN5, ROOT5, BRLEN5, T5, msa, q, ER, PI, rates, (1, 3, 4), 1e-12)
    print("R = %d: largest difference %.3g" % (R, worst))


def test_equals_the_double_oracles_on_the_toy_family(data_dir):
    h, children, root, brlen = _toy(data_dir)
    T, L = h.msa.shape[0] + 1, h.msa.shape[1]
    q = np.random.default_rng(3).dirichlet(np.ones(5), size=L)
    q[::7] = np.eye(5)[np.arange(len(q[::7])) % 5]
    rates = orc.gamma_rates_mean(0.4, 4)
    worst = _compare(children, root, brlen, T, h.msa, q, [1.3, 0.4, 2.0, 0.7, 1.1, 1.0], np.array([0.3, 0.2, 0.1, 0.4]), rates,
                     range(1, T), BOUND)
    print("toy family: largest difference %.3g" % worst)
