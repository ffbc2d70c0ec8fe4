"""The oracle of the amino-acid replacement posteriors along a lineage's edges (tests/codon_edge_oracle.py) against brute
force (enumeration of the inner states per naive basis, contracted with the enumerated state paths), against K13's and
K14's oracles and against consequences that need no oracle.  CPU only.

Bounds: identities between two double-precision evaluations of the same quantity 1e-12."""
import numpy as np
import pytest

from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import ancestral_probs_oracle as apo
from tests import codon_edge_oracle as ceo
from tests import codon_oracle as co
from tests import edge_oracle as eo
from tests import node_codon_oracle as nco
from tests import posterior_oracle as po
from tests.test_ancestral_marginal_oracle import BRLEN5, CHILDREN5, ER, PI, ROOT5, T5, _columns5
from tests.test_ancestral_probs_oracle import _golden, _light

IDENTITY = 1e-12


def _H(f, path, tip, **kw):
    return ceo.cond_edges(f.children, f.root, f.brlen, f.T, f.o.msa, f.row["er"], f.pi, f.rates, path, tip, **kw)


@pytest.fixture(params=["phylo_hmm_input", "phylo_hmm_input_extra"])
def golden(request, data_dir):
    return _golden(data_dir, request.param, 1)


@pytest.fixture(params=["phylo_hmm_input", "phylo_hmm_input_extra", "igk"])
def fam(request, data_dir, tmp_path):
    return _light(tmp_path) if request.param == "igk" else _golden(data_dir, request.param, 1)


def test_joint_equals_brute_force(golden):
    """E_s of every edge, every frame and every seed tip of the golden families' trees: the contraction of the
    message-passing H with the dense Q against the state-enumerated H summed over the enumerated naive paths."""
    f = golden
    assert f.T <= 5
    worst = 0.0
    for frame in range(3):
        table, seqs = co.enumerated(f.o, frame)
        Q, _ = co.dense(f.o, frame)
        assert np.abs(table - Q).max() < IDENTITY
        for tip in range(1, f.T):
            path = f.path(tip)
            H = _H(f, path, tip)
            Hb = _H(f, path, tip, enumerate_states=True)
            for s in range(len(path)):
                worst = max(worst, np.abs(ceo.joint(Q, H[s], frame) - ceo.joint_from_sequences(seqs, Hb[s], frame)).max())
    print("largest deviation", worst)
    assert worst < IDENTITY


@pytest.mark.parametrize("R", [1, 4])
def test_tables_equal_enumeration_on_five_tips(R):
    """H, and the joint under a Dirichlet Q, against the enumeration of all inner states on the 5-tip tree (an N tip, an
    all-N column), every seed tip and frame."""
    msa, _ = _columns5()
    rates = orc.gamma_rates_mean(0.6, R)
    L = msa.shape[1]
    rng = np.random.default_rng(11)
    worst = 0.0
    for tip in range(1, T5):
        path = amo.seed_path(CHILDREN5, ROOT5, T5, tip)
        H = ceo.cond_edges(CHILDREN5, ROOT5, BRLEN5, T5, msa, ER, PI, rates, path, tip)
        Hb = ceo.cond_edges(CHILDREN5, ROOT5, BRLEN5, T5, msa, ER, PI, rates, path, tip, enumerate_states=True)
        worst = max(worst, np.abs(H - Hb).max())
        for frame in range(3):
            nc = (L - frame) // 3
            Q = rng.dirichlet(np.full(125, 0.2), size=nc)
            a, b = ceo.tables(Q, H, frame), ceo.tables(Q, Hb, frame)
            worst = max(worst, max(np.abs(a[k] - b[k]).max() for k in a))
    print("largest deviation", worst)
    assert worst < IDENTITY


def test_sum_rules_and_margins(fam):
    f = fam
    tips = range(1, f.T) if f.L <= 20 else [1]
    for tip in tips:
        path = f.path(tip)
        H = _H(f, path, tip)
        n = len(path)
        # sum_c H = K13's table at the upper end, at both ends of the path
        assert np.abs(H[0].sum(axis=-1) - f.tables(path, apo.PARENT)).max() < IDENTITY
        G = f.tables(path, apo.MRCA)
        assert np.abs(H[-1].sum(axis=-1) - G).max() < IDENTITY
        # sum_a H_s = sum_c H_{s-1}: the lower end of an edge is the upper end of the next
        for s in range(1, n):
            assert np.abs(H[s].sum(axis=-2) - H[s - 1].sum(axis=-1)).max() < IDENTITY
        # sum_b q(b) H_s[b] is K12's edge under the naive distribution q
        q = po.site_base(f.o, po.smoothing(f.o))
        k12 = eo.edges(f.children, f.root, f.brlen, f.T, f.o.msa, q, f.row["er"], f.pi, f.rates, path, tip)
        assert np.abs(np.einsum("jb,sjbac->sjac", q, H) - k12["edge"]).max() < IDENTITY
        for frame in range(3):
            Q, _ = co.dense(f.o, frame)
            t = ceo.tables(Q, H, frame, P=n + 2)
            cc, aa, ec = t["codon_counts"], t["aa_counts"], t["edge_change"]
            assert np.abs(cc.sum(axis=1) - (n + 1)).max() < 1e-11
            assert np.abs(ec[:n].sum(axis=-1) - 1).max() < IDENTITY
            assert (ec[n:n + 2] == 0).all() and (t["edge_load"][n:n + 2] == 0).all()
            assert np.abs(np.trace(aa, axis1=1, axis2=2) - (cc[:, 0] + cc[:, 1])).max() < 1e-11
            assert np.abs(aa.sum(axis=(1, 2)) - cc[:, :3].sum(axis=1)).max() < 1e-11
            # the naive edge is K14's change at the MRCA
            ch = nco.change(Q, G, frame)
            assert np.abs(ec[n + 2] - ch[:, :3]).max() < IDENTITY
            assert np.abs(cc[:, 3] - ch[:, 3]).max() < IDENTITY
            assert np.abs(t["edge_load"] - ec[:, :, 1:].sum(axis=1)).max() == 0
            # the codon at the lower end of the seed edge: a seed without N in the codon has its own triple there
            E0 = ceo.joint(Q, H[0], frame)
            seed = np.asarray(f.o.msa)[tip - 1]
            for c in range(E0.shape[0]):
                tri = seed[frame + 3 * c:frame + 3 * c + 3]
                if (tri < 4).all():
                    y = 16 * tri[0] + 4 * tri[1] + tri[2]
                    assert abs(E0[c][:, y].sum() - 1) < IDENTITY


def test_edge_is_not_the_product_of_k12s_site_edges(data_dir):
    """Why K12's per-site tables cannot give a codon's edge: on phylo_hmm_input_extra (row 1, tip 1) the exact joint of a
    codon at the two ends of an edge differs from the product of K12's three site tables by far more than rounding (the
    identities above hold at 1e-12; anything above 1e-3 is the model, not the arithmetic) in every frame.  Measured:
    0.028, 0.041, 0.027 on the joint's cells and 0.013, 0.020, 0.024 on an edge's replacement class."""
    f = _golden(data_dir, "phylo_hmm_input_extra", 1)
    path = f.path(1)
    H = _H(f, path, 1)
    q = po.site_base(f.o, po.smoothing(f.o))
    k12 = eo.edges(f.children, f.root, f.brlen, f.T, f.o.msa, q, f.row["er"], f.pi, f.rates, path, 1)["edge"]
    cls = lp.edge_classes()
    for frame in range(3):
        Q, _ = co.dense(f.o, frame)
        gap = cgap = 0.0
        for s in range(len(path)):
            E = ceo.joint(Q, H[s], frame)
            e1, e2, e3 = nco.codon_G(k12[s], frame, E.shape[0])
            prod = np.einsum("cxu,cyv,czw->cxyzuvw", e1, e2, e3).reshape(-1, 64, 64)
            gap = max(gap, np.abs(E - prod).max())
            cgap = max(cgap, np.abs(np.where(cls == 2, E - prod, 0.0).sum(axis=(1, 2))).max())
        print("frame", frame, "joint gap", gap, "replacement-class gap", cgap)
        assert gap > 1e-3


def test_symbols_and_classes():
    sym = lp.aa_symbols()
    aa = lp.node_codon_amino_acids()
    assert len(set(sym)) == 21 and all(lp.AA_SYMBOLS[sym[x]] == aa[x] for x in range(64))
    cls = lp.edge_classes()
    for x in range(64):
        for y in range(64):
            assert cls[x, y] == (0 if x == y else 1 if aa[x] == aa[y] else 2)
