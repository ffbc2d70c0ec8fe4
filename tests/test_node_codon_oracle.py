"""The oracle of a lineage node's codon marginals (tests/node_codon_oracle.py) against the candidate route of K13's oracle,
against path enumeration, against K11's oracle, against the ancestral sampler's draws and against consequences that need no
oracle.  CPU only.

Bounds: identities between two double-precision evaluations of the same quantity 1e-12 (they were measured at 4e-15);
frequencies of N draws within 5 sigma + 1/N of the exact probability."""
import numpy as np
import pytest

from linearham_amd import host
from linearham_amd import posterior as lp
from oracle import asr_oracle as ao
from tests import ancestral_probs_oracle as apo
from tests import codon_oracle as co
from tests import node_codon_oracle as nco
from tests import posterior_oracle as po
from tests.test_ancestral_probs_oracle import _golden, _light

IDENTITY = 1e-12
NODES = (apo.PARENT, apo.MRCA)


@pytest.fixture(params=["phylo_hmm_input", "phylo_hmm_input_extra", "igk"])
def fam(request, data_dir, tmp_path):
    return _light(tmp_path) if request.param == "igk" else _golden(data_dir, request.param, 1)


@pytest.fixture(params=["phylo_hmm_input", "phylo_hmm_input_extra"])
def golden(request, data_dir):
    return _golden(data_dir, request.param, 1)


def test_contraction_equals_the_three_site_candidates(fam):
    """Every codon's table against exp(log_candidates) of its 64 three-site candidates: a forward sweep with modified
    emissions, another route to the same number."""
    path = fam.path(1)
    worst = 0.0
    for node in NODES:
        G = fam.tables(path, node)
        for frame in range(3):
            Q, _ = co.dense(fam.o, frame)
            T = nco.contraction(Q, G, frame)
            for c in range(T.shape[0]):
                ref = np.exp(apo.log_candidates(fam.o, G, nco.triple_candidates(fam.L, frame, c)))
                worst = max(worst, np.abs(T[c] - ref).max())
    print("largest deviation", worst)
    assert worst < IDENTITY


def test_contraction_equals_path_enumeration(golden):
    path = golden.path(1)
    worst = 0.0
    for frame in range(3):
        table, seqs = co.enumerated(golden.o, frame)
        Q, _ = co.dense(golden.o, frame)
        assert np.abs(table - Q).max() < IDENTITY
        for node in NODES:
            G = golden.tables(path, node)
            worst = max(worst, np.abs(nco.contraction(Q, G, frame) - nco.from_sequences(seqs, G, frame)).max())
    print("largest deviation", worst)
    assert worst < IDENTITY


def test_expanded_windows_give_the_same_table(fam):
    """Q from posterior.codon_table(windows, genes), what the device's tables restate, against the dense Q."""
    path = fam.path(1)
    G = fam.tables(path, apo.MRCA)
    for frame in range(3):
        Q, post = co.dense(fam.o, frame)
        Q2 = co.from_compact(fam.o, Q, post, frame)
        assert np.abs(nco.contraction(Q, G, frame) - nco.contraction(Q2, G, frame)).max() < IDENTITY
        assert np.abs(nco.change(Q, G, frame) - nco.change(Q2, G, frame)).max() < IDENTITY


def test_tables_sum_to_one_and_marginals_are_k11s(fam):
    path = fam.path(1)
    marg = fam.k11(path)
    for node in NODES:
        G = fam.tables(path, node)
        slot = apo.slot_of(node, path)
        for frame in range(3):
            Q, _ = co.dense(fam.o, frame)
            T = nco.contraction(Q, G, frame)
            assert np.abs(T.sum(axis=1) - 1).max() < IDENTITY
            m = nco.site_marginals(T).reshape(-1, 4)
            assert np.abs(m - marg[slot, frame:frame + len(m)]).max() < IDENTITY, (node, frame)


def test_table_is_not_the_product_of_its_site_marginals(data_dir):
    """Why K11's tables cannot give a node's codon: at the MRCA of tip 1 on phylo_hmm_input_extra (row 1 of
    ancestral_cases.toy) the exact table is at least 0.03 away from the product of its own site marginals in every frame
    (measured 0.053, 0.071, 0.059)."""
    f = _golden(data_dir, "phylo_hmm_input_extra", 1)
    G = f.tables(f.path(1), apo.MRCA)
    aa = lp.node_codon_amino_acids()
    for frame in range(3):
        Q, _ = co.dense(f.o, frame)
        T = nco.contraction(Q, G, frame)
        prod = nco.product_of_marginals(T)
        gap = np.abs(T - prod).max()
        letters = sorted(set(aa))
        fold = np.array([[int(a == l) for l in letters] for a in aa], dtype=float)
        aa_gap = np.abs(T @ fold - prod @ fold).max()
        print("frame", frame, "codon gap", gap, "amino-acid gap", aa_gap)
        assert gap >= 0.03


def test_change_classes(fam):
    """The fold sums to 1, equals a brute-force double loop over (b, x) with the host's translation, and its last entry
    is Q's mass on the triples that hold an N."""
    path = fam.path(1)
    aa125 = host.translate  # (one call per triple below)
    bases = lp.BASES
    for node in NODES:
        G = fam.tables(path, node)
        for frame in range(3):
            Q, _ = co.dense(fam.o, frame)
            ch = nco.change(Q, G, frame)
            assert np.abs(ch.sum(axis=1) - 1).max() < IDENTITY
            has_n = np.array([4 in (i // 25, (i // 5) % 5, i % 5) for i in range(125)])
            assert np.abs(ch[:, 3] - Q[:, has_n].sum(axis=1)).max() < IDENTITY
            J = nco.joint(Q, G, frame)
            brute = np.zeros_like(ch)
            for i in range(125):
                b = (i // 25, (i // 5) % 5, i % 5)
                for x in range(64):
                    xs = (x // 16, (x // 4) % 4, x % 4)
                    if 4 in b:
                        k = 3
                    elif b == xs:
                        k = 0
                    else:
                        k = 1 if aa125("".join(bases[v] for v in b)) == aa125("".join(bases[v] for v in xs)) else 2
                    brute[:, k] += J[:, i, x]
            assert np.abs(ch - brute).max() < IDENTITY
        if fam.L > 20:
            break  # (the double loop once per family is enough on the 62-site one)


def test_one_hot_naive_codon_is_identical_with_the_diagonal_product(golden):
    path = golden.path(1)
    G = golden.tables(path, apo.PARENT)
    frame, nc = 1, (golden.L - 1) // 3
    rng = np.random.default_rng(3)
    b = rng.integers(0, 4, size=(nc, 3))
    Q = np.zeros((nc, 125))
    Q[np.arange(nc), 25 * b[:, 0] + 5 * b[:, 1] + b[:, 2]] = 1.0
    ch = nco.change(Q, G, frame)
    g1, g2, g3 = nco.codon_G(G, frame, nc)
    want = g1[np.arange(nc), b[:, 0], b[:, 0]] * g2[np.arange(nc), b[:, 1], b[:, 1]] * g3[np.arange(nc), b[:, 2], b[:, 2]]
    assert np.abs(ch[:, 0] - want).max() < 1e-15
    assert (ch[:, 3] == 0).all()


def test_tables_against_draws(data_dir):
    """N = 4 000 draws as tests/test_ancestral_probs_oracle.test_two_site_probabilities_against_draws makes them: triple
    frequencies at the junction codons and class frequencies at every codon, within 5 sigma + 1/N, at both nodes."""
    f = _golden(data_dir, "phylo_hmm_input", 1)
    o, r = f.o, f.row
    path = f.path(1)
    assert len(path) == 2
    N, frame = 4000, 0
    code = {c: i for i, c in enumerate(o.alphabet)}
    naive = np.zeros((N, f.L), dtype=np.int64)
    draws = np.zeros((N, 2, f.L), dtype=np.int64)
    for i in range(N):
        naive[i] = [code[c] for c in o.sample_naive_sequence()]
        _, anc, _ = ao.asr_sample(f.children, f.root, f.brlen, f.T, o.msa, naive[i].astype(np.uint8), r["er"], f.pi, f.rates,
                                  91, i)
        draws[i, 0], draws[i, 1] = anc[path[0] - f.T], anc[path[-1] - f.T]
    Q, _ = co.dense(o, frame)
    nc = Q.shape[0]
    lay = lp.codon_layout(po.state_space(o), frame)
    assert lay["window_codon"]
    cls = lp.change_classes()
    sl = [slice(frame + k, frame + 3 * nc, 3) for k in range(3)]
    b = 25 * naive[:, sl[0]] + 5 * naive[:, sl[1]] + naive[:, sl[2]]
    for node in NODES:
        G = f.tables(path, node)
        T = nco.contraction(Q, G, frame)
        ch = nco.change(Q, G, frame)
        x = 16 * draws[:, node, sl[0]] + 4 * draws[:, node, sl[1]] + draws[:, node, sl[2]]
        for c in lay["window_codon"]:
            freq = np.bincount(x[:, c], minlength=64) / N
            assert (np.abs(freq - T[c]) <= 5 * np.sqrt(T[c] * (1 - T[c]) / N) + 1.0 / N).all(), (node, c)
        k = cls[b, x]
        for c in range(nc):
            freq = np.bincount(k[:, c], minlength=4) / N
            p = np.clip(ch[c], 0, 1)
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (node, c)
