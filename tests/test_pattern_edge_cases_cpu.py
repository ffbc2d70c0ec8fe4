"""tests/pattern_edge_cases.py without a GPU: the builder's premises for every case of the two GPU modules (exactly L distinct
columns, finite log-likelihood, every pattern read, emissions of distinct patterns more than 1e-7 apart), and the numpy
restatement of the structured algorithm on the descriptor (desc_builder.emulate_prune / emulate_forward) against the dense
oracle on three of the crafted families."""
import numpy as np
import pytest

from oracle import linearham_oracle as orc
from tests import desc_builder as db
from tests import pattern_edge_cases as pe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pattern_edges"))


def test_premises_of_every_case(workdir):
    cases = pe.all_cases()
    assert len(cases) >= 50 and {c.base for c in cases} == set(pe.BASES)
    assert {c.L for c in cases if c.base == "s1100" and not c.mixed} >= set(pe.K1_L) | set(pe.TREEPASS_L)
    hs, gap, low = {}, np.inf, np.inf
    for c in cases:
        h = hs[c.base] = pe.load_case(c, workdir, hs.get(c.base))
        for s in pe.samples(c.base, workdir):
            ll, em = pe.oracle_row(h, s, 4)
            f = pe.check_premises(h, c, ll, em)
            gap, low = min(gap, f["gap"]), min(low, f["min_emission"])
        assert pe.expected_info(h, c)[0] == c.L
    print("%d cases: smallest gap between two patterns' emissions %.3g, smallest emission %.3g" % (len(cases), gap, low))
    assert gap > pe.GAP and low > 1e-300


def test_a_closer_pair_of_emissions_would_be_refused(workdir):
    """check_premises is not vacuous: with two patterns' columns made equal the count is wrong, and with their emissions forced
    together the gap condition fires."""
    c = pe.Case("s256", 255)
    h = pe.load_case(c, workdir)
    ll, em = pe.oracle_row(h, pe.samples("s256", workdir)[0], 4)
    pe.check_premises(h, c, ll, em)
    base, site = pe.column_sites(h)
    pat = h.site_pattern[site]
    a = np.nonzero((base == base[0]) & (pat == pat[0]))[0]
    b = np.nonzero((base == base[0]) & (pat != pat[0]))[0][:1]
    close = em.copy()
    close[b] = em[a[0]] * (1 + 1e-8)
    with pytest.raises(AssertionError, match="too close"):
        pe.check_premises(h, c, ll, close)
    h.msa[:, 1] = h.msa[:, 0]
    with pytest.raises(AssertionError):
        pe.check_premises(h, c, ll, em)


@pytest.mark.parametrize("case,R", [(pe.Case("s1100", 1025), 4), (pe.Case("s256", 255, mixed=True, all_n=True), 3),
                                     (pe.Case("t60", 129), 4)], ids=lambda x: str(x))
def test_structured_restatement_equals_the_dense_oracle(workdir, case, R):
    import linearham_amd
    lib = linearham_amd.load_library()
    h = pe.load_case(case, workdir)
    desc = db.build_family_desc(h)
    T = h.msa.shape[0] + 1
    for s in pe.samples(case.base, workdir):
        ll, em = pe.oracle_row(h, s, R)
        children, root, brlen = db.tree_arrays(orc.parse_newick(s["tree"]), h.xmsa_labels)
        ops, _ = lib.schedule_tree(T, children, root)
        got = db.emulate_prune(desc, T, ops, brlen, s["er"], s["pi"], orc.gamma_rates_mean(s["alpha"], R))
        np.testing.assert_allclose(got, em, rtol=1e-10)
        assert abs(db.emulate_forward(desc, got) - ll) <= 1e-10 * abs(ll)
