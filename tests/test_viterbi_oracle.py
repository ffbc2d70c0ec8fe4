"""CPU checks of the Viterbi oracle (tests/viterbi_oracle.py): the dense max-product sweep equals the maximum over all
enumerated state paths on the golden families, value and path; the column-scaling identity of DESIGN section 2 holds in
its max-product form; the helper functions agree with each other."""
import math

import numpy as np
import pytest

from tests import k2_scaling_cases as kc
from tests import viterbi_cases as vc
from tests import viterbi_oracle as vo

LN2 = math.log(2.0)


@pytest.mark.parametrize("case,n_paths", [("phylo_hmm_input", 2750), ("phylo_hmm_input_extra", 1210)])
def test_viterbi_equals_brute_force(case, n_paths):
    o, rows = vc.golden_rows(case)
    ref = vc.oracle_row(o, rows[0])
    paths = vo.enumerate_paths(o, ref["ec"])
    assert len(paths) == n_paths
    w, p, n = vo.brute_force_max(o, ref["ec"])
    assert n == n_paths and p == ref["path"]
    assert abs(w - ref["log_path"]) < 1e-13 * abs(w)
    assert ref["margin"] > 0.0025
    # the margin is what it says at the end of the path: no other path comes closer than that
    others = sorted(x for x, q in paths if q != p)
    assert w - others[-1] >= ref["margin"] - 1e-12
    # the joint of the path, its prior, and the layout conversions
    assert abs(vo.path_log_joint(o, p, ref["ec"]) - w) < 1e-12 * abs(w)
    assert vo.from_states(o, vo.to_states(o, p)) == p
    assert ref["log_path"] < ref["loglik"]
    # all paths together are the likelihood, and their priors are a distribution's worth of mass at most
    assert abs(math.log(sum(math.exp(x - w) for x, _ in paths)) + w - ref["loglik"]) < 1e-10
    priors = [vo.log_path_prior(o, q) for _, q in paths]
    assert all(np.isfinite(priors)) and sum(math.exp(x) for x in priors) <= 1.0 + 1e-12


@pytest.mark.parametrize("name", ["toy", "small_igh", "small_igk"])
def test_column_scaling_identity(name, tmp_path):
    """Multiplying all columns of site t by 2^-k_t leaves the best path unchanged and moves log_path by exactly
    -ln 2 * sum(k): every path emits every site once."""
    h = kc.load_family(name, tmp_path)
    _, cases = kc.build_cases(h, kc.SEEDS[name])
    base = {}
    for c in cases:
        if c.sum_k == 0:
            base[c.name] = vo.viterbi(h, vo.set_emissions(h, c.em))
            assert base[c.name]["margin"] > 4e-4
    checked = 0
    for c in cases:
        if c.sum_k == 0 or c.expect != "finite":
            continue
        v = vo.viterbi(h, vo.set_emissions(h, c.em))
        want = base[c.base]["log_path"] - LN2 * c.sum_k
        assert v["path"] == base[c.base]["path"], c.name
        assert abs(v["log_path"] - want) <= 1e-14 * abs(want), (c.name, v["log_path"], want)
        assert abs(v["margin"] - base[c.base]["margin"]) < 1e-9, c.name
        checked += 1
    assert checked >= 5


def test_sampler_tables_describe_the_dense_transitions():
    """viterbi_oracle.sampler_tables (the tables the device's path priors are computed from) multiply out to the oracle's
    dense transition entries along every enumerated path of a golden family."""
    o, rows = vc.golden_rows("phylo_hmm_input_extra")
    ref = vc.oracle_row(o, rows[0])
    vd, dj = vo.sampler_tables(o)
    assert vd.n_states == o.vd_junction_transition.shape[0] and dj.n_states == o.dj_junction_transition.shape[0]
    T = o.vd_junction_transition
    for l in range(vd.n_left):
        for i in range(1, int(vd.left_rows[l])):
            a = int(vd.left_dense[l]) + i
            assert T[a - 1, a] == vd.left_trans[i, l]
    for r in range(vd.n_right):
        d0 = int(vd.right_dense[r])
        assert np.array_equal(T[d0:d0 + 4, d0:d0 + 4], vd.nti_transition[r])
        for l in range(vd.n_left):
            if vd.left_rows[l] > 0:
                want = (vd.left_lo[0, l] * vd.gene_prob[r]) * vd.nti_landing_in[r]
                assert np.allclose(T[int(vd.left_dense[l]), d0:d0 + 4], want, rtol=1e-15, atol=0)


def _structured_equals_dense(o, rows):
    from tests import desc_builder as db
    desc = db.build_family_desc(o)
    sampler = vo.sampler_tables(o)
    for r in rows:
        ref = vc.oracle_row(o, r)
        assert ref["margin"] > 1e-6
        # the oracle's emissions carry 2^256 rescalings in their germline products only; the per-column vector does not
        states, lp = vo.emulate_viterbi(desc, sampler, o.xmsa_emission)
        assert np.array_equal(states, ref["states"]), (states, ref["states"])
        assert abs(lp - ref["log_path"]) < 1e-10 * (1.0 + abs(lp))


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_structured_sweep_equals_dense_golden(case):
    """K8's algorithm (cross-gene maximum with one arg-max per row, predecessor codes, trace-back through the sampler
    tables: viterbi_oracle.emulate_viterbi) gives the dense sweep's path and value."""
    _structured_equals_dense(*vc.golden_rows(case))


@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_structured_sweep_equals_dense_synthetic(tmp_path, locus):
    o, rows, _ = vc.synthetic_rows(tmp_path, 2, locus=locus)
    _structured_equals_dense(o, rows)
