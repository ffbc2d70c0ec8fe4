"""The site-scaling identity behind tests/test_gpu_k2_forms.py, checked on the numpy oracle alone (no GPU).

Multiplying every xMSA column of alignment site t by 2^-k_t changes the log-likelihood by exactly -ln 2 * sum(k): every
path of the V/D/J HMM emits each site once.  tests/k2_scaling_cases.py builds, per family, emission vectors of that form
that reach each rescaling branch of K2; here the oracle (FillGermlinePaddingEmission's equalisation, ScaleMatrix on every
forward row: src/PhyloHMM.cpp:158-193, src/HMM.cpp:1107-1177, src/utils.cpp:135-144) must agree with the identity on
every finite case, overflow exactly on `delta4`, and show the count pattern every case is built for."""
import numpy as np
import pytest

from tests import k2_scaling_cases as kc

# The oracle's log-likelihood is log(sum of the last forward vector) - count * log(2^256): the products behind it are exact
# power-of-two multiples of the unscaled run's, so the two sides differ by the rounding of one log and one subtraction
# (measured 0 to 1.2e-16 relative); 1e-13 leaves room for the cancellation in log(sum) - count * 177.4.
RTOL = 1e-13


@pytest.mark.parametrize("family", list(kc.NEED))
def test_oracle_follows_the_site_scaling_identity(tmp_path, family):
    h = kc.load_family(family, tmp_path)
    site, cases = kc.build_cases(h, kc.SEEDS[family])
    refs = kc.references(h, cases)
    kc.check_conditions(h, cases, refs, need=kc.NEED[family])
    worst = 0.0
    for c in cases:
        ll, want = refs[c.name]["oracle"]["loglik"], refs[c.name]["identity"]
        assert np.isfinite(want), c.name
        if c.expect == "overflow":
            assert not np.isfinite(ll), (c.name, ll)
            continue
        dev = abs(ll - want) / abs(want)
        worst = max(worst, dev)
        assert dev <= RTOL, (c.name, ll, want, dev)
    print("%s: %d cases, largest deviation from the identity %.2e" % (family, len(cases), worst))


def test_batch_order_pairs_base_with_every_deep_case_both_ways(tmp_path):
    h = kc.load_family("small_igh", tmp_path)
    _, cases = kc.build_cases(h, kc.SEEDS["small_igh"])
    order = kc.batch_order(cases)
    assert len(order) >= 17 and len(order) % 2 == 1
    assert set(order) == {c.name for c in cases}
    pairs = [(order[i], order[i + 1]) for i in range(0, len(order) - 1, 2)]
    assert any(a == "base" and b != "base" for a, b in pairs) and any(a != "base" and b == "base" for a, b in pairs)
    assert all((a == "base") != (b == "base") for a, b in pairs)
