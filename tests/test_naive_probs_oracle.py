"""CPU checks of the factorisation K6 rests on (tests/naive_probs_oracle.py), on the oracle's dense matrices: grouping
every state path by the naive sequence it writes gives P_HMM(s) * prod_i E[s_i, i] / L, the grouped probabilities sum
to one, and their per-site marginals are K5's smoothing marginals.  Plus the C ABI's K6 symbols and their refusals
before anything reaches a device."""
import json
import math
import os
import re

import numpy as np
import pytest

from oracle import linearham_oracle as orc
from tests import naive_probs_oracle as npo
from tests import posterior_oracle as po

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
CASES = ["phylo_hmm_input", "phylo_hmm_input_extra"]


def _family(case):
    meta = GOLD["PhyloHMM:" + case]["meta"]
    h = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"],
                                  meta["num_rates"])
    h.initialize_phylo_emission()
    return h


@pytest.mark.parametrize("case", CASES)
def test_grouped_paths_equal_factorised_form(case):
    h = _family(case)
    ll = h.log_likelihood()
    bf = npo.by_enumeration(h)
    assert len(bf) > 1
    for s, p in bf.items():
        assert abs(math.exp(npo.log_cand(h, s, ll)) - p) < 1e-13, s


@pytest.mark.parametrize("case", CASES)
def test_grouped_probabilities_sum_to_one(case):
    h = _family(case)
    ll = h.log_likelihood()
    bf = npo.by_enumeration(h)
    assert abs(sum(bf.values()) - 1.0) < 1e-13
    assert abs(sum(math.exp(npo.log_cand(h, s, ll)) for s in bf) - 1.0) < 1e-13


@pytest.mark.parametrize("case", CASES)
def test_site_marginals_equal_smoothing(case):
    h = _family(case)
    h.log_likelihood()  # (the forward arrays smoothing reads)
    sb = npo.site_marginals(npo.by_enumeration(h), h.msa.shape[1])
    assert np.max(np.abs(sb - po.site_base(h, po.smoothing(h)))) < 1e-13


def test_impossible_sequence_has_zero_prior():
    h = _family("phylo_hmm_input")
    s = list(next(iter(npo.by_enumeration(h))))
    # a (site, base) pair no state writes
    i, b = next((i, b) for i in range(len(s)) for b in range(5) if (b, i) not in h.xmsa_ids)
    s[i] = b
    assert npo.constrained_log_prior(h, s) == -math.inf


def test_candidate_symbols_exported_and_refusals():
    import ctypes as C
    import linearham_amd
    from linearham_amd import capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "linearham_amd.h")).read()
    declared = set(re.findall(r"\b(lh_[a-z_]+)\s*\(", hdr))
    lib = linearham_amd.load_library()
    for name in capi.CANDIDATE_EXPORTS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib.lib, name), name
    with pytest.raises(RuntimeError, match="null family"):
        lib.set_candidates(None, np.zeros((2, 5), np.uint8))
    assert lib.lib.lh_family_set_candidates(None, 1, None, None) != 0
    assert "lh_family_set_candidates: null family" in lib.error()
    with pytest.raises(RuntimeError, match="lh_candidates_info: null family"):
        lib.candidates_info(None)
    with pytest.raises(ValueError, match="lh_family_set_candidates"):
        lib.set_candidates(None, np.full((2, 5), 5))
    with pytest.raises(ValueError, match="lh_family_set_candidates"):
        lib.set_candidates(None, np.zeros((2, 5), np.uint8), n_sites=6)
    with pytest.raises(RuntimeError, match="null family"):
        lib.eval_candidates_batch(None, 4, 1, np.zeros((1, 2, 4), np.int32), np.zeros((1, 6)), np.ones((1, 6)),
                                  np.full((1, 4), 0.25), np.ones(1), 4, 2)
    ms = (C.c_double * 2)()
    assert lib.lib.lh_candidates_profile_read(None, ms, None) != 0
