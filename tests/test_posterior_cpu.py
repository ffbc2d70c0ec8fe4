"""CPU checks of the posterior entry points: the C ABI exports them, and both refuse a family without sampler tables
or a batch they cannot take before anything reaches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest


def test_posterior_symbols_exported():
    import linearham_amd
    from linearham_amd import capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "linearham_amd.h")).read()
    declared = set(re.findall(r"\b(lh_[a-z_]+)\s*\(", hdr))
    for name in capi.POSTERIOR_EXPORTS:
        assert name in declared, name
        assert name in capi.EXPORTS, name
    lib = linearham_amd.load_library()
    for name in capi.POSTERIOR_EXPORTS:
        assert hasattr(lib.lib, name), name
    assert hasattr(lib, "eval_posterior_batch")


def test_posterior_refuses_null_family():
    import linearham_amd
    lib = linearham_amd.load_library()
    with pytest.raises(RuntimeError, match="null family"):
        lib.eval_posterior_batch(None, 4, 1, np.zeros((1, 2, 4), np.int32), np.zeros((1, 6)), np.ones((1, 6)),
                                 np.full((1, 4), 0.25), np.ones(1), 4)
    ms = C.c_double()
    assert lib.lib.lh_posterior_profile_read(None, C.byref(ms), None) != 0


def test_host_marginal_mapping_on_host_state_space():
    """linearham_amd.posterior reads the host library's state-space dump (no device needed for it): the layout's size is
    the forward size the family declares, and the mapping of the oracle's posteriors through the host's dump equals the
    mapping through the oracle's own state space."""
    from linearham_amd import host
    from linearham_amd import posterior as lp
    from oracle import linearham_oracle as orc
    from tests import posterior_oracle as po
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
    er, pi = [1.0] * 6, [0.17, 0.19, 0.25, 0.39]
    h = host.PhyloHMM(os.path.join(d, "phylo_hmm_input.yaml"), 0, os.path.join(d, "hmm_params"), 0)
    ss = h.dump(1)
    o = orc.PhyloHMM(os.path.join(d, "phylo_hmm_input.yaml"), 0, os.path.join(d, "hmm_params"), 0)
    o.initialize_phylo_parameters(os.path.join(d, "newton.tree"), er, pi, 1.0, 4)
    o.initialize_phylo_emission()
    o.log_likelihood()
    dense = po.smoothing(o)
    compact = po.to_compact(o, dense)
    assert np.array_equal(lp.site_base(ss, compact), po.site_base(o, dense))
    assert lp.gene_posteriors(ss, compact) == po.gene_posteriors(o, dense)
    back = lp.dense_posteriors(ss, compact)
    for region in dense:
        assert np.array_equal(back[region], dense[region]), region
