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
    with pytest.raises(RuntimeError, match="lh_candidates_layout: null family"):
        lib.candidates_layout(None)
    with pytest.raises(ValueError, match="lh_family_set_candidates"):
        lib.set_candidates(None, np.full((2, 5), 5))
    with pytest.raises(ValueError, match="lh_family_set_candidates"):
        lib.set_candidates(None, np.zeros((2, 5), np.uint8), n_sites=6)
    with pytest.raises(RuntimeError, match="null family"):
        lib.eval_candidates_batch(None, 4, 1, np.zeros((1, 2, 4), np.int32), np.zeros((1, 6)), np.ones((1, 6)),
                                  np.full((1, 4), 0.25), np.ones(1), 4, 2)
    ms = (C.c_double * 2)()
    assert lib.lib.lh_candidates_profile_read(None, ms, None) != 0


@pytest.mark.parametrize("case", CASES)
def test_prior_draws_follow_the_constrained_prior(case):
    """prior_draws (forward filtering / backward sampling of the prior chain): every draw has a finite prior, and the
    20 most frequent of 20 000 seeded draws agree with exp(constrained_log_prior) normalised over the enumerated
    support within 5 sigma."""
    import collections
    h = _family(case)
    h.log_likelihood()
    N = 20000
    d = npo.prior_draws(h, N, np.random.default_rng(20261016))
    assert d.shape == (N, h.msa.shape[1]) and d.dtype == np.uint8
    counts = collections.Counter(map(bytes, d))
    support = npo.by_enumeration(h)
    mass = sum(math.exp(npo.constrained_log_prior(h, s)) for s in support)
    assert abs(mass - math.exp(npo.log_prior_mass(h))) < 1e-12 * mass
    for s in counts:
        assert np.isfinite(npo.constrained_log_prior(h, np.frombuffer(s, np.uint8)))
    assert all(tuple(np.frombuffer(s, np.uint8)) in support for s in counts)
    for s, m in counts.most_common(20):
        p = math.exp(npo.constrained_log_prior(h, np.frombuffer(s, np.uint8))) / mass
        assert abs(m / N - p) < 5 * math.sqrt(p * (1 - p) / N), (m / N, p)


def _ucol_layout(msa, seqs):
    """The documented rule spelled out in lh_family_create's numbering (lh_device.h): patterns without N, then with
    some N, then the all-N pattern; u = base * n_prune + pattern, the all-N pattern's five bases last."""
    msa, seqs = np.asarray(msa), np.asarray(seqs)
    first, key = {}, []
    for i in range(msa.shape[1]):
        key.append(first.setdefault(msa[:, i].tobytes(), i))
    cls = lambda i: 0 if (msa[:, i] != 4).all() else 2 if (msa[:, i] == 4).all() else 1
    order = sorted(first.values(), key=lambda i: (cls(i), i))
    new_id = {i: q for q, i in enumerate(order)}
    npr = len(order) - int((msa[:, order[-1]] == 4).all())
    pat = [new_id[key[i]] for i in range(msa.shape[1])]

    def u(i, b):
        return b * npr + pat[i] if pat[i] < npr else 5 * npr + b
    K, L = seqs.shape
    var = [i for i in range(L) if (seqs[:, i] != seqs[0, i]).any()]
    vu = {u(i, seqs[k, i]) for i in var for k in range(K)}
    au = {u(i, seqs[0, i]) for i in range(L) if i not in var}
    assert max(vu | au) < 5 * npr + 5
    return len(var), len(vu | au), len(vu)


@pytest.mark.parametrize("case", CASES)
def test_candidate_layout_restatement(case):
    """naive_probs_oracle.candidate_layout (what lh_candidates_layout reports) against the u-column numbering spelled
    out, on prior draws of the golden families: one candidate, repeated candidates, and growing sets."""
    h = _family(case)
    h.log_likelihood()
    d = npo.prior_draws(h, 400, np.random.default_rng(3))
    msa = h.msa
    for seqs in (d[:1], d[[0, 0]], d[:2], d[:17], d[:256], d, np.concatenate([d[:5], d[:5]])):
        got = npo.candidate_layout(msa, seqs)
        assert got == _ucol_layout(msa, seqs)
        var, slots, idx = npo.gather_slots(msa, seqs)
        assert got[0] == len(var) and got[2] == len(slots) and (idx.size == 0 or idx.max() == len(slots) - 1)
    assert npo.candidate_layout(msa, d[:1])[::2] == (0, 0)
    assert npo.candidate_layout(msa, np.concatenate([d[:5], d[:5]])) == npo.candidate_layout(msa, d[:5])
    # an alignment with one all-N column and two identical columns: the pairs of identical columns are one u-column
    m = np.array(msa)
    m[:, 1] = m[:, 0]
    m[:, 2] = 4
    s = d[:3].copy()
    s[:, 0] = s[:, 1] = [0, 1, 1]
    s[:, 2] = [2, 3, 4]
    assert npo.candidate_layout(m, s) == _ucol_layout(m, s)
    V, _, nv = npo.candidate_layout(m, s)
    # sites 0 and 1 (one pattern, bases A, C, C) give two pairs, the all-N site 2 three
    assert V >= 3 and nv == len(npo.gather_slots(m, s)[1])
    assert nv == 2 + 3 + npo.candidate_layout(m[:, 3:], s[:, 3:])[2]


def _gpu_tol(ll):
    return 1e-10 + 1e-13 * abs(ll)   # test_gpu_naive_probs._tol


def _sensitivity_families():
    from tools import synth_family as sf
    import tempfile
    for case in CASES:
        yield case, _family(case)
    with tempfile.TemporaryDirectory(prefix="lh_sens_") as tmp:
        sf.generate(sf.Spec.small(n_samples=1), tmp)
        h = orc.PhyloHMM(os.path.join(tmp, "cluster.yaml"), 0, os.path.join(tmp, "hmm_params"), 0)
        r = sf.read_trees_tsv(os.path.join(tmp, "trees.tsv"))[0]
        h.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        h.initialize_phylo_emission()
        yield "small", h


def test_gather_off_by_one_and_swaps_are_visible():
    """The GPU checks of K6b's gather (log_cand - prior + loglik against log_emission_sum, at _tol) would catch an
    off-by-one in the gather or two candidates' columns swapped: on the golden families and Spec.small, every such
    change moves log_emission_sum by more than 100 times the tolerance."""
    for name, h in _sensitivity_families():
        ll = h.log_likelihood()
        d = npo.prior_draws(h, 300, np.random.default_rng(11))
        seqs = np.unique(d, axis=0)
        assert len(seqs) > 10, name
        les = npo.log_emission_sums(h, seqs)
        assert np.all(np.isfinite(les)) and np.allclose(les, [npo.log_emission_sum(h, s) for s in seqs], rtol=1e-14)
        var, slots, idx = npo.gather_slots(h.msa, seqs)
        sl = np.array([math.log(h.xmsa_emission[h.xmsa_ids[(b, i)]]) for i, b in slots])
        base = les - sl[idx].sum(axis=0)
        for shift in (1, -1):
            moved = np.clip(idx + shift, 0, len(sl) - 1)
            diff = np.abs(base + sl[moved].sum(axis=0) - les)
            assert diff.min() > 100 * _gpu_tol(ll), (name, shift, diff.min())
        # two candidates' columns swapped: wherever that changes a value at all, it changes it by far more than the
        # tolerance (pairs whose sums agree to rounding differ only where the emissions are equal, and a swap there is
        # harmless)
        gaps = np.abs(les[:, None] - les[None, :])[~np.eye(len(seqs), dtype=bool)]
        differ = gaps > 1e-12 * abs(ll)
        assert differ.mean() > 0.5, name
        assert gaps[differ].min() > 100 * _gpu_tol(ll), (name, gaps[differ].min())
