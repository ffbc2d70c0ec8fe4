"""CPU checks of the naive-sequence posterior oracle (tests/posterior_oracle.py): alpha-beta, smoothing and brute-force
enumeration agree on the golden families; the marginals are normalised; the log-likelihood identity holds; draws of
the reference-pinned sampler agree with the marginals; the pipeline weighting follows the R script."""
import json
import math
import os

import numpy as np
import pytest

from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc
from tests import posterior_oracle as po

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))


def _family(kind, case, seed=0):
    if kind == "PhyloHMM":
        meta = GOLD["PhyloHMM:" + case]["meta"]
        h = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), seed)
        h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"],
                                      meta["num_rates"])
        h.initialize_phylo_emission()
    else:
        h = orc.SimpleHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), seed)
    ec = po.emission_count(h)
    ll = h.log_likelihood()
    return h, ec, ll


CASES = [("PhyloHMM", "phylo_hmm_input"), ("PhyloHMM", "phylo_hmm_input_extra"), ("SimpleHMM", "simple_hmm_input"),
         ("SimpleHMM", "simple_hmm_input_extra")]


@pytest.mark.parametrize("kind,case", CASES)
def test_three_forms_agree(kind, case):
    h, ec, ll = _family(kind, case)
    fb, lls = po.forward_backward(h, ec)
    sm = po.smoothing(h)
    bf, n_paths = po.brute_force(h)
    assert n_paths > 1
    for k in sm:
        assert np.allclose(fb[k], sm[k], rtol=0, atol=1e-13), k
        assert np.allclose(bf[k], sm[k], rtol=0, atol=1e-13), k
    # sum_k alpha_i(k) beta_i(k) reproduces the log-likelihood on every row
    for v in lls:
        assert abs(v - ll) < 1e-10 * abs(ll), (v, ll)


@pytest.mark.parametrize("kind,case", CASES)
def test_pinned_logliks(kind, case):
    # the reference's pinned values (test/test.cpp, tests/golden/reference_goldens.json): sum_k alpha_i(k) beta_i(k)
    # reproduces them on every row
    h, ec, ll = _family(kind, case)
    want = GOLD[kind + ":" + case]["vars"]["loglikelihood"]
    for v in po.forward_backward(h, ec)[1]:
        assert abs(v - want) < 1e-4, (v, want)


@pytest.mark.parametrize("kind,case", CASES)
def test_marginals_normalised(kind, case):
    h, ec, ll = _family(kind, case)
    dense = po.smoothing(h)
    sb = po.site_base(h, dense)
    assert sb.shape == (h.msa.shape[1], 5)
    assert np.all(sb >= -1e-15)
    assert np.allclose(sb.sum(axis=1), 1.0, atol=1e-13)
    genes = po.gene_posteriors(h, dense)
    assert set(genes) == ({"V", "D", "J"} if h.locus == "igh" else {"V", "J"})
    for reg, d in genes.items():
        assert abs(sum(d.values()) - 1.0) < 1e-13, reg
    for region, p in dense.items():  # every junction row is a distribution
        p = np.atleast_2d(p)
        assert np.allclose(p.sum(axis=1), 1.0, atol=1e-13), region
    # the compact layout round-trips
    ss = po.state_space(h)
    back = lp.dense_posteriors(ss, po.to_compact(h, dense))
    for region in dense:
        assert np.array_equal(back[region], dense[region]), region


@pytest.mark.parametrize("kind,case", [("PhyloHMM", "phylo_hmm_input"), ("SimpleHMM", "simple_hmm_input")])
def test_marginals_match_pinned_sampler(kind, case):
    """20 000 draws of oracle.sample_naive_sequence (the reference's seed-0 path sequence) against the exact
    per-site marginals: every (site, base) within 5 sigma."""
    h, ec, ll = _family(kind, case)
    sb = po.site_base(h, po.smoothing(h))
    n = 20000
    counts = np.zeros_like(sb)
    for _ in range(n):
        s = h.sample_naive_sequence()
        for i, c in enumerate(s):
            counts[i, lp.BASES.index(c)] += 1
    freq = counts / n
    sigma = np.sqrt(np.maximum(sb * (1 - sb), 1.0 / n) / n)
    assert np.all(np.abs(freq - sb) <= 5 * sigma), np.max(np.abs(freq - sb) / sigma)


def test_weighting_semantics():
    """Burn-in drops floor(b N) leading rows; weights are exp(LH - RB) normalised over the kept rows; the batched form
    (linearham_amd.posterior.combine) equals the R script's one-shot normalisation."""
    rng = np.random.default_rng(3)
    N = 37
    lh = rng.normal(-100, 3, N)
    rb = rng.normal(-90, 3, N)
    lh[5] = np.nan  # a non-finite row is dropped
    x = rng.dirichlet(np.ones(6), N)
    for b in (0.0, 0.1, 0.25):
        mean, ess = po.weighted_marginals(lh, rb, x, b)
        first = int(math.floor(b * N))
        # the R script: tail(n = -(b N)), then w = exp(lw - max) / sum
        kept = np.arange(first, N)
        lw = lh[kept] - rb[kept]
        ok = np.isfinite(lw)
        w = np.exp(lw[ok] - np.max(lw[ok]))
        w /= w.sum()
        assert np.allclose(mean, w @ x[kept][ok], rtol=1e-14, atol=0)
        assert abs(ess - 1.0 / np.sum(w * w)) < 1e-9
        # batches combined as the device path does: per-batch (sum w x, [max lw, sum w, sum w^2]) relative to its own max
        parts = []
        for lo in range(first, N, 10):
            sl = np.arange(lo, min(N, lo + 10))
            lwb = lh[sl] - rb[sl]
            okb = np.isfinite(lwb)
            if not okb.any():
                parts.append((np.zeros(6), [-np.inf, 0.0, 0.0]))
                continue
            m = lwb[okb].max()
            wb = np.where(okb, np.exp(np.where(okb, lwb, 0) - m), 0.0)
            parts.append((wb @ np.nan_to_num(x[sl]), [m, wb.sum(), (wb * wb).sum()]))
        got, _, s1, s2 = lp.combine(parts)
        assert np.allclose(got, mean, rtol=1e-13, atol=0)
        assert abs(lp.kish_ess(s1, s2) - ess) < 1e-9 * ess
