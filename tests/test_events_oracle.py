"""CPU checks of the recombination-event oracle (tests/events_oracle.py): path enumeration, the dense difference and
backward-chain form and the numpy restatement of lh_events.hip's structured algorithm agree; every enumerated path reads
left* NTI* right*; every table sums to 1; span's margins are the gene sums of exit and enter; and the frequencies of
20 000 draws of the reference-pinned sampler lie on the tables, which pins the index -> annotation-column mapping to the
sampler's own bookkeeping."""
import json
import math
import os

import numpy as np
import pytest

from oracle import linearham_oracle as orc
from tests import events_oracle as eo

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
CASES = [("PhyloHMM", "phylo_hmm_input"), ("PhyloHMM", "phylo_hmm_input_extra"), ("SimpleHMM", "simple_hmm_input"),
         ("SimpleHMM", "simple_hmm_input_extra")]
_cache = {}


def _family(kind, case):
    if (kind, case) not in _cache:
        if kind == "PhyloHMM":
            meta = GOLD["PhyloHMM:" + case]["meta"]
            h = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
            h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"],
                                          meta["num_rates"])
            h.initialize_phylo_emission()
        else:
            h = orc.SimpleHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
        h.log_likelihood()
        _cache[(kind, case)] = (h, eo.dense(h))
    return _cache[(kind, case)]


def _diff(x, y):
    return max(np.max(np.abs(a - b)) for jx, jy in zip(x, y) for a, b in zip(jx, jy))


def _check_tables(tables):
    for ex, en, sp in tables:
        W = sp.shape[0] - 1
        for t in (ex, en, sp):
            assert abs(t.sum() - 1.0) < 1e-12
        assert np.max(np.abs(sp.sum(axis=1) - ex.sum(axis=0))) < 1e-12  # P(a)
        assert np.max(np.abs(sp.sum(axis=0) - en.sum(axis=0))) < 1e-12  # P(b)
        assert np.all(sp[np.tril_indices(W + 1, -1)] == 0.0)
        assert min(ex.min(), en.min(), sp.min()) > -1e-15


@pytest.mark.parametrize("kind,case", CASES)
def test_three_forms_agree(kind, case):
    h, dn = _family(kind, case)
    en, n_paths = eo.enumerated(h)  # asserts the left* NTI* right* shape of every path
    assert n_paths > 1
    st = eo.structured(h, *eo.sampler_tables(h))
    print("enumerated - dense:", _diff(en, dn), " structured - dense:", _diff(st, dn), " paths:", n_paths)
    assert _diff(en, dn) < 1e-13
    assert _diff(st, dn) < 1e-13
    for t in (en, dn, st):
        _check_tables(t)
    assert len(dn) == (2 if h.locus == "igh" else 1)
    # the flat layout round-trips
    back = eo.unflat(h, eo.flat(dn))
    assert _diff(back, dn) == 0.0


@pytest.mark.parametrize("locus,kw", [("igk", {}), ("igh", dict(ragged=4, ambiguous=0.02))])
def test_dense_and_structured_synthetic(tmp_path, locus, kw):
    """Dense against structured on families too large to enumerate: a light chain (one junction, J right of it) and
    ragged reads with ambiguous bases."""
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(locus=locus, n_samples=1, **kw), out)
    r = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))[0]
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    h.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
    h.initialize_phylo_emission()
    h.log_likelihood()
    dn = eo.dense(h)
    st = eo.structured(h, *eo.sampler_tables(h))
    print("structured - dense:", _diff(st, dn))
    assert _diff(st, dn) < 1e-13
    _check_tables(dn)
    _check_tables(st)
    assert len(dn) == (2 if locus == "igh" else 1)


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_draws_lie_on_the_tables(case):
    """20 000 seed-0 draws of the reference-pinned sampler: the frequency of every (gene, deletion) cell of the four
    junction-side columns and of both insertion lengths lies within 5 sqrt(p (1 - p) / N) + 1 / N of the exact tables."""
    h, dn = _family("PhyloHMM", case)
    cols = eo.columns(h, dn)
    N = 20000
    s = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    meta = GOLD["PhyloHMM:" + case]["meta"]
    s.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    s.initialize_phylo_emission()
    pairs = {"V3pDel": ("vgerm_state_str_samp", "vgerm_right_del_samp"), "D5pDel": ("dgerm_state_str_samp", "dgerm_left_del_samp"),
             "D3pDel": ("dgerm_state_str_samp", "dgerm_right_del_samp"), "J5pDel": ("jgerm_state_str_samp", "jgerm_left_del_samp")}
    ins = {"VDInsertion": "vd_junction_insertion_samp", "DJInsertion": "dj_junction_insertion_samp"}
    assert set(cols) == set(pairs) | set(ins)  # a heavy chain
    counts = {c: {} for c in list(pairs) + list(ins)}
    for _ in range(N):
        s.sample_naive_sequence()
        d = s.sample
        for c, (g, k) in pairs.items():
            key = (d[g], int(d[k]))
            counts[c][key] = counts[c].get(key, 0) + 1
        for c, k in ins.items():
            n = len(d[k])
            counts[c][n] = counts[c].get(n, 0) + 1
    worst = {}
    for c in counts:
        table = cols[c] if c in pairs else {k: p for k, p in enumerate(cols[c])}
        assert abs(sum(table.values()) - 1.0) < 1e-12
        for key in set(table) | set(counts[c]):
            p = table.get(key, 0.0)
            f = counts[c].get(key, 0) / N
            sd = math.sqrt(max(p * (1.0 - p), 0.0) / N)
            assert abs(f - p) <= 5.0 * sd + 1.0 / N, (c, key, f, p)
            if sd > 0:
                worst[c] = max(worst.get(c, 0.0), abs(f - p) / sd)
    print("worst cell in sigma:", worst)
