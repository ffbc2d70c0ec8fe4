"""CPU checks of the codon oracle (tests/codon_oracle.py) on the golden phylo families, frames 0, 1 and 2: path
enumeration, the three-position smoothing formula and the compact-layout expansion agree; every codon is normalised; the
table's site marginals are posterior_oracle's; the codon joint is NOT the product of its site marginals (the guard against
a product-of-marginals shortcut); the amino-acid fold equals translating every enumerated path with the host's table."""
import json
import os

import numpy as np
import pytest

from linearham_amd import host
from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc
from tests import codon_oracle as co
from tests import posterior_oracle as po

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
CASES = ["phylo_hmm_input", "phylo_hmm_input_extra"]
_cache = {}


def _family(case):
    if case not in _cache:
        meta = GOLD["PhyloHMM:" + case]["meta"]
        h = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
        h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"],
                                      meta["num_rates"])
        h.initialize_phylo_emission()
        h.log_likelihood()
        _cache[case] = h
    return _cache[case]


def _tables(case, frame):
    key = (case, frame)
    if key not in _cache:
        h = _family(case)
        _cache[key] = (co.enumerated(h, frame), co.dense(h, frame))
    return _cache[key]


@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_three_forms_agree(case, frame):
    h = _family(case)
    (enum, seqs), (dense, post) = _tables(case, frame)
    assert len(seqs) > 1
    assert enum.shape == dense.shape == (co.n_codons(h.msa.shape[1], frame), 125)
    err = np.max(np.abs(enum - dense))
    print("enumerated - dense:", err)
    assert err < 1e-13
    compact = co.from_compact(h, dense, post, frame)
    assert np.max(np.abs(compact - dense)) < 1e-13
    assert np.max(np.abs(dense.sum(axis=1) - 1.0)) < 1e-12
    assert np.max(np.abs(enum.sum(axis=1) - 1.0)) < 1e-12


@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_site_marginals(case, frame):
    h = _family(case)
    _, (dense, post) = _tables(case, frame)
    L = h.msa.shape[1]
    sb = lp.codon_site_base(dense, frame, L)
    want = po.site_base(h, post)
    covered = ~np.isnan(sb[:, 0])
    assert covered.sum() == 3 * dense.shape[0]
    assert np.max(np.abs(sb[covered] - want[covered])) < 1e-13


@pytest.mark.parametrize("case", CASES)
def test_codons_are_not_products_of_site_marginals(case):
    """A condition on the fixture, not a tolerance: in frame 0 some codon entry differs from the product of the codon's own
    site marginals by more than 1e-2 (0.019 and 0.27 on the two families), so a product-of-marginals shortcut fails."""
    _, (dense, _) = _tables(case, 0)
    gap = np.max(np.abs(dense - co.product_of_marginals(dense)))
    print("gap to the product of marginals:", gap)
    assert gap > 1e-2


@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_amino_acid_fold(case, frame):
    (enum, seqs), (dense, _) = _tables(case, frame)
    want = [dict() for _ in range(dense.shape[0])]
    for p, seq in seqs:
        aa = host.translate(seq[frame:])
        assert len(aa) == len(want)
        for c, a in enumerate(aa):
            want[c][a] = want[c].get(a, 0.0) + p
    got = lp.aa_table(dense)
    for c in range(len(want)):
        keys = set(want[c]) | set(got[c])
        assert max(abs(want[c].get(a, 0.0) - got[c].get(a, 0.0)) for a in keys) < 1e-13, c
        assert abs(sum(got[c].values()) - 1.0) < 1e-12


def test_layout_refuses_a_bad_frame():
    h = _family(CASES[0])
    with pytest.raises(ValueError):
        lp.codon_layout(po.state_space(h), 3)


@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("case", CASES)
def test_structured_algorithm(case, frame):
    """K9's structured algorithm in numpy (tests/codon_structured.py: the tables lh_family_set_codons builds from the
    descriptor, lh_codon.hip's tagged steps on the compact forward arrays and the sampler tables) = the dense form."""
    from tests import codon_structured as cs
    from tests import desc_builder as db
    from tests import viterbi_oracle as vo
    h = _family(case)
    _, (dense, post) = _tables(case, frame)
    desc = db.build_family_desc(h)
    tab = cs.tables(desc, frame)
    want_w, want_g, lay = co.window_inputs(h, dense, post, frame)
    assert tab["window_codon"] == lay["window_codon"] and tab["n_codons"] == lay["n_codons"]
    svd, sdj = vo.sampler_tables(h)
    igh = h.locus == "igh"
    fwd = {k: getattr(h, k + "_forward") for k in ["vgerm", "vd_junction", "jgerm"] + (["dgerm", "dj_junction"] if igh else [])}
    F = po.to_compact(h, fwd)
    got_w, got_g = cs.kernel(tab, svd, sdj, len(h.vgerm_forward), len(h.dgerm_forward) if igh else 0, len(h.jgerm_forward), F)
    assert not np.isnan(got_w).any()  # every one of the 125 entries of every window is written
    assert np.max(np.abs(got_w - want_w)) < 1e-13
    assert np.max(np.abs(got_g - want_g)) < 1e-13


@pytest.mark.parametrize("locus,kw", [("igk", {}), ("igh", dict(ragged=4, ambiguous=0.02))])
def test_structured_algorithm_synthetic(tmp_path, locus, kw):
    """The same on synthetic families: a light chain (one junction, J right of it) and ragged reads with ambiguous bases."""
    from tests import codon_structured as cs
    from tests import desc_builder as db
    from tests import viterbi_oracle as vo
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(locus=locus, n_samples=1, **kw), out)
    r = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))[0]
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    h.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
    h.initialize_phylo_emission()
    h.log_likelihood()
    igh = h.locus == "igh"
    desc = db.build_family_desc(h)
    svd, sdj = vo.sampler_tables(h)
    fwd = {k: getattr(h, k + "_forward") for k in ["vgerm", "vd_junction", "jgerm"] + (["dgerm", "dj_junction"] if igh else [])}
    F = po.to_compact(h, fwd)
    for frame in (0, 1, 2):
        dense, post = co.dense(h, frame)
        want_w, want_g, lay = co.window_inputs(h, dense, post, frame)
        tab = cs.tables(desc, frame)
        assert tab["window_codon"] == lay["window_codon"]
        got_w, got_g = cs.kernel(tab, svd, sdj, len(h.vgerm_forward), len(h.dgerm_forward) if igh else 0,
                                 len(h.jgerm_forward), F)
        assert not np.isnan(got_w).any()
        assert np.max(np.abs(got_w - want_w)) < 1e-13 and np.max(np.abs(got_g - want_g)) < 1e-13
        assert np.max(np.abs(co.from_compact(h, dense, post, frame) - dense)) < 1e-13
