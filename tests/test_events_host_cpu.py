"""The host side of the recombination-event tables, no GPU: PhyloHMM::MapEvents (table indices -> the units of the
annotation columns, through the members the sampler reads) and the three writers, on hand-made tables and on the oracle's
exact tables of the golden families."""
import json
import os

import numpy as np
import pytest

from linearham_amd import host
from oracle import linearham_oracle as orc
from tests import events_oracle as eo
from tests import posterior_oracle as po

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
CASES = ["phylo_hmm_input", "phylo_hmm_input_extra"]


def _pair(case):
    h = host.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    o = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    return h, o


def _dims(o):
    return [(i["n_rows"], nL, nR) for _, _, _, i, nL, nR in eo._info(o)]


@pytest.mark.parametrize("case", CASES)
def test_sizes_are_the_layouts(case):
    h, o = _pair(case)
    size, ng = h.events_sizes()
    assert size == sum((nL + nR + W + 1) * (W + 1) for W, nL, nR in _dims(o))
    assert ng == len(o.vgerm.state_strs) + len(o.dgerm.state_strs) + len(o.jgerm.state_strs)
    with pytest.raises(ValueError):
        h.map_events(np.zeros(size + 1), np.zeros(ng))
    with pytest.raises(ValueError):
        h.map_events(np.zeros(size), np.zeros(ng - 1))


@pytest.mark.parametrize("case", CASES)
def test_every_cell_maps_to_the_samplers_units(case):
    """One unit of weight on a single cell of a single table: the C++ mapping names the column, gene and length that
    events_oracle.columns reads off the oracle's members (the ones sample_junction_states / sample_germline_state read).
    Cells of states that do not exist are refused."""
    h, o = _pair(case)
    dims = _dims(o)
    size, ng = h.events_sizes()
    genes = np.zeros(ng)
    cols = [("V3pDel", "D5pDel", "VD"), ("D3pDel", "J5pDel", "DJ")]
    n_cells = n_refused = 0
    for j, (W, nL, nR) in enumerate(dims):
        for t, n_g in ((0, nL), (1, nR)):
            for g in range(n_g):
                for k in range(W + 1):
                    tables = [tuple(np.zeros(s) for s in ((a, w + 1), (b, w + 1), (w + 1, w + 1))) for w, a, b in dims]
                    tables[j][t][g, k] = 1.0
                    try:
                        want = eo.columns(o, tables)[cols[j][t]]
                    except ValueError:
                        want = None  # the oracle has no such state
                    try:
                        got = h.map_events(eo.flat(tables), genes)
                    except RuntimeError as e:
                        assert "has no state on" in str(e) and want is None
                        n_refused += 1
                        continue
                    assert want is not None
                    (gene, length), = [key for key, p in want.items() if p == 1.0]
                    assert got["deletions"] == {(cols[j][t], gene, length): 1.0, (cols[j][t], "*", length): 1.0}
                    assert got["insertions"] == {} and got["spans"] == {}
                    n_cells += 1
    assert n_cells > 8 and n_refused > 0
    # a span cell: its diagonal is the insertion length
    for j, (W, nL, nR) in enumerate(dims):
        for a in range(W + 1):
            for b in range(a, W + 1):
                tables = [tuple(np.zeros(s) for s in ((x, w + 1), (y, w + 1), (w + 1, w + 1))) for w, x, y in dims]
                tables[j][2][a, b] = 0.25
                got = h.map_events(eo.flat(tables), genes)
                assert got["spans"] == {(cols[j][2], a, b): 0.25}
                assert got["insertions"] == {(cols[j][2] + "Insertion", b - a): 0.25}
                assert got["deletions"] == {}
    # the outer ends are folded from the gene posteriors
    nV, nJ = len(o.vgerm.state_strs), len(o.jgerm.state_strs)
    for g in range(nV):
        genes = np.zeros(ng)
        genes[g] = 0.5
        got = h.map_events(np.zeros(size), genes)
        k = o.vgerm.left_del[g]
        assert got["deletions"] == {("V5pDel", o.vgerm.state_strs[g], k): 0.5, ("V5pDel", "*", k): 0.5}
    for g in range(nJ):
        genes = np.zeros(ng)
        genes[ng - nJ + g] = 0.5
        got = h.map_events(np.zeros(size), genes)
        k = o.jgerm.right_del[g]
        assert got["deletions"] == {("J3pDel", o.jgerm.state_strs[g], k): 0.5, ("J3pDel", "*", k): 0.5}


@pytest.mark.parametrize("case", CASES)
def test_oracle_tables_through_the_mapping(case):
    """The oracle's exact tables of the golden tree through the C++ mapping = through events_oracle.columns; every
    column's gene-summed rows and every junction's insertion lengths and spans sum to 1; numbers round-trip (%.17g)."""
    h, o = _pair(case)
    meta = GOLD["PhyloHMM:" + case]["meta"]
    o.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    o.initialize_phylo_emission()
    o.log_likelihood()
    post = po.smoothing(o)
    tables = eo.dense(o, post)
    genes = np.concatenate([post[k] for k in ("vgerm", "dgerm", "jgerm")])
    got = h.map_events(eo.flat(tables), genes)
    want = eo.columns(o, tables)
    for c in ("V3pDel", "D5pDel", "D3pDel", "J5pDel"):
        mine = {(g, k): p for (cc, g, k), p in got["deletions"].items() if cc == c and g != "*"}
        keys = {key for key, p in want[c].items() if p > 0}
        assert set(mine) == keys
        assert all(mine[key] == want[c][key] or abs(mine[key] - want[c][key]) < 1e-15 for key in keys)
    for c in ("V5pDel", "V3pDel", "D5pDel", "D3pDel", "J5pDel", "J3pDel"):
        assert abs(sum(p for (cc, g, _), p in got["deletions"].items() if cc == c and g == "*") - 1.0) < 1e-12
        assert abs(sum(p for (cc, g, _), p in got["deletions"].items() if cc == c and g != "*") - 1.0) < 1e-12
    for jn, (ex, en, sp) in zip(("VD", "DJ"), tables):
        W = sp.shape[0] - 1
        for k in range(W + 1):
            assert abs(got["insertions"].get((jn + "Insertion", k), 0.0) - np.trace(sp, k)) < 1e-15
        for a in range(W + 1):
            for b in range(W + 1):
                assert got["spans"].get((jn, a, b), 0.0) == sp[a, b]  # %.17g round-trips every double


def test_writers_format():
    """The texts: headers, column order (V5pDel, V3pDel, D5pDel, D3pDel, J5pDel, J3pDel; "*" before the genes; lengths
    ascending), %.17g, entries above 0 only; a NaN row (a sample without a finite likelihood) writes nothing."""
    import ctypes as C
    h, o = _pair(CASES[1])
    size, ng = h.events_sizes()
    rng = np.random.default_rng(5)
    dims = _dims(o)
    tables = []
    for W, nL, nR in dims:
        S = eo.sampler_tables(o)[len(tables)]
        ex, en = np.zeros((nL, W + 1)), np.zeros((nR, W + 1))
        for l in range(nL):
            ex[l, :S.left_rows[l] + 1] = rng.random(S.left_rows[l] + 1)
        for r in range(nR):
            en[r, S.right_first[r]:] = rng.random(W + 1 - S.right_first[r])
        tables.append((ex, en, np.triu(rng.random((W + 1, W + 1)))))
    genes = rng.random(ng)
    f = h.lib.lhh_phylo_map_events
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]
    out = C.c_char_p()
    row = np.ascontiguousarray(eo.flat(tables))
    assert f(h.h, row.ctypes.data, genes.ctypes.data, C.byref(out)) == 0
    dele, ins, spans = out.value.decode().split("\n\n")
    assert dele.split("\n")[0] == "column\tgene\tlength\tprobability"
    assert ins.split("\n")[0] == "junction\tlength\tprobability"
    assert spans.split("\n")[0] == "junction\tleft_rows\tright_first\tprobability"
    rows = [ln.split("\t") for ln in dele.strip("\n").split("\n")[1:]]
    order = ["V5pDel", "V3pDel", "D5pDel", "D3pDel", "J5pDel", "J3pDel"]
    keys = [(order.index(c), g, int(k)) for c, g, k, _ in rows]
    assert keys == sorted(keys) and {k[0] for k in keys} == set(range(6))
    for c in range(6):
        assert [k for k in keys if k[0] == c][0][1] == "*"
    for text in (dele, ins, spans):
        for ln in text.strip("\n").split("\n")[1:]:
            p = ln.split("\t")[-1]
            assert p == "%.17g" % float(p) and float(p) > 0
    got = host.parse_events(dele, ins, spans)
    for jn, (_, _, sp) in zip(("VD", "DJ"), tables):
        assert {(a, b): p for (j, a, b), p in got["spans"].items() if j == jn} == \
            {(a, b): sp[a, b] for a in range(sp.shape[0]) for b in range(sp.shape[0]) if sp[a, b] > 0}
    # NaN rows write empty tables
    got = h.map_events(np.full(size, np.nan), np.full(ng, np.nan))
    assert got == dict(deletions={}, insertions={}, spans={})
