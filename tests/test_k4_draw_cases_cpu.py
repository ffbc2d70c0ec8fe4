"""The rows of tests/k4_draw_cases.py, checked on the numpy oracle without a GPU: per family, on the oracle's own forward
arrays,
  * every tier-2 row (a random stream on a finite case) keeps every uniform further than 1e-7 relative from every partial
    sum at which its answer changes -- a hundred times the 1e-9 to which the device's forward arrays agree with the
    oracle's -- so the end-to-end oracle is a fair reference for those rows;
  * every row consumes exactly the words the structure says (two per region or junction row with more than one state),
    the rows of all-ones words and of `hi1` included (a draw beyond the last partial sum takes no more and no fewer);
  * the rows reach what they are for, so that no device test passes vacuously:
      (a) a draw with no positive weight, in a finite row (heavy chains; see LIGHT below);
      (b) a draw beyond the last partial sum that returns the dense vector's last element;
      (c) a drawn state of zero weight that a later draw follows;
      (d) a wave whose rows find their answers in different 16-gene chunks of the same draw (families with a set of more
          than 16 genes);
      (e) a wave with a chunk that is all zero in one row and not in another, one of the two a `zero` row;
      (f) a non-finite row (delta4) sharing a wave with finite rows (families that can express delta4)."""
import numpy as np
import pytest

from tests import k2_scaling_cases as kc
from tests import k4_draw_cases as k4

# a germline set of more than 16 genes: (d) can happen
MULTI_CHUNK = ("igh_70_33_5", "igh_v130_d30_j12", "igh_v260", "igh_d65", "igk_v70_j70")
# Light chains.  A uniform of 0 picks element 0 of the dense vector whatever it holds.  In a heavy chain's D-J junction that is
# a D allele's (the left gene's) state of row 0, which has zero weight on every other row and no predecessor with a forward
# entry: the next draw has no positive weight, (a).  In a light chain's only junction the J alleles sort first and element 0
# is an NTI state, which has predecessors on every row; (a) then needs (b) on a junction row -- the last element is a V
# allele's state of the last row -- and whether the last partial sum falls below the largest uniform, 1 - 2^-53, is a matter
# of rounding: on the oracle's own forward arrays it never does in small_igk, and in igk_v70_j70 only in draws whose last
# element has a positive weight (on the device's arrays, which differ in the last bits, it does in both: the device test
# prints its own counts).  Here their draws without a positive weight are those of delta4's NaN rows.
LIGHT = {"small_igk": ("a_finite", "b"), "igk_v70_j70": ("a_finite",)}


def test_layout():
    rows = k4.layout(5)
    assert len(rows) == 41 and rows[-1] == (0, 0)
    assert {(c, p) for c, p in rows[:-1]} == {(c, p) for c in range(5) for p in range(8)}   # every case meets every pattern
    for w in range(0, 40, 4):
        wave = rows[w:w + 4]
        assert len({c for c, _ in wave}) == 4 and len({p for _, p in wave}) > 1                # unlike rows in every wave
    pat = k4.patterns(8, 1)
    assert pat.shape == (8, 8) and pat.dtype == np.uint32
    assert not pat[0].any() and (pat[1] == 0xFFFFFFFF).all() and list(pat[2][:2]) == [1, 0]
    assert list(pat[3][:2]) == [0xFFFFF800, 0xFFFFFFFF] and set(np.unique(pat[4])) <= {0, 0xFFFFFFFF}


@pytest.mark.parametrize("name", k4.FAMILIES)
def test_rows_on_the_oracle(tmp_path, name):
    h, rows = k4.build_rows(name, tmp_path)
    assert [c.name for c in rows.cases][0] == "base" and all(n in [c.name for c in rows.cases] for n in kc.NEED[name])
    assert rows.n_words == 2 * sum(1 for s in k4.draw_sizes(h) if s > 1) and rows.n_words <= 624
    worst, tier2 = k4.check_margins(h, rows)
    assert len(tier2) == 3 * sum(1 for c in rows.cases if c.expect == "finite")
    recorded = []
    for r in range(rows.n):
        st, used, draws = k4.draws_end_to_end(h, rows.em[r], rows.words[r], record=True)
        assert used == rows.n_words, (r, rows.layout[r], used)
        assert st.shape == (len(k4.draw_sizes(h)),) and np.all(st >= 0) and np.all(st < np.array(k4.draw_sizes(h)))
        if r in tier2:
            assert np.array_equal(st, tier2[r])
        recorded.append(draws)
    cl = k4.classes(h, rows, recorded)
    print("%s: n = %d rows of %d words, %d tier-2 rows, worst margin %.3e, classes %s, %s form"
          % (name, rows.n, rows.n_words, len(tier2), worst, cl, "saved" if k4.saves_weights(h) else "recompute"))
    for key in ("a", "a_finite", "b", "c", "e", "e_zero"):
        assert cl[key] >= 1 or key in LIGHT.get(name, ()), (key, cl)
    assert (h.locus == "igh") == (name not in LIGHT)
    if name in MULTI_CHUNK:
        assert k4.widest_draw(h) > k4.kG and cl["d"] >= 1 and cl["d_max"] >= 3, cl
    else:
        assert k4.widest_draw(h) == k4.kG
    if "delta4" in kc.NEED[name]:
        assert cl["f"] >= 1, cl
    assert k4.saves_weights(h) == (name != "igh_v260")
