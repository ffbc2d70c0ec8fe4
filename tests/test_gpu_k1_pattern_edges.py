"""K1 (lh_prune.hip) and lh_family_create's state planes at their pattern-count edges, against the oracle.

launch_prune picks its kernel from L = n_prune, R and the tree size: n2 = L / 128 two-site waves per rate, one more for a
remainder above 64, ONE one-site wave for a remainder of 1 to 64; all rates in one workgroup while R * wpr <= 8 (<= 16
within 80 KB of LDS); tiles of at most 1 024 patterns in blocks of 128; the register budgets ct6 / ct5 / ct4 by the LDS left
per CU.  tests/pattern_edge_cases.py builds families with exactly L distinct alignment columns, no two of whose emissions
are within 1e-7 of each other, so that a lane reading a neighbour's, the clamped last or another tile's pattern fails the
1e-10 emission bound.

TABLE holds the cases with the kernel form each must run, LITERALLY: read off launch_prune by hand (columns n2, n1, tiles,
fused; the form string is what lh_family_prune_form reports).  A later change of the selection rule then shows as a failing
expectation here instead of silently moving a case off its kernel.  (R * wpr = 17 cannot be formed from the R of the list
with at most eight waves per rate: the upper side of the 16-wave limit is taken at 18, 20, 21 and 24 waves.)

Every process is a child (tests/k1_pattern_edges_worker.py) under its own time limit; nothing is started after a child that
did not end cleanly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.pattern_edge_cases import K1_L, K1_N_L, Case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "k1_pattern_edges_worker.py")
_stopped = []

F, U = True, False      # fused: all rates in one workgroup | a workgroup per (sample, rate)


def _ct(budget, n_aware, fused, asm):
    low = lambda b: "true" if b else "false"
    return "ct%d<4,%s,%s,%s>" % (budget, low(n_aware), low(fused), low(asm))


def _row(base, L, R, n2, n1, tiles, fused, budget, mixed=False, all_n=False):
    """A table row: (case, R, form in the default mode, form in the extended-range mode -- the C++ walk --, n2, n1, tiles, fused)."""
    return (Case(base, L, mixed=mixed, all_n=all_n), R, _ct(budget, mixed, fused, True), _ct(budget, mixed, fused, False), n2, n1, tiles, fused)


# the R = 4 list on the 10-leaf family (T = 11: a tip table of 1 408 bytes, so the exchange area [R][pad] * 44 bytes decides)
_R4 = [
    #  L   n2 n1 tiles fused budget
    (1, 0, 1, 1, F, 6), (2, 0, 1, 1, F, 6), (63, 0, 1, 1, F, 6), (64, 0, 1, 1, F, 6),
    (65, 1, 0, 1, F, 6), (127, 1, 0, 1, F, 6), (128, 1, 0, 1, F, 6),
    (129, 1, 1, 1, F, 6), (191, 1, 1, 1, F, 6), (192, 1, 1, 1, F, 6),
    (193, 2, 0, 1, F, 6), (255, 2, 0, 1, F, 6), (256, 2, 0, 1, F, 6),
    (257, 2, 1, 1, F, 6), (320, 2, 1, 1, F, 6),                     # 12 waves, 56 320 bytes
    (321, 3, 0, 1, F, 6), (384, 3, 0, 1, F, 6),                     # 12 waves, 67 584 bytes
    (385, 3, 1, 1, F, 6),                                           # 16 waves, 78 848 bytes: the largest fused workgroup
    (511, 4, 0, 1, U, 6), (512, 4, 0, 1, U, 6),                     # 16 waves but 90 112 bytes: past the 80 KB limit
    (513, 4, 1, 1, U, 6), (1023, 8, 0, 1, U, 6), (1024, 8, 0, 1, U, 6),
    (1025, 5, 0, 2, U, 6),                                          # two tiles of 640
]
assert tuple(r[0] for r in _R4) == K1_L

TABLE = [_row("s1100", L, 4, n2, n1, tiles, fused, b) for L, n2, n1, tiles, fused, b in _R4] + [
    # R * wpr at 8 | 9
    _row("s1100", 512, 2, 4, 0, 1, F, 6),        # 8 waves, 45 056 bytes
    _row("s1100", 1024, 1, 8, 0, 1, F, 6),       # 8 waves of one rate
    _row("s1100", 320, 3, 2, 1, 1, F, 6),        # 9 waves
    # 16 | more
    _row("s1100", 192, 8, 1, 1, 1, F, 6),        # 16 waves, 67 584 bytes
    _row("s1100", 768, 3, 6, 0, 1, U, 6),        # 18
    _row("s1100", 385, 5, 3, 1, 1, U, 6),        # 20
    _row("s1100", 257, 7, 2, 1, 1, U, 6),        # 21
    _row("s1100", 257, 8, 2, 1, 1, U, 6),        # 24
    # workgroups of 5, 6, 7, 14 and 15 waves
    _row("s1100", 64, 5, 0, 1, 1, F, 6), _row("s1100", 129, 3, 1, 1, 1, F, 6), _row("s1100", 65, 7, 1, 0, 1, F, 6),
    _row("s1100", 129, 7, 1, 1, 1, F, 6), _row("s1100", 257, 5, 2, 1, 1, F, 6), _row("s1100", 513, 3, 4, 1, 1, F, 6),
    _row("s1100", 1, 1, 0, 1, 1, F, 6),          # one wave in all
    # R = 2 at one tile | two tiles: 16 waves past the LDS limit | two fused tiles of 640 in ten waves, 56 320 bytes: ct5
    _row("s1100", 1024, 2, 8, 0, 1, U, 6), _row("s1100", 1025, 2, 5, 0, 2, F, 5),
    # the 256- and 257-site families
    _row("s256", 255, 4, 2, 0, 1, F, 6), _row("s257", 255, 4, 2, 0, 1, F, 6), _row("s256", 129, 2, 1, 1, 1, F, 6),
    # one all-N site beside the patterns (alignment padding): n_prune and the form stay, lh_family_info's second figure moves
    _row("s1100", 64, 4, 0, 1, 1, F, 6, all_n=True), _row("s1100", 1025, 4, 5, 0, 2, U, 6, all_n=True),
    _row("s256", 255, 4, 2, 0, 1, F, 6, all_n=True), _row("s257", 255, 4, 2, 0, 1, F, 6, all_n=True),
] + [
    # N in some patterns: the N-aware kernels
    _row("s1100", L, 4, n2, n1, tiles, fused, b, mixed=True) for L, n2, n1, tiles, fused, b in _R4 if L in K1_N_L
] + [
    # (Both families' J alleles reach the end of the alignment: with J alleles of unequal length these rows met a fault of
    # K2a's extended-range mode, not of K1 -- tests/pattern_edge_cases.BASES and DESIGN section 2, "Pattern-count edges".)
    # 60 leaves (tip tables of 7 808 bytes: four of them 31 728 bytes with the walk descriptors -- five workgroups per CU)
    _row("t60", 64, 4, 0, 1, 1, F, 5), _row("t60", 128, 4, 1, 0, 1, F, 5), _row("t60", 129, 4, 1, 1, 1, F, 6),
    # 100 leaves (12 928 bytes each, four 52 528: three workgroups per CU)
    _row("t100", 64, 4, 0, 1, 1, F, 4), _row("t100", 65, 4, 1, 0, 1, F, 4), _row("t100", 129, 4, 1, 1, 1, F, 6),
    # and a one-site wave beside a two-site wave under ct5: five tip tables, 65 456 bytes, ten waves
    _row("t100", 129, 5, 1, 1, 1, F, 5),
]
assert sorted(r[0].L for r in TABLE if r[0].mixed) == sorted(K1_N_L)


def r4_rows():
    return TABLE[:len(_R4)]


# The hook processes run the R = 4 list.  The hooks only push a shape onto a form another shape takes by itself, with the
# same n2 / n1 split: (form of a row that is fused by default, form of one that is not), default mode then extended range.
HOOKS = {
    # the register-stack form for fused shapes; this family's two tree samples have stack depth 1 (up to 3: the w6 budget)
    "stack": (dict(LH_K1_STACK="1"), ("w6<3,false>", _ct(6, False, U, True)), ("w6<3,false>", _ct(6, False, U, False))),
    "no_fuse": (dict(LH_K1_NO_FUSE="1"), (_ct(6, False, U, True),) * 2, (_ct(6, False, U, False),) * 2),
    "segments": (dict(LH_K1_SEGMENTS="1"), ("seg4<4,false>",) * 2, ("seg4<4,false>",) * 2),
    "tables_cxx": (dict(LH_K1_TABLES="1", LH_K1_CXX_WALK="1"), (_ct(6, False, F, False), _ct(6, False, U, False)),
                   (_ct(6, False, F, False), _ct(6, False, U, False))),
}
BETWEEN_FORMS = 1e-13        # emissions between two forms of K1


def _child(which, workdir, env=None, limit=90):        # (a hook process takes 5 to 7 s, the default one 12 s)
    assert not _stopped, "not started: an earlier child did not end cleanly (%s)" % _stopped[0]
    out = os.path.join(workdir, "k1_%s.npz" % "_".join(sorted(env or {"default": ""})).lower())
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, WORKER, which, workdir, out]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        _stopped.append("%s: exit status %d" % (which, r.returncode))
        raise AssertionError("%s %s: exit status %d\n%s\n%s" % (which, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for rec in res["rows"]:
        print(rec["key"], rec["form"], rec["form_ext"], json.dumps(rec["figures"]))
    return res, np.load(out)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("k1_edges"))


@pytest.fixture(scope="module")
def default(workdir):
    return _child("default", workdir, limit=150)


def _check(res, table, forms):
    assert [r["key"] for r in res["rows"]] == ["%s_R%d" % (row[0].name, row[1]) for row in table]
    bad = []
    for rec, row, (form, form_ext) in zip(res["rows"], table, forms):
        if rec["form"] != form or rec["form_ext"] != form_ext:
            bad.append("%s: ran %s / %s, the table says %s / %s" % (rec["key"], rec["form"], rec["form_ext"], form, form_ext))
        if rec["n_patterns"] != row[0].L:
            bad.append("%s: n_prune %d" % (rec["key"], rec["n_patterns"]))
        bad += ["%s: %s" % (rec["key"], f) for f in rec["failures"]]
        assert len(rec["premises"]) == 2 and len(rec["figures"]) == 8
    assert not bad, "\n".join(bad)


def test_every_case_matches_the_oracle_on_its_literal_form(default):
    res, _ = default
    assert len(TABLE) == 24 + 24 + 8 + 7
    _check(res, TABLE, [(row[2], row[3]) for row in TABLE])


def test_the_forms_reached_cover_the_launcher(default):
    res, _ = default
    forms = {rec["form"] for rec in res["rows"]} | {rec["form_ext"] for rec in res["rows"]}
    ran = {rec["key"]: rec["form"] for rec in res["rows"]}
    for b in ("ct6", "ct5", "ct4"):
        assert any(f.startswith(b) for f in forms), b
    parts = [tuple(f[f.index("<") + 1:-1].split(",")) for f in forms]
    assert {p[2] for p in parts} == {"true", "false"}, "fused and unfused"
    assert {p[3] for p in parts} == {"true", "false"}, "assembly and C++ walk"
    assert {p[1] for p in parts} == {"true", "false"}, "N-aware and not"
    rows = {"%s_R%d" % (row[0].name, row[1]): row for row in TABLE}
    beside = [k for k, row in rows.items() if row[5] == 1 and row[4] >= 1]
    alone = [k for k, row in rows.items() if row[5] == 1 and row[4] == 0]
    two_tiles = [k for k, row in rows.items() if row[6] == 2]
    assert beside and alone and two_tiles and all(k in ran for k in beside + alone + two_tiles)
    # the budgets below ct6 with a one-site wave and without one
    for b in ("ct5", "ct4"):
        assert {rows[k][5] for k, f in ran.items() if f.startswith(b)} == {0, 1}, b
    # an all-N site beside the patterns: n_prune stays L, the (naive base, pattern) pairs in use differ (each figure is
    # asserted in the worker against the alignment, through lh_family_info)
    info = {rec["key"]: rec["info"] for rec in res["rows"]}
    assert all(info[k][0] == rows[k][0].L for k in rows)
    padded = [k for k in rows if rows[k][0].all_n]
    assert len(padded) == 4
    assert all(info[k][0] == info[k.replace("_pad", "")][0] for k in padded)
    # (where the site that became all N was not the only one to read its (naive base, pattern) pair, the second figure grows)
    assert info["s256_L255_pad_R4"][1] == info["s256_L255_R4"][1] + 1


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_hook_forms_match_the_oracle_and_the_default_process(default, workdir, hook):
    env, forms, forms_ext = HOOKS[hook]
    table = r4_rows()
    res, arrays = _child("r4", workdir, env=env)
    _check(res, table, [(forms[0 if row[7] else 1], forms_ext[0 if row[7] else 1]) for row in table])
    _, base = default
    worst = 0.0
    for rec in res["rows"]:
        k = rec["key"]
        for em, sco in (("_em", "_sco"), ("_emx", "_scox")):
            assert np.array_equal(arrays[k + sco], base[k + sco]), (k, "scaler counts differ from the default process")
            d = float(np.max(np.abs(arrays[k + em] - base[k + em]) / base[k + em]))
            worst = max(worst, d)
            assert d <= BETWEEN_FORMS, (k, em, d)
    print(hook, "largest emission deviation from the default process: %.3g" % worst)
