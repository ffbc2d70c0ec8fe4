"""K15 (exact amino-acid replacement posteriors along the edges of a seed's lineage: lh_eval_codon_edges_batch,
lh_asr_codon_edges_batch) on the device against tests/codon_edge_oracle.py, against K12's, K13's and K14's own device
outputs and against itself.

Bounds: tables against the oracle 1e-10 absolute (ancestral_cases.BOUND); two device outputs of the same quantity 1e-12;
frequencies of N draws within 5 sigma + 1/N; what is said to have the same bits is compared with array_equal.  Every test
prints the largest deviation it saw."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import capi
from linearham_amd import posterior as lp
from tests import ancestral_probs_oracle as apo
from tests import codon_edge_oracle as ceo
from tests.ancestral_cases import BOUND
from tests.codon_edges_cases import TABLES, check, rules, synth, toy_case
from tests.codon_edges_cases import dirichlet_codons as _dirichlet
from tests.node_codons_cases import MRCA, PARENT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def test_symbol_map_is_the_hosts(hip):
    """The kernel's compile-time triple -> symbol map against posterior.aa_symbols (the host library's translation)."""
    assert np.array_equal(hip.codon_edge_symbols(), lp.aa_symbols())
    assert capi.AA_SYMBOLS == lp.AA_SYMBOLS


# ---- against the oracle ----

def _seed_op_kind(ops, tip):
    """The kind of the schedule op that takes the tip: 0 a cherry, 1 a tip-accumulate op."""
    for op in np.asarray(ops).reshape(-1, 4):
        kind = int(op[0]) & 15
        if (kind == 0 and tip in (op[1], op[2])) or (kind == 1 and op[1] == tip):
            return kind
    return None


def test_toy_family(hip, data_dir, tmp_path):
    """L = 15, T = 4: a seed under the root (a chain of one node: the seed edge and the naive edge alone) and seeds with
    a chain of two; all seed tips, three frames."""
    c = toy_case(hip, data_dir, tmp_path)
    paths = check(c, {t: [0, 1] for t in range(1, c.T)})
    assert {len(p) for p in paths} == {1, 2}


@pytest.mark.parametrize("locus", ["igh", "igk", "igl"])
def test_every_tip_as_the_seed(hip, tmp_path, locus):
    """Spec.small (8 leaves x 62 sites), three tree samples, every tip in turn as the seed: both forms of the seed edge (a
    cherry's tip, the tip of a tip-accumulate op)."""
    c = synth(hip, tmp_path, locus=locus, n_samples=3, seed={"igh": 7, "igk": 5, "igl": 6}[locus])
    kinds = {_seed_op_kind(c.ops[i], t) for i in range(3) for t in range(1, c.T)}
    assert kinds == {0, 1}
    paths = check(c, {t: [0, 1, 2] for t in range(1, c.T)})
    assert len({len(p) for p in paths}) > 1


@pytest.mark.parametrize("R", [1, 8])
def test_rate_counts_at_both_ends(hip, tmp_path, R):
    c = synth(hip, tmp_path, R=R, n_samples=2, n_leaves=17, seed=8 if R == 1 else 9)
    check(c, {t: [0, 1] for t in (1, 6, 11, 17)}, frames=(R % 3,))


def test_n_inside_columns(hip, tmp_path):
    """N in the seed's own codons and all-N columns."""
    c = synth(hip, tmp_path, n_leaves=20, n_samples=3, seed=42, ragged=6, ambiguous=0.02)
    n_n = (c.o.msa == 4).sum(axis=0)
    assert ((n_n > 0) & (n_n < c.o.msa.shape[0])).any() and (n_n == c.o.msa.shape[0]).any()
    tips = list(range(1, c.T, 7))
    assert any((c.o.msa[t - 1] == 4).any() for t in tips)
    check(c, {t: [0, 1, 2] for t in tips}, frames=(1,))


def test_ladder_of_forty(hip, tmp_path):
    """A ladder-shaped 40-leaf tree with the deepest tip as the seed: a chain of 39, the deepest slot loop; path_len padded
    beyond the chain (padding slots 0)."""
    rng = np.random.default_rng(6)

    def ladder(rows):
        import re
        leaves = [lab for lab in re.findall(r"[(,]([^(),:;\[]+)[\[:]", rows[0]["tree"]) if lab != "naive"]
        assert len(leaves) == 40
        bl = lambda: "%.6f" % max(rng.exponential(0.02), 1e-4)
        sub = "(%s:%s,%s:%s)" % (leaves[-2], bl(), leaves[-1], bl())
        for lab in reversed(leaves[1:-2]):
            sub = "(%s:%s,%s:%s)" % (lab, bl(), sub, bl())
        return [dict(rows[0], tree="(naive:%s,%s:%s,%s:%s);" % (bl(), leaves[0], bl(), sub, bl()))]
    c = synth(hip, tmp_path, rows=ladder, n_leaves=40, n_samples=1, seed=11)
    deepest = max(range(1, c.T), key=lambda t: len(c.path(0, t)))
    assert len(c.path(0, deepest)) == 39
    check(c, {deepest: [0]}, frames=(0,))
    paths = check(c, {1: [0]}, frames=(0,), pad=3)
    assert len(paths[0]) < 4


def test_many_allele_family(hip, tmp_path):
    """70 V and 33 D genes: gene groups beyond a wave in the naive codon posteriors."""
    c = synth(hip, tmp_path, n_samples=2, seed=61, locus="igh", n_v=70, n_d=33, n_j=5)
    check(c, {1: [0], 4: [1], c.T - 1: [1]}, frames=(0, 2))


# ---- the given-rates form ----

def test_more_than_256_patterns(hip, tmp_path):
    """A 20-leaf family of 340 sites with more than 256 site patterns, so K15b's pattern loop makes a second trip per wave;
    the given-rates form with a Dirichlet Q: cond_edge and the five tables against the tree-only oracle."""
    c = synth(hip, tmp_path, n_leaves=20, n_sites=340, len_v=250, len_d=(11, 20), len_j=(48, 63), v_l_width=3, v_r_width=10,
              n_samples=1, seed=17, divergence=0.1, brlen_mean=0.05, ambiguous=0.06)
    msa = np.asarray(c.o.msa)
    cols = {tuple(msa[:, j]) for j in range(c.L) if (msa[:, j] != 4).any()}
    n_prune = len(cols)
    assert c.L >= 300 and n_prune > 256, n_prune
    frame, tip = 1, 3
    nc = c.set_frame(frame)["n_codons"]
    pairs = [(0, tip)]
    Q = _dirichlet(np.random.default_rng(3), (1, nc))
    got = c.given_edges(pairs, tip, Q, want=TABLES + ("cond_edge",))
    path = c.path(0, tip)
    H = c.oracle_H(0, path, tip)
    worst_h = np.abs(got["cond_edge"][0, :len(path)] - H).max()
    want = ceo.tables(Q[0], H, frame)
    worst = max(np.abs(got[k][0] - want[k]).max() for k in TABLES)
    print("n_prune %d: cond_edge %.3g, tables %.3g from the oracle" % (n_prune, worst_h, worst))
    assert worst_h < BOUND and worst < BOUND


# ---- against K12, K13 and K14 on the device ----

def test_device_identities(hip, tmp_path):
    """sum_c cond_edge at slot 0 / the last slot = lh_eval_ancestral_candidates_batch's cond at the parent / the MRCA;
    edge_change[P] = K14's change[0..2] at the MRCA; with a one-hot N-free Q, edge_change[s][c][0] = the product over the
    codon's sites of the traces of lh_asr_edges_batch's edge[s] under the matching one-hot naive_prob.  All at 1e-12."""
    c = synth(hip, tmp_path, n_samples=3, seed=45)
    frame, tip = 1, 6
    nc = c.set_frame(frame)["n_codons"]
    pairs = [(i, tip) for i in range(3)]
    n = len(pairs)
    rng = np.random.default_rng(4)
    paths = [c.path(*p) for p in pairs]
    P = max(len(p) for p in paths)
    # K13
    got = c.given_edges(pairs, tip, _dirichlet(rng, (n, nc)), want=("cond_edge",))
    worst13 = 0.0
    for node in (PARENT, MRCA):
        cond, _ = c.probs(pairs, node, np.full((1, c.L), apo.OPEN), want=("cond",))
        for i in range(n):
            s = apo.slot_of(node, paths[i])
            worst13 = max(worst13, np.abs(got["cond_edge"][i, s].sum(axis=-1) - cond["cond"][i]).max())
    # K14
    ev, _ = c.codon_edges(pairs, tip)
    k14, _ = c.node_codons(pairs, MRCA, want=("change",))
    worst14 = max(np.abs(ev["edge_change"][:, P] - k14["change"][..., :3]).max(),
                  np.abs(ev["codon_counts"][..., 3] - k14["change"][..., 3]).max())
    # K12
    b = rng.integers(0, 4, size=(n, nc, 3))
    hot = np.zeros((n, nc, 125))
    np.put_along_axis(hot, (25 * b[..., 0] + 5 * b[..., 1] + b[..., 2])[..., None], 1.0, axis=-1)
    one = c.given_edges(pairs, tip, hot, want=("edge_change",))
    q = np.zeros((n, c.L, 5))
    q[..., 4] = 1.0
    for k in range(3):
        sites = frame + 3 * np.arange(nc) + k
        q[:, sites] = np.eye(5)[b[..., k]]
    rows = [p[0] for p in pairs]
    a = c.args(rows)
    fam = capi.Family.borrow(c.family, hip)
    _, evr = fam.eval_batch(*a, want=("rates",))
    k12 = fam.asr_edges_batch(a[0], a[1], a[2], a[3], a[4], a[5], evr["rates"], q, capi.pad_paths(paths), tip, want=("edge",))
    tr = np.trace(k12["edge"], axis1=-2, axis2=-1)                                # [n][P][L]
    worst12 = 0.0
    for i in range(n):
        for s in range(len(paths[i])):
            t3 = tr[i, s, frame:frame + 3 * nc].reshape(nc, 3)
            worst12 = max(worst12, np.abs(one["edge_change"][i, s, :, 0] - t3.prod(axis=1)).max())
    print("against K13 %.3g, K14 %.3g, K12 %.3g" % (worst13, worst14, worst12))
    assert worst13 < 1e-12 and worst14 < 1e-12 and worst12 < 1e-12


def test_given_rates_form_has_the_evaluations_bits(hip, tmp_path):
    """lh_asr_codon_edges_batch on the evaluation's rates and its own expanded K9 table: the evaluation form's bits."""
    c = synth(hip, tmp_path, n_samples=3, seed=45)
    lay = c.set_frame(1)
    tip = 1
    pairs = [(i, tip) for i in range(3)]
    k9 = c.hip.eval_codons_batch(c.family, *c.args([p[0] for p in pairs]), want=("windows", "genes"))
    Q = np.stack([lp.codon_table(c.state_space, k9["windows"][i], k9["genes"][i], lay) for i in range(3)])
    ev, _ = c.codon_edges(pairs, tip)
    got = c.given_edges(pairs, tip, Q)
    for k in TABLES:
        assert np.array_equal(got[k], ev[k]), k
    print("largest deviation 0 (bit-identical)")


# ---- batching ----

@pytest.fixture(scope="module")
def small(hip, tmp_path_factory):
    c = synth(hip, tmp_path_factory.mktemp("cedge"), n_samples=5, seed=45)
    c.set_frame(0)
    return c


def test_rows_do_not_depend_on_their_batch(small):
    c = small
    tip = 6
    pairs = [(i, tip) for i in range(4)]
    full, _ = c.codon_edges(pairs, tip)
    again, _ = c.codon_edges(pairs, tip)
    for i, p in enumerate(pairs):
        alone, _ = c.codon_edges([p], tip)
        second, _ = c.codon_edges([pairs[(i + 1) % len(pairs)], p], tip)
        for key in ("loglik", "codon_counts", "aa_counts", "seed_change"):
            assert np.array_equal(alone[key][0], full[key][i]) and np.array_equal(second[key][1], full[key][i]), key
        for key in ("loglik",) + TABLES:
            assert np.array_equal(again[key], full[key])
        # (a batch's path_len is its longest chain: the slots of a row and its naive edge keep their bits)
        k = len(c.path(*p))
        for key in ("edge_change", "edge_load"):
            for other in (alone[key][0], second[key][1]):
                assert np.array_equal(other[:k], full[key][i][:k]) and np.array_equal(other[-1], full[key][i][-1]), key
    print("largest deviation 0 (bit-identical)")


def _worker(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "codon_edges_worker.py"), mode], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_across_the_launch_group_cut():
    """LH_CODON_EDGES_MB=1 cuts a call of 11 rows into several launch groups: the rows' bits and the weighted sums stay."""
    res = _worker("groups", {"LH_CODON_EDGES_MB": "1"})
    print(res)
    assert res["n"] == 11 and res["groups"] >= 2 and res["finite"]
    assert res["mismatches"] == [] and res["weighted_sums"]


def test_weighted_sums(small):
    """n = 256 + 1 rows (one past a slab of the reduction), random log_offset: the weighted sums within n 2^-52 relative of
    a long-double host sum of the returned rows, bit-stable over two calls, and two half batches combined by
    posterior.combine within 1e-14 of the whole."""
    c = small
    n, tip = 257, 6
    rng = np.random.default_rng(12)
    pairs = [(i % 5, tip) for i in range(n)]
    off = -1000.0 + 3.0 * rng.standard_normal(n)
    members = ("codon_counts", "aa_counts", "seed_change")
    want = ("loglik",) + members + tuple("weighted_" + k for k in members) + ("weight_stats",)
    res, _ = c.codon_edges(pairs, tip, log_offset=off, want=want)
    again, _ = c.codon_edges(pairs, tip, log_offset=off, want=want)
    for k in want[4:]:
        assert np.array_equal(res[k], again[k]), k
    lw = res["loglik"] - off
    m = lw.max()
    w = np.exp(lw - m)
    st = res["weight_stats"]
    assert st[0] == m and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    h1 = 128
    a, _ = c.codon_edges(pairs[:h1], tip, log_offset=off[:h1], want=want)
    b, _ = c.codon_edges(pairs[h1:], tip, log_offset=off[h1:], want=want)
    worst = 0.0
    for k in members:
        ref = np.tensordot(w.astype(np.longdouble), res[k].astype(np.longdouble), axes=1)
        dev = np.abs(res["weighted_" + k] - ref)
        worst = max(worst, float((dev / np.where(ref > 0, ref, 1)).max()))
        assert (dev <= n * 2.0 ** -52 * np.abs(ref)).all(), k
        mean, mx, s1, s2 = lp.combine([(a["weighted_" + k], a["weight_stats"]), (b["weighted_" + k], b["weight_stats"])])
        assert np.allclose(mean, res["weighted_" + k] / st[1], rtol=1e-14, atol=1e-300)
        assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]
    print("weighted sums: worst relative difference from the long-double sum %.3g" % worst)


# ---- the extended-range mode ----

@pytest.mark.parametrize("family", ["toy", "igk"])
def test_extended_range_equals_default(hip, data_dir, tmp_path, family):
    c = toy_case(hip, data_dir, tmp_path) if family == "toy" else synth(hip, tmp_path, locus="igk", n_samples=2, seed=5)
    c.set_frame(0)
    tip = c.T - 1
    pairs = [(i, tip) for i in range(2)]
    a, paths = c.codon_edges(pairs, tip)
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    b, _ = c.codon_edges(pairs, tip)
    rules(a, paths)
    worst = max(np.abs(a[k] - b[k]).max() for k in TABLES)
    print("largest deviation %.3g" % worst)
    assert all(np.isfinite(a[k]).all() for k in TABLES) and worst < BOUND
    assert np.allclose(a["loglik"], b["loglik"], rtol=1e-12)


# ---- the _device form, refusals, the output bound ----

def test_device_entry_point_on_a_torch_stream():
    """The _device form on a stream of torch's (its own process): equal to the host-pointer form; a path that is not a chain
    and a seed that is not a child of path[0] each give that row NaN and no weight and raise the handle's error word once,
    the other rows keep their bits; the host-pointer form refuses both."""
    res = _worker("device")
    print(res)
    assert res["clean_status"] == "" and res["clean_equals_host"]
    for k in ("not_a_chain", "not_a_child"):
        assert res[k]["victim_all_nan"] and res[k]["others_unchanged"] and res[k]["weights_leave_the_victim_out"], k
        assert "not a chain" in res[k]["status"] and res[k]["second_status"] == "", k
    assert "is not a chain" in res["host_not_a_chain"] and "is not a child of path[0]" in res["host_not_a_child"]


def test_refusals(hip, tmp_path):
    c = synth(hip, tmp_path, n_samples=1, seed=37)
    tip = 1
    path = capi.pad_paths([c.path(0, tip)])
    a = c.args([0])
    import ctypes as C
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ll = np.zeros(1)
    outs = capi._CodonEdgesOutputs()
    outs.loglik = ll.ctypes.data_as(f64)
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in a[3:7]]
    ops32 = np.ascontiguousarray(a[2], dtype=np.int32)
    raw = lambda seed: hip.lib.lh_eval_codon_edges_batch(c.family, 1, a[0], a[1], ops32.ctypes.data_as(i32),
                                                         *[x.ctypes.data_as(f64) for x in arrs], a[7],
                                                         path.ctypes.data_as(i32), path.shape[1], seed, C.byref(outs))
    assert raw(tip) != 0 and "no frame set" in hip.error()
    c.set_frame(0)
    assert raw(tip) == 0 and np.isfinite(ll[0])
    assert raw(0) != 0 and "seed_tip must be a tip other than naive" in hip.error()
    assert raw(c.T) != 0 and "seed_tip must be a tip other than naive" in hip.error()
    other = [u for u in range(1, c.T) if c.path(0, u)[0] != c.path(0, tip)[0]][0]
    with pytest.raises(RuntimeError, match="is not a child of path\\[0\\]"):
        c.hip.eval_codon_edges_batch(c.family, *a, path, other)
    # the extended-range mode is honoured
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    res, _ = c.codon_edges([(0, tip)], tip)
    assert all(np.isfinite(res[k]).all() for k in TABLES)


def test_output_bound_names_the_largest_n():
    """The refusal of the host-pointer form, through its hook (LH_EDGE_OUT_MB=1, read once per process)."""
    res = _worker("bound", {"LH_EDGE_OUT_MB": "1"})
    print(res)
    assert res["most"] > 8
    assert "batch too large" in res["message"] and "at most %d samples per call" % res["most"] in res["message"]
    assert res["largest_passes"]


# ---- what the numbers are expectations of ----

def test_tables_against_device_draws(hip, data_dir, tmp_path):
    """20 000 draws of the device on row 1, tip 1 of the toy family through lh_eval_lineage_batch (naive states from the
    posterior, their sequences, one ancestral draw of the lineage under each), classified per edge and codon on the host.
    edge_change is a probability: its frequency lies within 5 sigma + 1/N.  A cell of aa_counts is the mean of a count k
    in 0 .. E (E = len + 1 edges), whose variance is at most E times its mean (k^2 <= E k): the mean of N draws lies within
    5 sqrt(E p / N) + E / N."""
    from oracle import linearham_oracle as orc
    c = toy_case(hip, data_dir, tmp_path)
    row, tip, N, frame = 1, 1, 20000, 0
    path = c.path(row, tip)
    P = len(path)
    assert P == 2
    nc = c.set_frame(frame)["n_codons"]
    T, depth, ops, brl, er, pi, alpha, R = c.args([row])
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a), N, axis=0))
    fam = capi.Family.borrow(c.family, hip)
    nw = hip.lib.lh_sample_words(c.family)
    rng = orc.MT19937(5)
    words = np.array([rng() for _ in range(N * nw)], dtype=np.uint32).reshape(N, nw)
    chain = fam.eval_lineage_batch(T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(alpha), R, words, 23,
                                   rep(capi.pad_paths([path])))
    assert np.isfinite(chain["loglik"]).all()
    naive = chain["naive"].astype(np.int64)
    flat = (np.arange(N) * (P + 1))[:, None] + np.arange(P)[None, :]
    nodes = fam.lineage_rows_read(flat.reshape(-1), c.L).reshape(N, P, c.L).astype(np.int64)
    seed = np.asarray(c.o.msa)[tip - 1].astype(np.int64)
    sl = [slice(frame + k, frame + 3 * nc, 3) for k in range(3)]
    # a codon of the seed with an N is not observed: the draws say nothing about its lower end on the seed edge
    seen = np.array([(seed[frame + 3 * k:frame + 3 * k + 3] < 4).all() for k in range(nc)])
    assert seen.sum() >= nc - 1
    tri = lambda s: 16 * s[..., sl[0]] + 4 * s[..., sl[1]] + s[..., sl[2]]
    x = tri(nodes)                                                                # [N][P][nc]
    xs = np.broadcast_to(tri(np.where(seed < 4, seed, 0)), (N, nc))
    res, _ = c.codon_edges([(row, tip)], tip)
    cls, sym = lp.edge_classes(), lp.aa_symbols()
    worst = 0.0
    counts = np.zeros((N, nc, 21, 21))
    ar = np.arange(N)
    for s in range(P):
        up, lo = x[:, s], (x[:, s - 1] if s > 0 else xs)
        k = cls[up, lo]
        for cdn in np.nonzero(seen | (s > 0))[0]:
            p = np.clip(res["edge_change"][0, s, cdn], 0.0, 1.0)
            freq = np.bincount(k[:, cdn], minlength=3) / N
            worst = max(worst, np.abs(freq - p).max())
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (s, cdn)
            np.add.at(counts, (ar, cdn, sym[up[:, cdn]], sym[lo[:, cdn]]), 1.0)
    # the naive edge: the naive triples without an N
    b = [naive[:, sl[k]] for k in range(3)]
    free = (b[0] < 4) & (b[1] < 4) & (b[2] < 4)
    nb = np.where(free, 16 * b[0] + 4 * b[1] + b[2], 0)
    k = np.where(free, cls[nb, x[:, P - 1]], 3)
    for cdn in range(nc):
        p = np.clip(np.append(res["edge_change"][0, P, cdn], res["codon_counts"][0, cdn, 3]), 0.0, 1.0)
        freq = np.bincount(k[:, cdn], minlength=4) / N
        worst = max(worst, np.abs(freq - p).max())
        assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), ("naive", cdn)
        f = free[:, cdn]
        np.add.at(counts, (ar[f], cdn, sym[nb[f, cdn]], sym[x[f, P - 1, cdn]]), 1.0)
    E = P + 1
    mean = counts.mean(axis=0)
    p = np.clip(res["aa_counts"][0], 0.0, E)
    worst = max(worst, np.abs(mean - p)[seen].max())
    assert (np.abs(mean - p) <= 5 * np.sqrt(E * p / N) + E / N)[seen].all()
    print("largest deviation of a frequency %.3g" % worst)


# ---- the host library: PhyloHMM::LineageReplacements, the pipeline over a RevBayes table, the CLI ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _check_files(res, per_row, first, frame):
    used = per_row[first:]
    lw = np.array([r[0] for r in used])
    w = np.exp(lw - lw.max())
    mean = {k: sum(wi * r[1][k] for wi, r in zip(w, used)) / w.sum() for k in ("codon_counts", "aa_counts", "seed_change")}
    off = 1.0 - np.eye(21)
    worst = max(np.abs(res["codon_counts"] - mean["codon_counts"]).max(), np.abs(res["seed_change"] - mean["seed_change"]).max(),
                np.abs(res["aa_counts"] - mean["aa_counts"] * off).max())
    print("pipeline: worst difference from the oracle's weighted tables %.3g" % worst)
    assert worst < BOUND
    assert [r[0] for r in res["rows"]] == list(range(first, 9))
    assert np.allclose([r[1] for r in res["rows"]], w, rtol=1e-9)
    assert [r[2] for r in res["rows"]] == [r[2] for r in used]
    for got, r in zip(res["rows"], used):
        assert abs(got[3] - r[1]["codon_counts"][:, 1].sum()) < BOUND and abs(got[4] - r[1]["codon_counts"][:, 2].sum()) < BOUND
    sm = res["summary"]
    assert sm["rows_used"] == 9 - first and sm["rows_skipped_nonfinite"] == 0 and sm["frame"] == frame
    assert abs(sm["kish_ess"] - w.sum() ** 2 / (w * w).sum()) < 1e-9 * sm["kish_ess"]
    # the summary's expectations are the column sums of the codon changes, and of the off-diagonal cells
    assert abs(sm["expected_synonymous"] - res["codon_counts"][:, 1].sum()) < 1e-12
    assert abs(sm["expected_replacement"] - res["codon_counts"][:, 2].sum()) < 1e-12
    assert abs(sm["expected_replacement"] - res["aa_counts"].sum()) < 1e-10


def test_pipeline_and_cli(hip, tmp_path):
    """PhyloHMM::RunLineageReplacementsPipeline on a 9-row table, through the library (burn-in 0.25) and through `linearham
    --lineage-replacements-pipeline` (no burn-in; with LH_PIPELINE_BATCH 2 and 4: byte-identical files), against the
    oracle's per-row tables weighted by exp(LHLogLikelihood - Likelihood); then PhyloHMM::LineageReplacements and `linearham
    --lineage-replacements` on the first row's tree."""
    from linearham_amd import host
    from tests.codon_edges_cases import CodonEdgesCase
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=9, seed=41), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = CodonEdgesCase(hip, yaml_path, pdir, rows, 4, tmp_path)
    tip, frame = 3, 1
    seed_seq = list(c.o.xmsa_labels)[tip]
    c.frame = frame
    per_row = []
    for i in range(9):
        path = c.path(i, tip)
        Q = c.naive_codons(i)
        ll = c.o.log_likelihood()
        per_row.append((ll - rows[i]["likelihood"], ceo.tables(Q, c.oracle_H(i, path, tip), frame), len(path)))
    _check_files(c.hh.run_lineage_replacements_pipeline(tsv, seed_seq, str(tmp_path / "lib"), 4, burnin_frac=0.25, frame=frame),
                 per_row, 2, frame)
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq,
              "--frame", str(frame)]
    names = (("cli", {}), ("cli2", {"LH_PIPELINE_BATCH": "2"}), ("cli4", {"LH_PIPELINE_BATCH": "4"}))
    for name, env in names:
        r = subprocess.run([_exe(), "--lineage-replacements-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / name)]
                           + common, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
    _check_files(host.read_lineage_replacements(str(tmp_path / "cli")), per_row, 0, frame)
    for f in ("replacements.tsv", "codon_changes.tsv", "seed_edge.tsv", "rows.tsv", "summary.tsv"):
        whole = open(str(tmp_path / "cli") + "." + f, "rb").read()
        for name, _ in names[1:]:
            assert open(str(tmp_path / name) + "." + f, "rb").read() == whole, (name, f)
    # one tree
    row = c.rows[0]
    path = c.path(0, tip)
    Q = c.naive_codons(0)
    ll = c.o.log_likelihood()
    want = ceo.tables(Q, c.oracle_H(0, path, tip), frame)
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one = c.hh.lineage_replacements(seed_seq, frame)
    assert one["nodes"] == list(path) and abs(one["loglik"] - ll) < 1e-9 * abs(ll)
    worst = max(np.abs(one[k] - want[k]).max() for k in TABLES)
    newick = str(tmp_path / "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    args = [_exe(), "--lineage-replacements", "--newick-path", newick, "--alpha", repr(row["alpha"])] + common
    args += sum([["--er", repr(x)] for x in row["er"]], []) + sum([["--pi", repr(x)] for x in row["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = host.parse_lineage_replacements(r.stdout)
    assert np.array_equal(got["codon_counts"], one["codon_counts"]) and np.array_equal(got["seed_change"], one["seed_change"])
    assert np.array_equal(got["aa_counts"], one["aa_counts"] * (1.0 - np.eye(21)))
    edges = [ln.split("\t") for ln in r.stdout.strip("\n").split("\n\n")[3].split("\n")]
    assert edges[0] == ["edge", "upper", "lower", "expected_synonymous", "expected_replacement"] and len(edges) == len(path) + 2
    assert np.array_equal(np.array([[float(x) for x in e[3:]] for e in edges[1:]]), one["edge_load"])
    print("one tree: worst difference from the oracle %.3g" % worst)
    assert worst < BOUND
