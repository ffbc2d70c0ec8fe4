"""K14 (exact codon marginals of a node of a seed's lineage: lh_eval_node_codons_batch, lh_asr_node_codons_batch) on the
device against tests/node_codon_oracle.py, against K13's and K11's own device outputs and against itself.

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
from tests import node_codon_oracle as nco
from tests.ancestral_cases import BOUND
from tests.node_codons_cases import HAS_N, MRCA, NODES, PARENT, check, synth, toy_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def test_class_table_is_the_hosts(hip):
    """The kernel's compile-time class relation against posterior.change_classes (the host library's translation)."""
    assert np.array_equal(hip.node_codon_classes(), lp.change_classes())


# ---- against the oracle ----

def test_toy_family(hip, data_dir, tmp_path):
    """L = 15: five codons in frame 0, four with leftover sites in frames 1 and 2; T = 4: a seed under the root (parent =
    MRCA: the same bits) and seeds with a chain of two."""
    c = toy_case(hip, data_dir, tmp_path)
    paths = check(c, [(i, t) for i in range(2) for t in range(1, c.T)])
    assert {len(p) for p in paths} == {1, 2}
    assert c.L == 15 and [c.set_frame(f)["n_codons"] for f in range(3)] == [5, 4, 4]


@pytest.mark.parametrize("locus", ["igh", "igk", "igl"])
def test_every_tip_as_the_seed(hip, tmp_path, locus):
    """Spec.small (8 leaves x 62 sites), three tree samples, every tip in turn as the seed in one batch; a light-chain
    codon spans V | V-J rows | J.  These families have codons with a site no state covers: their naive triple is N with
    probability 1 and class 3 takes everything."""
    c = synth(hip, tmp_path, locus=locus, n_samples=3, seed={"igh": 7, "igk": 5, "igl": 6}[locus])
    pairs = [(i, t) for t in range(1, c.T) for i in range(3)]
    paths = check(c, pairs)
    assert len({len(p) for p in paths}) > 1
    c.set_frame(0)
    res, _ = c.node_codons(pairs[:1], MRCA)
    Q = c.naive_codons(0)
    open_codons = np.nonzero(Q[:, HAS_N].sum(axis=1) == 1.0)[0]
    assert len(open_codons) > 0 and np.abs(res["change"][0, open_codons, 3] - 1.0).max() < 1e-12  # (a sum of gene posteriors)
    assert not res["change"][0, open_codons, :3].any()


@pytest.mark.parametrize("R", [1, 8])
def test_rate_counts_at_both_ends(hip, tmp_path, R):
    c = synth(hip, tmp_path, R=R, n_samples=2, n_leaves=17, seed=8 if R == 1 else 9)
    check(c, [(i, t) for t in (1, 6, 11, 17) for i in range(2)], frames=(R % 3,))


@pytest.mark.parametrize("preset", ["mixed_n", "mixed_n_deep"])
def test_n_inside_columns(hip, tmp_path, preset):
    """N inside columns and all-N columns; the balanced 64-leaf tree."""
    kw = {"mixed_n": dict(n_leaves=20, n_samples=3, seed=42, ragged=6, ambiguous=0.02),
          "mixed_n_deep": dict(n_leaves=64, n_samples=2, seed=49, tree_shape="balanced", n_nni=0, ragged=6, ambiguous=0.01)}
    c = synth(hip, tmp_path, **kw[preset])
    n_n = (c.o.msa == 4).sum(axis=0)
    assert ((n_n > 0) & (n_n < c.o.msa.shape[0])).any() and (n_n == c.o.msa.shape[0]).any()
    check(c, [(i, t) for t in range(1, c.T, 7) for i in range(len(c.rows))], frames=(1,) if preset == "mixed_n" else (2,))


def test_ladder_of_forty(hip, tmp_path):
    """A ladder-shaped 40-leaf tree with the deepest tip as the seed: a chain of 39."""
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
    paths = check(c, [(0, deepest), (0, 1)], frames=(0,))
    assert len(paths[0]) == 39


@pytest.mark.parametrize("name,kw", [("igh_70_33", dict(locus="igh", n_v=70, n_d=33, n_j=5)),
                                     ("igh_v260", dict(locus="igh", n_v=260, n_d=3, n_j=3))])
def test_many_allele_families(hip, tmp_path, name, kw):
    """Regions with more genes than a wave has lanes: a germline codon's naive posterior is summed over groups of genes."""
    c = synth(hip, tmp_path, n_samples=2, seed=61, **kw)
    ss = c.state_space
    assert max(len(ss[r + "_ggene_ranges"]) for r in ("vgerm", "dgerm", "jgerm")) > 64
    check(c, [(0, 1), (1, 4), (1, c.T - 1)], frames=(0, 2))


# ---- against K13 and K11 on the device ----

@pytest.mark.parametrize("locus", ["igh", "igk"])
def test_against_k13_and_k11_on_the_device(hip, tmp_path, locus):
    """For the first codon, a junction codon and the last one, exp(log_cand) of the 64 three-site candidates (K13's sweeps)
    against codons within 1e-10; the site marginals of codons against lh_eval_ancestral_batch's marg at the node's slot
    within 1e-12."""
    c = synth(hip, tmp_path, locus=locus, n_samples=2, seed=5 if locus == "igk" else 7)
    pairs = [(0, 1), (1, 4)]
    worst13 = worst11 = 0.0
    for frame in (0, 1):
        lay = c.set_frame(frame)
        nc = lay["n_codons"]
        picked = [0, lay["window_codon"][len(lay["window_codon"]) // 2], nc - 1]
        cands = np.concatenate([nco.triple_candidates(c.L, frame, k) for k in picked])
        k11, _ = c.run(pairs, want=("marg",))
        for node in NODES:
            res, paths = c.node_codons(pairs, node)
            k13, _ = c.probs(pairs, node, cands, want=("log_cand",))
            for i in range(len(pairs)):
                for j, k in enumerate(picked):
                    worst13 = max(worst13, np.abs(np.exp(k13["log_cand"][i, 64 * j:64 * j + 64]) - res["codons"][i, k]).max())
                m = nco.site_marginals(res["codons"][i]).reshape(-1, 4)
                worst11 = max(worst11, np.abs(m - k11["marg"][i, apo.slot_of(node, paths[i]), frame:frame + 3 * nc]).max())
    print("against K13: %.3g, against K11: %.3g" % (worst13, worst11))
    assert worst13 < BOUND and worst11 < 1e-12


# ---- the given-rates form ----

def test_given_rates_form(hip, tmp_path):
    c = synth(hip, tmp_path, n_samples=3, seed=45)
    lay = c.set_frame(1)
    nc = lay["n_codons"]
    pairs = [(i, t) for i in range(3) for t in (1, 6)]
    n = len(pairs)
    rows = [p[0] for p in pairs]
    k9 = c.hip.eval_codons_batch(c.family, *c.args(rows), want=("windows", "genes"))
    Q = np.stack([lp.codon_table(c.state_space, k9["windows"][i], k9["genes"][i], lay) for i in range(n)])
    rng = np.random.default_rng(4)
    for node in NODES:
        ev, paths = c.node_codons(pairs, node)
        codons, change = c.given(pairs, node, Q)
        # the evaluation's own expanded K9 table: the evaluation form's bits
        assert np.array_equal(codons, ev["codons"]) and np.array_equal(change, ev["change"])
        cond, _ = c.probs(pairs, node, np.full((1, c.L), apo.OPEN), want=("cond",))
        G = cond["cond"]
        # one-hot Q: the product of three rows of cond
        b = rng.integers(0, 5, size=(n, nc, 3))
        hot = np.zeros((n, nc, 125))
        np.put_along_axis(hot, (25 * b[..., 0] + 5 * b[..., 1] + b[..., 2])[..., None], 1.0, axis=-1)
        codons, change = c.given(pairs, node, hot)
        s = 1 + 3 * np.arange(nc)
        g = [np.take_along_axis(G[:, s + k], b[..., k][..., None, None], axis=2)[:, :, 0] for k in range(3)]
        want = np.einsum("ncx,ncy,ncz->ncxyz", g[0], g[1], g[2]).reshape(n, nc, 64)
        rel = np.abs(codons - want) / np.where(want > 0, want, 1.0)
        print("one-hot: worst relative difference %.3g" % rel.max())
        assert rel.max() < 1e-15 and not codons[want == 0].any()
        has_n = (b == 4).any(axis=-1)
        assert (change[..., 3] == has_n).all()
        # a Dirichlet Q against the oracle's contraction on the device's own cond
        dq = rng.dirichlet(np.ones(125) * 0.05, size=(n, nc))
        dq[dq < 1e-3] = 0.0
        dq /= dq.sum(axis=-1, keepdims=True)
        codons, change = c.given(pairs, node, dq)
        worst = max(max(np.abs(codons[i] - nco.contraction(dq[i], G[i], 1)).max(),
                        np.abs(change[i] - nco.change(dq[i], G[i], 1)).max()) for i in range(n))
        print("Dirichlet: worst difference %.3g" % worst)
        assert worst < 1e-12
        # all mass on NNN
        nnn = np.zeros((n, nc, 125))
        nnn[..., 124] = 1.0
        codons, change = c.given(pairs, node, nnn)
        assert (change[..., 3] == 1.0).all() and not change[..., :3].any()
        assert np.abs(codons.sum(axis=-1) - 1).max() < 1e-12


# ---- batching ----

@pytest.fixture(scope="module")
def small(hip, tmp_path_factory):
    c = synth(hip, tmp_path_factory.mktemp("nodec"), n_samples=5, seed=45)
    c.set_frame(0)
    return c


def test_rows_do_not_depend_on_their_batch(small):
    c = small
    pairs = [(i, t) for i in range(3) for t in (1, 6)]
    for node in NODES:
        full, _ = c.node_codons(pairs, node)
        again, _ = c.node_codons(pairs, node)
        for i, p in enumerate(pairs):
            alone, _ = c.node_codons([p], node)
            second, _ = c.node_codons([pairs[(i + 1) % len(pairs)], p], node)
            for key in ("loglik", "codons", "change"):
                assert np.array_equal(alone[key][0], full[key][i]) and np.array_equal(second[key][1], full[key][i]), key
                assert np.array_equal(again[key], full[key])
    print("largest deviation 0 (bit-identical)")


def _worker(mode, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "node_codons_worker.py"), mode], capture_output=True,
                       text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_across_the_launch_group_cut():
    res = _worker("chunk", {"LH_CHUNK": "256"})
    print(res)
    assert res["n"] == 259 and res["groups"] == 2 and res["finite"]
    assert res["rows_checked"] == [0, 255, 256, 258]
    assert res["mismatches"] == []


def test_weighted_sums(small):
    """n = 256 + 1 rows (one past a slab of the reduction), random log_offset: the weighted sums within n 2^-52 relative of
    a long-double host sum of the returned rows, bit-stable over two calls, and two half batches combined by
    posterior.combine within 1e-14 of the whole."""
    c = small
    n = 257
    rng = np.random.default_rng(12)
    pairs = [(i % 5, 1 + (i * 3) % (c.T - 1)) for i in range(n)]
    off = -1000.0 + 3.0 * rng.standard_normal(n)
    want = ("loglik", "codons", "change", "weighted_codons", "weighted_change", "weight_stats")
    res, _ = c.node_codons(pairs, PARENT, log_offset=off, want=want)
    again, _ = c.node_codons(pairs, PARENT, log_offset=off, want=want)
    for k in ("weighted_codons", "weighted_change", "weight_stats"):
        assert np.array_equal(res[k], again[k]), k
    lw = res["loglik"] - off
    m = lw.max()
    w = np.exp(lw - m)
    st = res["weight_stats"]
    assert st[0] == m and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    h1 = 128
    a, _ = c.node_codons(pairs[:h1], PARENT, log_offset=off[:h1], want=want)
    b, _ = c.node_codons(pairs[h1:], PARENT, log_offset=off[h1:], want=want)
    worst = 0.0
    for k in ("codons", "change"):
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
    pairs = [(i, t) for i in range(2) for t in (1, c.T - 1)]
    a, _ = c.node_codons(pairs, MRCA)
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    b, _ = c.node_codons(pairs, MRCA)
    worst = max(np.abs(a[k] - b[k]).max() for k in ("codons", "change"))
    print("largest deviation %.3g" % worst)
    assert np.isfinite(a["codons"]).all() and np.isfinite(a["change"]).all() and worst < BOUND
    assert np.allclose(a["loglik"], b["loglik"], rtol=1e-12)


def test_extended_range_overflow_row(hip, tmp_path):
    """configs[4] (500 leaves x 600 sites), as tests/test_gpu_ancestral.py's case: on a tree sample whose default-mode
    log-likelihood overflows the default mode gives NaN, the extended-range mode finite tables that sum to 1 and whose site
    marginals equal K11's device output at 1e-12."""
    from linearham_amd import host
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec(n_leaves=500, n_sites=600, n_samples=64), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = hh.flatten_tsv(tsv, 64)
    fam = fl["family"]
    tree_args = lambda sl: (fl["n_tips"], fl["max_depth"], fl["ops"][sl], fl["brlen"][sl], fl["er"][sl], fl["pi"][sl],
                            fl["alpha"][sl], 4)
    default = hip.eval_posterior_batch(fam, *tree_args(slice(0, 64)), want=("loglik",))
    bad = [i for i in range(64) if not np.isfinite(default["loglik"][i])]
    assert bad, "no overflow row in the first 64 samples"
    i = bad[0]
    from oracle import linearham_oracle as orc
    labels = list(orc.PhyloHMM(yaml_path, 0, pdir, 0).xmsa_labels)
    children, root, _ = host.newick_arrays(sf.read_trees_tsv(tsv)[i]["tree"], labels)
    path = capi.seed_path(len(labels), children, root, 1)
    sl = slice(i, i + 1)
    frame = 2
    nc = hip.set_codons(fam, frame)["n_codons"]
    nan = hip.eval_node_codons_batch(fam, *tree_args(sl), [path], MRCA, want=("codons", "change"))
    assert np.isnan(nan["codons"]).all() and np.isnan(nan["change"]).all()
    hip.check(hip.lib.lh_family_set_extended_range(fam, 1))
    ext = hip.eval_node_codons_batch(fam, *tree_args(sl), [path], MRCA, want=("loglik", "codons", "change"))
    k11 = hip.eval_ancestral_batch(fam, *tree_args(sl), [path], want=("marg",))
    assert np.isfinite(ext["loglik"][0]) and np.isfinite(ext["codons"]).all() and np.isfinite(ext["change"]).all()
    m = nco.site_marginals(ext["codons"][0]).reshape(-1, 4)
    worst = np.abs(m - k11["marg"][0, len(path) - 1, frame:frame + 3 * nc]).max()
    print("site marginals against K11: %.3g" % worst)
    assert worst < 1e-12
    assert np.abs(ext["codons"].sum(axis=-1) - 1).max() < 1e-12 and np.abs(ext["change"].sum(axis=-1) - 1).max() < 1e-12


# ---- the _device form, refusals, the output bound ----

def test_device_entry_point_on_a_torch_stream():
    """The _device form on a stream of torch's (its own process): equal to the host-pointer form; a rejected
    device-resident schedule, a path that is not a chain and a path whose last entry is not the root each give that row
    NaN and no weight and raise the handle's error word once, the other rows keep their bits."""
    res = _worker("device")
    print(res)
    assert res["clean_status"] == "" and res["clean_equals_host"]
    for k in ("schedule", "not_a_chain", "not_the_root"):
        assert res[k]["victim_all_nan"] and res[k]["others_unchanged"] and res[k]["weights_leave_the_victim_out"], k
        assert res[k]["second_status"] == "", k
    assert "malformed schedule" in res["schedule"]["status"]
    assert "not a chain" in res["not_a_chain"]["status"] and "not a chain" in res["not_the_root"]["status"]


def test_refusals(hip, tmp_path):
    import ctypes as C
    c = synth(hip, tmp_path, n_samples=1, seed=37)
    pairs = [(0, 1)]
    with pytest.raises(RuntimeError, match="lh_family_set_codons has not been called"):
        c.node_codons(pairs, MRCA)
    # lh_eval_node_codons_batch itself (not the wrapper, which asks lh_codon_layout first)
    T, depth, ops, brl, er, pi, alpha, R = c.args([0])
    path = capi.pad_paths([c.path(0, 1)])
    ll = np.zeros(1)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    outs = capi._NodeCodonsOutputs(None, ll.ctypes.data_as(f64), None, None, None, None, None)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (brl, er, pi, alpha)]
    ops32 = np.ascontiguousarray(ops, dtype=np.int32)
    raw = lambda node: hip.lib.lh_eval_node_codons_batch(c.family, 1, T, depth, ops32.ctypes.data_as(i32),
                                                         *[a.ctypes.data_as(f64) for a in arrs], R,
                                                         path.ctypes.data_as(i32), path.shape[1], node, C.byref(outs))
    assert raw(MRCA) != 0 and hip.error() == "lh_eval_node_codons_batch: lh_family_set_codons has not been called"
    c.set_frame(0)
    assert raw(MRCA) == 0 and np.isfinite(ll[0])
    assert raw(2) != 0 and "node must be 0" in hip.error()
    with pytest.raises(RuntimeError, match="node must be 0"):
        c.node_codons(pairs, 2)
    p = c.path(0, 1)
    assert len(p) >= 2
    with pytest.raises(RuntimeError, match="is not a chain"):
        hip.eval_node_codons_batch(c.family, *c.args([0]), [p[::-1]], MRCA)
    with pytest.raises(RuntimeError, match="null array"):
        hip.check(hip.lib.lh_asr_node_codons_batch(c.family, 1, T, depth, ops32.ctypes.data_as(i32),
                                                   *[a.ctypes.data_as(f64) for a in arrs], R, None,
                                                   path.ctypes.data_as(i32), path.shape[1], MRCA, None, None))
    # no candidates are needed, and the extended-range mode is honoured
    assert hip.ancestral_candidates_info(c.family)[0] == 0
    capi.Family.borrow(c.family, hip).set_extended_range(True)
    res, _ = c.node_codons(pairs, MRCA)
    assert np.isfinite(res["codons"]).all()


def test_refused_without_an_msa_or_a_frame(hip, data_dir):
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    h = orc.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    desc = db.build_family_desc(h)
    desc.msa = np.zeros(0, dtype=np.uint8)          # no alignment: a forward-only family
    fam = linearham_amd.Family(desc, hip)
    with pytest.raises(RuntimeError, match="lh_family_set_sampler has not been called|without an MSA"):
        hip.set_codons(fam, 0)
    fam.close()


def test_output_bound_names_the_largest_n():
    """The refusal of the host-pointer form, through its hook (LH_ANC_OUT_MB=1, read once per process)."""
    res = _worker("bound", {"LH_ANC_OUT_MB": "1"})
    print(res)
    assert res["most"] > 8
    assert "batch too large" in res["message"] and "at most %d samples per call" % res["most"] in res["message"]
    assert res["largest_passes"]


# ---- what the probabilities are probabilities of ----

def test_tables_against_device_draws(hip, data_dir, tmp_path):
    """20 000 draws of the device on one toy row through lh_eval_lineage_batch (the chain: naive states from the posterior,
    their sequences, one ancestral draw under each), the row and the std::mt19937 words set up as
    tests/test_gpu_ancestral_probs.py's test_two_site_tables_against_device_draws sets them up; the nodes' bases read back
    with lh_lineage_rows_read.  The triple frequencies at two junction codons and the class frequencies at every codon, at
    both nodes, within 5 sigma + 1/N."""
    from oracle import linearham_oracle as orc
    c = toy_case(hip, data_dir, tmp_path)
    row, tip, N, frame = 1, 1, 20000, 0
    path = c.path(row, tip)
    assert len(path) == 2
    lay = c.set_frame(frame)
    nc = lay["n_codons"]
    junction = lay["window_codon"][:2]
    assert len(junction) == 2
    T, depth, ops, brl, er, pi, alpha, R = c.args([row])
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a), N, axis=0))
    fam = capi.Family.borrow(c.family, hip)
    nw = hip.lib.lh_sample_words(c.family)
    rng = orc.MT19937(5)
    words = np.array([rng() for _ in range(N * nw)], dtype=np.uint32).reshape(N, nw)
    P = len(path)
    chain = fam.eval_lineage_batch(T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(alpha), R, words, 23,
                                   rep(capi.pad_paths([path])))
    assert np.isfinite(chain["loglik"]).all()
    naive = chain["naive"]
    flat = (np.arange(N) * (P + 1))[:, None] + np.array([0, P - 1])[None, :]      # slot 0: the parent, the last: the MRCA
    node_seqs = fam.lineage_rows_read(flat.reshape(-1), c.L).reshape(N, 2, c.L)
    cls = lp.change_classes()
    sl = [slice(frame + k, frame + 3 * nc, 3) for k in range(3)]
    naive = naive.astype(np.int64)
    b = 25 * naive[:, sl[0]] + 5 * naive[:, sl[1]] + naive[:, sl[2]]
    worst = 0.0
    for node in NODES:
        res, _ = c.node_codons([(row, tip)], node)
        seqs = node_seqs[:, node].astype(np.int64)
        x = 16 * seqs[:, sl[0]] + 4 * seqs[:, sl[1]] + seqs[:, sl[2]]
        for k in junction:
            p = res["codons"][0, k]
            freq = np.bincount(x[:, k], minlength=64) / N
            worst = max(worst, np.abs(freq - p).max())
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (node, k)
        kk = cls[b, x]
        for k in range(nc):
            p = np.clip(res["change"][0, k], 0.0, 1.0)
            freq = np.bincount(kk[:, k], minlength=4) / N
            worst = max(worst, np.abs(freq - p).max())
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N).all(), (node, k)
    print("largest deviation of a frequency %.3g" % worst)


# ---- the host library: PhyloHMM::NodeCodonMarginals, the pipeline over a RevBayes table, the CLI ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _check_files(res, per_row, first, frame, node_name):
    used = per_row[first:]
    lw = np.array([r[0] for r in used])
    w = np.exp(lw - lw.max())
    codons = sum(wi * r[1] for wi, r in zip(w, used)) / w.sum()
    change = sum(wi * r[2] for wi, r in zip(w, used)) / w.sum()
    worst = max(np.abs(res["codons"] - codons).max(), np.abs(res["change"] - change).max())
    print("pipeline: worst difference from the oracle's weighted tables %.3g" % worst)
    assert worst < BOUND
    want_aa = lp.node_aa_table(codons)
    for c, d in enumerate(res["aa"]):
        assert max(abs(d.get(a, 0.0) - want_aa[c].get(a, 0.0)) for a in set(d) | set(want_aa[c])) < BOUND
    assert [r[0] for r in res["rows"]] == list(range(first, 9))
    assert np.allclose([r[1] for r in res["rows"]], w, rtol=1e-9)
    assert [r[2] for r in res["rows"]] == [r[3] for r in used]
    sm = res["summary"]
    assert sm["rows_used"] == 9 - first and sm["rows_skipped_nonfinite"] == 0 and sm["frame"] == frame and sm["node"] == node_name
    assert abs(sm["kish_ess"] - w.sum() ** 2 / (w * w).sum()) < 1e-9 * sm["kish_ess"]
    assert abs(sm["expected_synonymous"] - res["change"][:, 1].sum()) < 1e-12
    assert abs(sm["expected_replacement"] - res["change"][:, 2].sum()) < 1e-12


def test_pipeline_and_cli(hip, tmp_path):
    """PhyloHMM::RunNodeCodonsPipeline on a 9-row table, through the library (burn-in 0.25) and through `linearham
    --node-codons-pipeline` (no burn-in; with LH_PIPELINE_BATCH 2 and 4: byte-identical files), against the oracle's per-row
    tables weighted by exp(LHLogLikelihood - Likelihood); then PhyloHMM::NodeCodonMarginals and `linearham --node-codons`
    on the first row's tree, at the other node."""
    from linearham_amd import host
    from tests.node_codons_cases import NodeCodonsCase
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(n_samples=9, seed=41), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = NodeCodonsCase(hip, yaml_path, pdir, rows, 4, tmp_path)
    tip, frame = 3, 1
    seed_seq = list(c.o.xmsa_labels)[tip]
    c.frame = frame
    per_row = []
    for i in range(9):
        path = c.path(i, tip)
        Q = c.naive_codons(i)
        ll = c.o.log_likelihood()
        T, ch = c.oracle_node(Q, i, path, MRCA)
        per_row.append((ll - rows[i]["likelihood"], T, ch, len(path)))
    _check_files(c.hh.run_node_codons_pipeline(tsv, seed_seq, "mrca", str(tmp_path / "lib"), 4, burnin_frac=0.25, frame=frame),
                 per_row, 2, frame, "mrca")
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq,
              "--frame", str(frame)]
    names = (("cli", {}), ("cli2", {"LH_PIPELINE_BATCH": "2"}), ("cli4", {"LH_PIPELINE_BATCH": "4"}))
    for name, env in names:
        r = subprocess.run([_exe(), "--node-codons-pipeline", "--input-path", tsv, "--output-path", str(tmp_path / name),
                            "--node", "mrca"] + common, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr
    _check_files(host.read_node_codons(str(tmp_path / "cli")), per_row, 0, frame, "mrca")
    for f in ("codons.tsv", "aa.tsv", "changes.tsv", "rows.tsv", "summary.tsv"):
        whole = open(str(tmp_path / "cli") + "." + f, "rb").read()
        for name, _ in names[1:]:
            assert open(str(tmp_path / name) + "." + f, "rb").read() == whole, (name, f)
    # one tree, the other node
    row = c.rows[0]
    path = c.path(0, tip)
    Q = c.naive_codons(0)
    ll = c.o.log_likelihood()
    T, ch = c.oracle_node(Q, 0, path, PARENT)
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one = c.hh.node_codon_marginals(seed_seq, "parent", frame)
    assert one["node"] == path[0] and abs(one["loglik"] - ll) < 1e-9 * abs(ll)
    worst = max(np.abs(one["codons"] - T).max(), np.abs(one["change"] - ch).max())
    newick = str(tmp_path / "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    args = [_exe(), "--node-codons", "--newick-path", newick, "--alpha", repr(row["alpha"]), "--node", "parent"] + common
    args += sum([["--er", repr(x)] for x in row["er"]], []) + sum([["--pi", repr(x)] for x in row["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = host.parse_node_codons(r.stdout)
    assert np.array_equal(got["codons"], one["codons"]) and np.array_equal(got["change"], one["change"])
    print("one tree: worst difference from the oracle %.3g" % worst)
    assert worst < BOUND
