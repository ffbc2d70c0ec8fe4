"""K5 (exact naive-sequence posterior marginals) on the device against tests/posterior_oracle.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import host
from linearham_amd import posterior as lp
from oracle import linearham_oracle as orc
from tests import posterior_oracle as po

pytestmark = pytest.mark.gpu

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
BOUND = 1e-10


def _pair(yaml_path, pdir, tree, er, pi, alpha, R, is_path):
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    h.initialize_phylo_parameters(tree, er, pi, alpha, R, is_path=is_path)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    o.initialize_phylo_parameters(tree, er, pi, alpha, R, is_path=is_path)
    o.initialize_phylo_emission()
    o.log_likelihood()
    return h, o


def _golden(case):
    meta = GOLD["PhyloHMM:" + case]["meta"]
    return _pair(os.path.join(D, case + ".yaml"), os.path.join(D, "hmm_params"), os.path.join(D, "newton.tree"),
                 meta["er"], meta["pi"], meta["alpha"], meta["num_rates"], True)


def _synthetic(tmp_path, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(**kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    r = sf.read_trees_tsv(tsv)[0]
    return _pair(yaml_path, pdir, r["tree"], r["er"], r["pi"], r["alpha"], 4, False), (yaml_path, pdir, tsv)


def _check(h, o):
    post, ll = h.naive_posterior()
    assert abs(ll - o.log_likelihood()) < 1e-9 * abs(ll)
    want = po.to_compact(o, po.smoothing(o))
    assert post.shape == want.shape
    err = np.max(np.abs(post - want))
    assert err < BOUND, err
    # dense, state by state
    ss = h.dump(1)
    dense = lp.dense_posteriors(ss, post)
    for region, p in po.smoothing(o).items():
        assert np.max(np.abs(dense[region] - p)) < BOUND, region
    # site marginals and gene posteriors through the host
    sb, genes = h.naive_marginals()
    assert np.max(np.abs(sb - po.site_base(o, po.smoothing(o)))) < BOUND
    assert np.allclose(sb.sum(axis=1), 1.0, atol=1e-12)
    og = po.gene_posteriors(o, po.smoothing(o))
    assert set(genes) == set(og)
    for reg in og:
        assert set(genes[reg]) == set(og[reg])
        for g in og[reg]:
            assert abs(genes[reg][g] - og[reg][g]) < BOUND, (reg, g)
    return post


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_golden_families(case):
    h, o = _golden(case)
    _check(h, o)


@pytest.mark.parametrize("locus,kw", [("igh", {}), ("igk", {}), ("igl", {}), ("igh", dict(ragged=4, ambiguous=0.02)),
                                      ("igh", dict(n_v=300, n_d=70, n_j=5)), ("igk", dict(n_v=150, n_j=70)),
                                      ("igh", dict(n_d=65, n_j=30))])
def test_synthetic_families(tmp_path, locus, kw):
    (h, o), _ = _synthetic(tmp_path, locus=locus, n_samples=2, **kw)
    _check(h, o)


def test_extended_range_equals_default(tmp_path):
    (h, o), _ = _synthetic(tmp_path, locus="igh", n_samples=2)
    a, _ = h.naive_posterior()
    h.set_extended_range(True)
    b, _ = h.naive_posterior()
    assert np.all(np.isfinite(a))
    assert np.max(np.abs(a - b)) < 1e-12


def test_batches_and_weight_stats(tmp_path):
    (h, o), (yaml_path, pdir, tsv) = _synthetic(tmp_path, locus="igh", n_samples=300)
    from linearham_amd.capi import load_library
    hip = load_library()
    fl = h.flatten_tsv(tsv, 300)
    from tools import synth_family as sf
    rb = np.array([r["likelihood"] for r in sf.read_trees_tsv(tsv)])

    def run(sl):
        return hip.eval_posterior_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"][sl], fl["brlen"][sl],
                                        fl["er"][sl], fl["pi"][sl], fl["alpha"][sl], 4, log_offset=rb[sl])
    full = run(slice(0, 300))
    lw = full["loglik"] - rb
    m = lw.max()
    w = np.exp(lw - m)
    st = full["weight_stats"]
    assert st[0] == m
    assert abs(st[1] - w.sum()) < 1e-13 * w.sum()
    assert abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    ref = w @ full["posterior"]
    assert np.allclose(full["weighted_sum"], ref, rtol=1e-12, atol=1e-300)
    # every row's posterior against the oracle (first rows)
    for i, r in enumerate(sf.read_trees_tsv(tsv)[:3]):
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        assert np.max(np.abs(full["posterior"][i] - po.to_compact(o, po.smoothing(o)))) < BOUND
    # 100 + 200 combined on the host == one batch of 300
    a, b = run(slice(0, 100)), run(slice(100, 300))
    mean, mx, s1, s2 = lp.combine([(a["weighted_sum"], a["weight_stats"]), (b["weighted_sum"], b["weight_stats"])])
    one = full["weighted_sum"] / st[1]
    assert np.allclose(mean, one, rtol=1e-14, atol=1e-300)
    assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]


def _oracle_rows(o, rows):
    lls, sites, genes = [], [], []
    for r in rows:
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        lls.append(o.log_likelihood())
        dense = po.smoothing(o)
        sites.append(po.site_base(o, dense))
        g = po.gene_posteriors(o, dense)
        genes.append(np.array([g[reg][name] for reg in sorted(g) for name in sorted(g[reg])]))
    return np.array(lls), np.array(sites), np.array(genes), g


def _check_aggregate(sb, genes, summary, prefix, want_sb, want_genes, keys, ess, n_used):
    assert np.max(np.abs(sb - want_sb)) < BOUND
    got = np.array([genes[reg][name] for reg, name in keys])
    assert np.max(np.abs(got - want_genes)) < BOUND
    assert summary["rows_used"] == n_used and summary["rows_skipped_nonfinite"] == 0
    assert abs(summary["kish_ess"] - ess) < 1e-9 * ess
    lines = open(prefix + ".sites.tsv").read().split("\n")
    assert lines[0] == "site\tA\tC\tG\tT\tN\tmap_base"
    for ln in lines[1:-1]:
        f = ln.split("\t")
        p = [float(x) for x in f[1:6]]
        assert abs(sum(p) - 1.0) < 1e-12
        assert f[6] == lp.BASES[int(np.argmax(p))]
    g = [ln.split("\t") for ln in open(prefix + ".genes.tsv").read().strip().split("\n")]
    assert g[0] == ["region", "gene", "probability"]
    probs = [float(x[2]) for x in g[1:]]
    assert probs == sorted(probs, reverse=True)  # sorted by probability


@pytest.mark.parametrize("via", ["library", "cli"])
def test_marginals_pipeline(tmp_path, via):
    """PhyloHMM::RunMarginalsPipeline (library call and `linearham --marginals-pipeline`), with and without burn-in,
    against the oracle's per-row posteriors aggregated by the R script's rules (tests/posterior_oracle.py)."""
    (h, o), (yaml_path, pdir, tsv) = _synthetic(tmp_path, locus="igh", n_samples=40)
    from tools import synth_family as sf
    rows = sf.read_trees_tsv(tsv)
    lls, sites, genes, g = _oracle_rows(o, rows)
    keys = [(reg, name) for reg in sorted(g) for name in sorted(g[reg])]
    rb = np.array([r["likelihood"] for r in rows])
    for b in (0.0, 0.25):
        prefix = str(tmp_path / ("m%d" % int(100 * b)))
        if via == "library":
            sb, gn, summary = h.run_marginals_pipeline(tsv, prefix, 4, burnin_frac=b)
        else:
            r = subprocess.run([_exe(), "--marginals-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0",
                                "--hmm-param-dir", pdir, "--input-path", tsv, "--output-path", prefix, "--num-rates", "4",
                                "--burnin-frac", str(b)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            sb, gn, summary = host.read_marginals(prefix)
        want_sb, ess = po.weighted_marginals(lls, rb, sites, b)
        want_genes, _ = po.weighted_marginals(lls, rb, genes, b)
        _check_aggregate(sb, gn, summary, prefix, want_sb, want_genes, keys, ess,
                         len(rows) - int(math.floor(b * len(rows))))


def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def test_cli_marginals_golden():
    """`linearham --marginals` (the arguments of --compute-logl) on the golden family: the site and gene tables equal
    posterior_oracle's."""
    case = "phylo_hmm_input"
    meta = GOLD["PhyloHMM:" + case]["meta"]
    h, o = _golden(case)
    args = [_exe(), "--marginals", "--yaml-path", os.path.join(D, case + ".yaml"), "--cluster-ind", "0",
            "--hmm-param-dir", os.path.join(D, "hmm_params"), "--newick-path", os.path.join(D, "newton.tree"),
            "--num-rates", str(meta["num_rates"]), "--alpha", repr(meta["alpha"])]
    args += sum([["--er", repr(x)] for x in meta["er"]], []) + sum([["--pi", repr(x)] for x in meta["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    site_part, gene_part = r.stdout.split("\n\n")
    lines = site_part.strip().split("\n")
    assert lines[0] == "site\tA\tC\tG\tT\tN\tmap_base"
    sb = np.array([[float(x) for x in ln.split("\t")[1:6]] for ln in lines[1:]])
    dense = po.smoothing(o)
    assert np.max(np.abs(sb - po.site_base(o, dense))) < BOUND
    og = po.gene_posteriors(o, dense)
    got = {}
    for ln in gene_part.strip().split("\n")[1:]:
        reg, name, p = ln.split("\t")
        got.setdefault(reg, {})[name] = float(p)
    assert set(got) == set(og)
    for reg in og:
        for name in og[reg]:
            assert abs(got[reg][name] - og[reg][name]) < BOUND
    # more than one device is refused by the marginals pipeline
    r = subprocess.run([_exe(), "--marginals-pipeline", "--yaml-path", os.path.join(D, case + ".yaml"), "--cluster-ind",
                        "0", "--hmm-param-dir", os.path.join(D, "hmm_params"), "--input-path", "x", "--output-path", "y",
                        "--devices", "0,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr


def test_malformed_device_schedule():
    """lh_eval_posterior_batch_device with one sample's DEVICE-RESIDENT schedule corrupted (a tip number far outside
    the alignment, as tests/device_schedule_worker.py builds it; in its own process, tests/posterior_schedule_worker.py):
    K0c rejects it on the device, the sample's posterior is NaN, the handle's error word is raised once, and
    weighted_sum / weight_stats are numpy's over the other rows."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "posterior_schedule_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["status"] != 0 and "malformed schedule" in res["message"], res
    assert res["second_status"] == 0  # reported once
    assert res["victim_all_nan"] and res["victim_loglik_nan"]
    assert res["others_equal_clean"]
    assert res["max_lw_equal"] and res["zeros_where_ref_zero"]
    assert res["sum_w_rel"] < 1e-14 and res["sum_w2_rel"] < 1e-14
    assert res["weighted_sum_rel"] < 1e-13


def test_k4_draws_match_k5(tmp_path):
    """K4 (lh_eval_sample_batch) draws one tree 20 000 times with distinct engine-word slices; the frequency of every
    state at every junction row and of every gene of every region agrees with K5's posterior within 5 sigma."""
    import ctypes as C
    from linearham_amd.capi import load_library
    (h, o), (yaml_path, pdir, tsv) = _synthetic(tmp_path, locus="igh", n_samples=2)
    hip = load_library()
    fl = h.flatten_tsv(tsv, 1)
    fam = C.c_void_p(fl["family"])
    lib = hip.lib
    lib.lh_sample_words.argtypes = [C.c_void_p]
    lib.lh_sample_states.argtypes = [C.c_void_p]
    nw, ns = lib.lh_sample_words(fam), lib.lh_sample_states(fam)
    n = 20000
    rep = lambda a: np.ascontiguousarray(np.repeat(a[:1], n, axis=0))
    ops, brlen, er, pi, alpha = (rep(fl[k]) for k in ("ops", "brlen", "er", "pi", "alpha"))
    words = np.random.default_rng(11).integers(0, 1 << 32, size=(n, nw), dtype=np.uint64).astype(np.uint32)
    ll, states = np.zeros(n), np.zeros((n, ns), dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    hip.check(lib.lh_eval_sample_batch(fam, n, fl["n_tips"], fl["max_depth"], p(ops, C.c_int32), p(brlen, C.c_double),
                                       p(er, C.c_double), p(pi, C.c_double), p(alpha, C.c_double), 4,
                                       p(words, C.c_uint32), p(ll, C.c_double), None, p(states, C.c_int32)))
    res = hip.eval_posterior_batch(fam, fl["n_tips"], fl["max_depth"], fl["ops"][:1], fl["brlen"][:1], fl["er"][:1],
                                   fl["pi"][:1], fl["alpha"][:1], 4)
    dense = lp.dense_posteriors(h.dump(1), res["posterior"][0])
    W_dj, W_vd = dense["dj_junction"].shape[0], dense["vd_junction"].shape[0]
    # states: J gene | D-J rows | D gene | V-D rows | V gene
    cols = [("jgerm", None)] + [("dj_junction", i) for i in range(W_dj)] + [("dgerm", None)] + \
        [("vd_junction", i) for i in range(W_vd)] + [("vgerm", None)]
    assert len(cols) == ns
    for c, (region, row) in enumerate(cols):
        want = dense[region] if row is None else dense[region][row]
        freq = np.bincount(states[:, c], minlength=len(want)) / n
        sigma = np.sqrt(np.maximum(want * (1 - want), 1.0 / n) / n)
        assert np.all(np.abs(freq - want) <= 5 * sigma), (region, row, np.max(np.abs(freq - want) / sigma))


def test_config2_first_16_samples(tmp_path):
    """The full configs[2] family, first 16 tree samples: K5 against posterior_oracle's smoothing of the dense forward
    arrays of the C oracle (oracle_c.eval_forward) with the numpy oracle's dense transitions."""
    from oracle import oracle_c
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec(n_samples=16), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = h.flatten_tsv(tsv, 16)
    from linearham_amd.capi import load_library
    res = load_library().eval_posterior_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"],
                                              fl["er"], fl["pi"], fl["alpha"], 4)
    rows = sf.read_trees_tsv(tsv)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    labels = list(o.xmsa_labels)
    trees = [host.newick_arrays(r["tree"], labels) for r in rows]
    oracle_c.build()
    cf = oracle_c.COracleFamily(o, 4)
    fwds = cf.eval_forward(trees, [r["er"] for r in rows], [r["pi"] for r in rows], [r["alpha"] for r in rows],
                           n_threads=min(16, len(os.sched_getaffinity(0))))
    for i in range(16):
        assert np.isfinite(fwds[i]["loglik"])
        want = po.to_compact(o, po.smoothing(o, forward=fwds[i]))
        assert np.max(np.abs(res["posterior"][i] - want)) < BOUND, i


def test_extended_range_overflow_row(tmp_path):
    """configs[4]: on a tree sample whose default-mode log-likelihood overflows (found as test_config4_full_size_family
    finds them), extended-range K5 is finite and normalised, and equals posterior_oracle's smoothing of the device's OWN
    extended-range forward arrays (lh_eval_batch with outs.forward)."""
    import ctypes as C
    from linearham_amd.capi import _EvalOutputs, load_library
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec(n_leaves=500, n_sites=600, n_samples=64), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = h.flatten_tsv(tsv, 64)
    hip = load_library()
    fam = C.c_void_p(fl["family"])
    args = (fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"], fl["er"], fl["pi"], fl["alpha"], 4)
    default = hip.eval_posterior_batch(fam, *args)
    bad = [i for i in range(64) if not np.isfinite(default["loglik"][i])]
    assert bad, "no overflow row in the first 64 samples"
    assert all(np.all(np.isnan(default["posterior"][i])) for i in bad)
    hip.check(hip.lib.lh_family_set_extended_range(fam, 1))
    ext = hip.eval_posterior_batch(fam, *args)
    ok = [i for i in range(64) if np.isfinite(default["loglik"][i])]
    assert np.max(np.abs(ext["posterior"][ok] - default["posterior"][ok])) < 1e-12
    i = bad[0]
    post = ext["posterior"][i]
    assert np.isfinite(ext["loglik"][i]) and np.all(np.isfinite(post))
    ss = h.dump(1)
    dense = lp.dense_posteriors(ss, post)
    for region, p in dense.items():
        assert np.allclose(np.atleast_2d(p).sum(axis=1), 1.0, atol=1e-12), region
    # the device's own extended-range forward arrays of that sample, smoothed by the oracle
    FS = hip.lib.lh_forward_size(fam)
    fwd, ll = np.zeros(FS), np.zeros(1)
    outs = _EvalOutputs()
    outs.forward = fwd.ctypes.data_as(C.POINTER(C.c_double))
    pp = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    sel = {k: np.ascontiguousarray(fl[k][i:i + 1]) for k in ("ops", "brlen", "er", "pi", "alpha")}
    hip.check(hip.lib.lh_eval_batch(fam, 1, fl["n_tips"], fl["max_depth"], pp(sel["ops"], C.c_int32),
                                    pp(sel["brlen"], C.c_double), pp(sel["er"], C.c_double), pp(sel["pi"], C.c_double),
                                    pp(sel["alpha"], C.c_double), 4, pp(ll, C.c_double), C.byref(outs)))
    fd = lp.dense_posteriors(ss, fwd)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    want = po.smoothing(o, forward={k + "_forward": v for k, v in fd.items()})
    for region in want:
        assert np.max(np.abs(dense[region] - want[region])) < BOUND, region


CRAFTED = ("toy", "small_igh", "small_igk", "igh_70_33_5", "igh_v130_d30_j12", "igh_v260", "igh_d65", "igk_v70_j70")


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_emissions(tmp_path, name):
    """lh_posterior_forward_batch on the cases of tests/k2_scaling_cases.py, the rows of its batch_order, in both range modes
    (as test_gpu_events.py::test_crafted_emissions does for K10): scaling every column of a site by 2^-k changes no
    posterior, so every deep case's posterior equals its base's to 1e-12; base cases against posterior_oracle.smoothing on
    the same emissions; site marginals sum to 1; delta4 overflows the default mode (log-likelihood not finite, posterior
    NaN) and is finite and equal to its base in the extended-range mode; every row bit-equal alone, as row 1 of a call of
    two, and in the full call."""
    from linearham_amd.capi import load_library
    from tests import k2_scaling_cases as kc
    from tests import viterbi_cases as vc
    from tests import viterbi_oracle as vo
    hip = load_library()
    h = kc.load_family(name, tmp_path)
    _, cases = kc.build_cases(h, kc.SEEDS[name])
    by = {c.name: c for c in cases}
    want = {}
    for c in cases:
        if c.sum_k == 0:
            vo.set_emissions(h, c.em)
            h.cache_forward = True  # (new emissions: the forward arrays of the last vector are stale)
            assert np.isfinite(h.log_likelihood())
            want[c.name] = po.to_compact(h, po.smoothing(h))
    assert "base" in want and all(c.base in want for c in cases)
    order = kc.batch_order(cases)
    assert set(order) == set(by) and len(order) >= 17 and len(order) % 2 == 1
    em = np.stack([by[n].em for n in order])
    ss = po.state_space(h)
    lay = lp.layout(ss)
    fam = vc.device_family(hip, h)
    finite = {}
    for ext in (False, True):
        fam.set_extended_range(ext)
        ll, post = fam.posterior_forward_batch(em)
        assert post.shape == (len(order), fam.forward_size)
        first = {}
        for i, n in enumerate(order):
            j = first.setdefault(n, i)
            assert ll[i:i + 1].tobytes() + post[i].tobytes() == ll[j:j + 1].tobytes() + post[j].tobytes(), (n, i, j)
        for n, i in first.items():
            l1, p1 = fam.posterior_forward_batch(by[n].em[None])
            l2, p2 = fam.posterior_forward_batch(np.stack([by["base"].em, by[n].em]))
            mine = ll[i:i + 1].tobytes() + post[i].tobytes()
            assert l1.tobytes() + p1[0].tobytes() == mine, (n, ext, "alone")
            assert l2[1:2].tobytes() + p2[1].tobytes() == mine, (n, ext, "row 1 of a call of two")
            if by[n].expect == "overflow" and not ext:
                assert not np.isfinite(ll[i]) and np.all(np.isnan(post[i])), (n, ll[i])
                continue
            assert np.isfinite(ll[i]) and np.all(np.isfinite(post[i])), (n, ext)
            d_base = np.max(np.abs(post[i] - post[first[by[n].base]]))
            d_orc = np.max(np.abs(post[i] - want[by[n].base]))
            d_sum = np.max(np.abs(lp.site_base(ss, post[i], lay).sum(axis=1) - 1.0))
            print(name, "ext" if ext else "default", n, "vs base", d_base, "vs oracle", d_orc, "site sums", d_sum)
            assert d_base < 1e-12, (n, ext, d_base)
            assert d_orc < BOUND, (n, ext, d_orc)
            assert d_sum < 1e-12, (n, ext, d_sum)
        finite[ext] = {n: post[i] for n, i in first.items() if np.isfinite(ll[i])}
    assert set(finite[True]) == set(by) and len(finite[False]) >= len(by) - 1
    if "delta4" in by:
        assert "delta4" not in finite[False]
    for n in finite[False]:
        assert np.max(np.abs(finite[False][n] - finite[True][n])) < 1e-12, n
    fam.close()


def test_one_handle_through_every_entry_point():
    """One family handle, profiling on, through every batched entry point -- the evaluation, the forward sweep, K3 to K9,
    the lineages and the chain, and their _device forms -- in turn, neighbours sharing a buffer, for batch sizes that grow
    and then shrink: every result is bit-identical to the same call on a fresh handle, and every *_profile_read reports the
    launch groups of the call just made with a positive time, then zero (tests/handle_reuse_worker.py, its own process)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "handle_reuse_worker.py")], capture_output=True,
                       text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["calls"] == 110
    assert res["mismatches"] == []
    assert res["bad_profile"] == []
