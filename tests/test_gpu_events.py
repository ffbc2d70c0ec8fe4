"""K10 (exact posteriors of deletion and insertion lengths, lh_events.hip) on the device against tests/events_oracle.py.

Bound: 1e-10 against the dense oracle form, K5's and K9's bound for the same ratio chains.  The families are the shapes
at which the kernel can go wrong: one and two junctions, more right genes than the sixteen lanes of a group (33 D: three
rounds), 260 V, genes that stop before the junction's last row and genes without a germline state in the junction."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import events_oracle as eo
from tests import k2_scaling_cases as kc
from tests import viterbi_cases as vc
from tests import viterbi_oracle as vo
from tests.helpers import gene_entries

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUND = 1e-10  # K5's

FAMILIES = {
    "golden": None,
    "golden_extra": None,
    "small_igh": dict(locus="igh"),
    "small_igk": dict(locus="igk"),
    "small_igl": dict(locus="igl"),
    "ragged": dict(locus="igh", ragged=4, ambiguous=0.02),
    "igh_70_33": dict(locus="igh", n_v=70, n_d=33, n_j=5),
    "igh_v260": dict(locus="igh", n_v=260, n_d=3, n_j=3),
}


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def _rows(name, tmp_path, n_rows=2):
    if FAMILIES[name] is None:
        o, rows = vc.golden_rows("phylo_hmm_input" if name == "golden" else "phylo_hmm_input_extra")
        return o, rows
    o, rows, _ = vc.synthetic_rows(tmp_path, n_rows, **FAMILIES[name])
    return o, rows


def _eval(hip, fam, inp, sl=slice(None), **kw):
    return hip.eval_events_batch(fam, inp["n_tips"], inp["max_depth"], inp["ops"][sl], inp["brlen"][sl], inp["er"][sl],
                                 inp["pi"][sl], inp["alpha"][sl], inp["R"], **kw)


def _posterior(hip, fam, inp):
    return hip.eval_posterior_batch(fam, inp["n_tips"], inp["max_depth"], inp["ops"], inp["brlen"], inp["er"], inp["pi"],
                                    inp["alpha"], inp["R"], want=("loglik", "posterior"))


def _diff(x, y):
    return max(float(np.max(np.abs(a - b))) for jx, jy in zip(x, y) for a, b in zip(jx, jy))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_families(hip, tmp_path, name):
    from linearham_amd.capi import split_events
    o, rows = _rows(name, tmp_path)
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    lay = hip.events_layout(fam)
    S = [s for s in eo.sampler_tables(o) if s is not None]
    assert [(j["rows"], j["n_left"], j["n_right"]) for j in lay["junctions"]] == [(s.n_rows, s.n_left, s.n_right) for s in S]
    assert len(S) == (2 if o.locus == "igh" else 1)
    res = _eval(hip, fam, inp)
    post = _posterior(hip, fam, inp)
    assert res["events"].shape == (len(rows), lay["size"]) and res["genes"].shape == (len(rows), lay["n_genes"])
    seen = dict(a0=0.0, bW=0.0, ab=0.0)
    for i, r in enumerate(rows):
        vc.set_row(o, r)
        ll = o.log_likelihood()
        assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll)
        want = eo.dense(o)
        got = split_events(lay, res["events"][i])
        err = _diff(got, want)
        # exit and enter against K5's own device output through the difference identity
        mine = eo.structured(o, *eo.sampler_tables(o), P=post["posterior"][i])
        ident = max(float(np.max(np.abs(g[k] - m[k]))) for g, m in zip(got, mine) for k in (0, 1))
        print(name, "row", i, "max deviation from the dense oracle", err, "difference identity", ident)
        assert err < BOUND
        assert ident < 1e-12
        assert np.array_equal(res["genes"][i], gene_entries(lay, post["posterior"][i]))
        for ex, en, sp in got:
            W = sp.shape[0] - 1
            assert max(abs(ex.sum() - 1.0), abs(en.sum() - 1.0), abs(sp.sum() - 1.0)) < BOUND
            assert np.all(sp[np.tril_indices(W + 1, -1)] == 0.0)
            assert np.max(np.abs(sp.sum(axis=1) - ex.sum(axis=0))) < BOUND
            assert np.max(np.abs(sp.sum(axis=0) - en.sum(axis=0))) < BOUND
        for ex, en, sp in want:
            W = sp.shape[0] - 1
            seen["a0"] = max(seen["a0"], sp[0].sum())
            seen["bW"] = max(seen["bW"], sp[:, W].sum())
            seen["ab"] = max(seen["ab"], np.trace(sp))
    # conditions on the fixtures, asserted on the oracle: the edge cells carry weight, the ragged shapes exist
    if name == "golden_extra":
        assert min(seen.values()) > 0.1, seen
    if name in ("small_igk", "igh_70_33"):
        assert any((s.left_rows < s.n_rows).any() for s in S) and any((s.right_first == s.n_rows).any() for s in S)
    if name == "igh_70_33":
        assert S[0].n_right > 32  # three rounds of sixteen lanes, the last one partly empty
    fam.close()


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    work = tmp_path_factory.mktemp("events_crafted")
    cache = {}

    def get(name):
        if name not in cache:
            h = kc.load_family(name, work)
            _, cases = kc.build_cases(h, kc.SEEDS[name])
            refs = {}
            for c in cases:
                if c.sum_k == 0:
                    vo.set_emissions(h, c.em)
                    h.cache_forward = True  # (new emissions: the forward arrays of the last vector are stale)
                    h.log_likelihood()
                    refs[c.name] = eo.flat(eo.dense(h))
            cache[name] = (h, cases, refs)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(kc.family_specs()))
def test_crafted_emissions(hip, crafted, name):
    """lh_events_forward_batch on the cases of tests/k2_scaling_cases.py: scaling every column of a site by 2^-k changes no
    posterior, so every deep case's tables equal its base's to 1e-12, in both range modes; delta4 overflows the default
    mode (NaN) and is finite and equal in the extended-range mode."""
    h, cases, refs = crafted(name)
    names = [c.name for c in cases]
    by = {c.name: c for c in cases}
    assert "base" in names and all(c.base in refs for c in cases)
    em = np.stack([c.em for c in cases])
    fam = vc.device_family(hip, h)
    results = {}
    for ext in (False, True):
        fam.set_extended_range(ext)
        ll, ev = hip.events_forward_batch(fam, em)
        results[ext] = ev
        for i, n in enumerate(names):
            if n == "delta4" and not ext:
                assert not np.isfinite(ll[i]) and np.all(np.isnan(ev[i])), (n, ll[i])
                continue
            assert np.isfinite(ll[i]) and np.all(np.isfinite(ev[i])), (n, ext)
            base = ev[names.index(by[n].base)]
            d_base, d_orc = np.max(np.abs(ev[i] - base)), np.max(np.abs(ev[i] - refs[by[n].base]))
            print(name, "ext" if ext else "default", n, "vs base", d_base, "vs oracle", d_orc)
            assert d_base < 1e-12, (n, ext, d_base)
            assert d_orc < BOUND, (n, ext, d_orc)
    ok = np.all(np.isfinite(results[False]), axis=1)
    assert ok.sum() >= len(names) - 1
    assert np.max(np.abs(results[False][ok] - results[True][ok])) < 1e-12
    fam.close()


def test_rows_alone_and_in_batches(hip, tmp_path):
    """Every row carries the same bits alone, in calls of 5 and in the call of 23; only what is asked for comes back; the
    weighted sums of the 23-row call against numpy; two batches combine to the single call."""
    from linearham_amd import posterior as lp
    o, rows, _ = vc.synthetic_rows(tmp_path, 23, locus="igh", ragged=4, ambiguous=0.02)
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    rb = np.array([r["likelihood"] for r in rows])
    full = _eval(hip, fam, inp, log_offset=rb)
    assert np.all(np.isfinite(full["events"]))
    for n in (1, 5):
        for first in range(0, 23 - n + 1, n):
            sl = slice(first, first + n)
            part = _eval(hip, fam, inp, sl, want=("loglik", "events", "genes"))
            assert set(part) == {"loglik", "events", "genes"}
            for k in part:
                assert part[k].tobytes() == full[k][sl].tobytes(), (n, first, k)
    lw = full["loglik"] - rb
    w = np.exp(lw - lw.max())
    st = full["weight_stats"]
    assert st[0] == lw.max() and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    assert np.allclose(full["weighted_events"], w @ full["events"], rtol=1e-12, atol=1e-300)
    assert np.allclose(full["weighted_genes"], w @ full["genes"], rtol=1e-12, atol=1e-300)
    a, b = _eval(hip, fam, inp, slice(0, 9), log_offset=rb[:9]), _eval(hip, fam, inp, slice(9, 23), log_offset=rb[9:])
    for key in ("weighted_events", "weighted_genes"):
        mean, mx, s1, s2 = lp.combine([(a[key], a["weight_stats"]), (b[key], b["weight_stats"])])
        assert np.allclose(mean, full[key] / st[1], rtol=1e-14, atol=1e-300)
        assert mx == st[0] and abs(s1 - st[1]) < 1e-14 * st[1]
    fam.close()


HOOKS = {"LH_HOST_SUB": "1536", "LH_CHUNK": "1024"}


@pytest.fixture(scope="module")
def anchors(tmp_path_factory):
    from tests import events_boundaries_worker as ew
    d = str(tmp_path_factory.mktemp("events_boundaries"))
    return d, ew.build_anchors(d)


def test_anchor_rows_match_the_oracle(hip, anchors):
    from tests import batch_boundaries_worker as bw
    d, A = anchors
    F = bw.Fam(d, "igh")
    for i, s in enumerate(F.rows):
        F.o.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], 4, is_path=False)
        F.o.initialize_phylo_emission()
        ll = F.o.log_likelihood()
        assert abs(A["loglik"][i] - ll) <= 1e-12 * abs(ll)
        assert np.max(np.abs(A["events"][i] - eo.flat(eo.dense(F.o)))) < BOUND, i
    F.close()


@pytest.mark.parametrize("extra", [{}, {"LH_EVENTS_BLOCKS": "8"}], ids=["groups-and-slabs", "capped-grid"])
def test_weighted_sums_across_groups_and_slabs(anchors, extra):
    """n = 2048 + 257 with launch groups of 1024 (tests/test_gpu_codons_batch_boundaries.py's scheme, one child process):
    row i carries the bits of anchor row (7 i + i // G) % 23; the weighted sums lie within n 2^-52 of a long-double host
    sum and are bit-stable over two calls.  capped-grid: K10's workgroup cap lowered to 8, so that every lane group walks
    eight or more samples of a launch group over the same scratch tables."""
    e = {k: v for k, v in os.environ.items() if k not in HOOKS and k != "LH_EVENTS_BLOCKS"}
    e.update(HOOKS)
    e.update(extra)
    r = subprocess.run([sys.executable, "-m", "tests.events_boundaries_worker", "events", anchors[0], "ns=2305", "G=1024"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, "worker exited %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res["info"]))
    assert res["failures"] == [], "\n".join(res["failures"])


def test_device_entry_point():
    """lh_eval_events_batch_device with device-resident inputs on a torch stream (tests/events_device_worker.py, its own
    process): the bits of the host-pointer call; with one sample's device-resident schedule corrupted, that sample is NaN,
    is left out of the weighted sums and raises the handle's error word once."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "events_device_worker.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(res["same_bits"].values()), res["same_bits"]
    assert res["status_clean"] == 0
    assert res["status"] != 0 and "malformed schedule" in res["message"], res
    assert res["second_status"] == 0
    assert res["victim_all_nan"] and res["others_equal_clean"] and res["finite_sums"]
    assert res["max_lw_equal"] and res["sum_w_rel"] < 1e-14 and res["sum_w2_rel"] < 1e-14
    assert res["weighted_events_rel"] < 1e-13 and res["weighted_genes_rel"] < 1e-13


def test_refusals(hip, tmp_path):
    import linearham_amd
    from linearham_amd.capi import _EventsOutputs
    from tests import desc_builder as db
    o, rows, _ = vc.synthetic_rows(tmp_path, 2, locus="igh")
    inp = vc.device_inputs(hip, o, rows)
    vc.set_row(o, rows[0])
    bare = linearham_amd.Family(db.build_family_desc(o), hip)
    with pytest.raises(RuntimeError, match="lh_events_layout: lh_family_set_sampler has not been called"):
        hip.events_layout(bare)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = {k: np.ascontiguousarray(inp[k][:1]) for k in ("ops", "brlen", "er", "pi", "alpha")}
    ll = np.zeros(1)
    outs = _EventsOutputs(None, ll.ctypes.data_as(f64), None, None, None, None, None)

    def raw(handle, ops):
        return hip.lib.lh_eval_events_batch(handle, 1, inp["n_tips"], inp["max_depth"], ops,
                                            *[a[k].ctypes.data_as(f64) for k in ("brlen", "er", "pi", "alpha")], inp["R"],
                                            C.byref(outs))
    assert raw(bare.handle, a["ops"].ctypes.data_as(i32)) != 0
    assert hip.error() == "lh_eval_events_batch: lh_family_set_sampler has not been called"
    em = np.full((1, bare.n_xmsa), 0.5)
    assert hip.lib.lh_events_forward_batch(bare.handle, 1, em.ctypes.data_as(f64), None, None) != 0
    assert hip.error() == "lh_events_forward_batch: lh_family_set_sampler has not been called"
    bare.close()
    fam = vc.device_family(hip, o)
    assert raw(fam.handle, None) != 0 and hip.error() == "lh_eval_events_batch: null array"
    assert hip.lib.lh_events_forward_batch(fam.handle, 1, None, None, None) != 0
    assert hip.error() == "lh_events_forward_batch: null array"
    assert hip.lib.lh_events_forward_batch(fam.handle, -1, em.ctypes.data_as(f64), None, None) != 0
    assert raw(fam.handle, a["ops"].ctypes.data_as(i32)) == 0 and np.isfinite(ll[0])  # the handle still works
    # an empty batch and a call that asks for nothing are no errors
    assert hip.lib.lh_events_forward_batch(fam.handle, 0, None, None, None) == 0
    assert np.all(np.isfinite(_eval(hip, fam, inp)["events"]))
    fam.close()


def test_profile_read(hip, tmp_path):
    o, rows, _ = vc.synthetic_rows(tmp_path, 2, locus="igh")
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    fam.profile_enable(True)
    _eval(hip, fam, inp)
    _eval(hip, fam, inp)
    smooth_ms, events_ms, calls = hip.events_profile_read(fam)
    assert calls == 2 and smooth_ms > 0 and events_ms > 0
    assert hip.events_profile_read(fam)[2] == 0
    fam.profile_enable(False)
    fam.close()


# ---- the host library: one tree, the pipeline, the command line ----

def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _want_files(o, tables):
    """The three tables as the host writes them, from oracle tables through the oracle's own column mapping."""
    cols = eo.columns(o, tables)
    dele = {}
    for c in ("V3pDel", "D5pDel", "D3pDel", "J5pDel"):
        for (g, k), p in cols.get(c, {}).items():
            dele[(c, g, k)] = dele.get((c, g, k), 0.0) + p
            dele[(c, "*", k)] = dele.get((c, "*", k), 0.0) + p
    ins = {(c, k): p for c in ("VDInsertion", "VJInsertion", "DJInsertion") for k, p in enumerate(cols.get(c, []))}
    return dele, ins


def _compare_host(o, tables, genes, got, bound):
    dele, ins = _want_files(o, tables)
    # V5pDel and J3pDel are functions of the gene alone
    nV = len(o.vgerm.state_strs)
    for c, G, p in (("V5pDel", o.vgerm, genes[:nV]), ("J3pDel", o.jgerm, genes[len(genes) - len(o.jgerm.state_strs):])):
        for g, name in enumerate(G.state_strs):
            k = (G.left_del if c == "V5pDel" else G.right_del)[g]
            dele[(c, name, k)] = dele.get((c, name, k), 0.0) + p[g]
            dele[(c, "*", k)] = dele.get((c, "*", k), 0.0) + p[g]
    keys = {k for k, p in dele.items() if p > 0} | set(got["deletions"])
    assert keys, "empty table"
    assert max(abs(dele.get(k, 0.0) - got["deletions"].get(k, 0.0)) for k in keys) < bound
    keys = {k for k, p in ins.items() if p > 0} | set(got["insertions"])
    assert max(abs(ins.get(k, 0.0) - got["insertions"].get(k, 0.0)) for k in keys) < bound
    names = ["VD", "DJ"] if o.locus == "igh" else ["VJ"]
    for jn, (_, _, sp) in zip(names, tables):
        for (j, a, b), p in got["spans"].items():
            if j == jn:
                assert abs(sp[a, b] - p) < bound
        assert abs(sum(p for (j, _, _), p in got["spans"].items() if j == jn) - 1.0) < bound


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_host_one_tree_and_cli(case):
    """PhyloHMM::RearrangementEvents on the golden families against the oracle's tables mapped by the oracle's own members;
    `linearham --events` prints the same numbers."""
    from linearham_amd import host
    meta = vc.GOLD["PhyloHMM:" + case]["meta"]
    yaml_path, pdir, tree = os.path.join(vc.D, case + ".yaml"), os.path.join(vc.D, "hmm_params"), os.path.join(vc.D, "newton.tree")
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    h.initialize_phylo_parameters(tree, meta["er"], meta["pi"], meta["alpha"], meta["num_rates"], is_path=True)
    got = h.rearrangement_events()
    o, rows = vc.golden_rows(case)
    vc.set_row(o, rows[0])
    o.log_likelihood()
    from tests import posterior_oracle as po
    post = po.smoothing(o)
    genes = np.concatenate([post[k] for k in ("vgerm", "dgerm", "jgerm") if k in post])
    _compare_host(o, eo.dense(o, post), genes, got, BOUND)
    args = [_exe(), "--events", "--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--newick-path", tree,
            "--num-rates", str(meta["num_rates"]), "--alpha", repr(meta["alpha"])]
    args += sum([["--er", repr(x)] for x in meta["er"]], []) + sum([["--pi", repr(x)] for x in meta["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert host.parse_events(*r.stdout.split("\n\n")) == got


def test_pipeline_and_cli(tmp_path):
    """`linearham --events-pipeline` on a 150-row table with burn-in against the oracle's per-row tables weighted as
    po.weighted_marginals does; the files are byte-identical at two batch sizes; the library call writes the same files."""
    from linearham_amd import host
    from tests import posterior_oracle as po
    o, rows, (yaml_path, pdir, tsv) = vc.synthetic_rows(tmp_path, 150, locus="igh")
    rb = np.array([r["likelihood"] for r in rows])
    b = 0.2
    lls, flat, genes = [], [], []
    for r in rows:
        vc.set_row(o, r)
        lls.append(o.log_likelihood())
        post = po.smoothing(o)
        flat.append(eo.flat(eo.dense(o, post)))
        genes.append(np.concatenate([post[k] for k in ("vgerm", "dgerm", "jgerm")]))
    want, ess = po.weighted_marginals(np.array(lls), rb, np.array(flat), b)
    want_genes, _ = po.weighted_marginals(np.array(lls), rb, np.array(genes), b)
    texts = {}
    for batch in ("64", "1000"):
        prefix = str(tmp_path / ("e_" + batch))
        r = subprocess.run([_exe(), "--events-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir,
                            "--input-path", tsv, "--output-path", prefix, "--num-rates", "4", "--burnin-frac", str(b)],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, LH_PIPELINE_BATCH=batch))
        assert r.returncode == 0, r.stderr
        texts[batch] = [open(prefix + ext).read() for ext in (".deletions.tsv", ".insertions.tsv", ".spans.tsv", ".summary.tsv")]
    assert texts["64"] == texts["1000"]
    got, summary = host.read_events(prefix)
    _compare_host(o, eo.unflat(o, want), want_genes, got, BOUND)
    assert summary["rows_used"] == 150 - int(math.floor(b * 150)) and summary["rows_skipped_nonfinite"] == 0
    assert abs(summary["kish_ess"] - ess) < 1e-9 * ess
    for ln in texts["64"][0].split("\n")[1:-1]:
        p = ln.split("\t")[3]
        assert p == "%.17g" % float(p) and float(p) > 0
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    got2, summary2 = h.run_events_pipeline(tsv, str(tmp_path / "lib"), 4, burnin_frac=b)
    assert got2 == got and summary2 == summary
    r = subprocess.run([_exe(), "--events-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir,
                        "--input-path", "x", "--output-path", "y", "--devices", "0,1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr
