"""K9 (exact codon and amino-acid marginals of the naive sequence, lh_codon.hip) on the device against
tests/codon_oracle.py."""
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
from tests import codon_oracle as co
from tests import posterior_oracle as po
from tests.helpers import gene_entries

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "golden", "data")
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_goldens.json")))
BOUND = 1e-10  # K5's


def _hip():
    from linearham_amd.capi import load_library
    return load_library()


def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _oracle_row(o, r, R=4):
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
    o.initialize_phylo_emission()
    return o.log_likelihood()


def _synthetic(tmp_path, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(**kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    return host.PhyloHMM(yaml_path, 0, pdir, 0), orc.PhyloHMM(yaml_path, 0, pdir, 0), (yaml_path, pdir, tsv), \
        sf.read_trees_tsv(tsv)


def _eval(hip, fl, sl=slice(None), **kw):
    return hip.eval_codons_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"][sl], fl["brlen"][sl], fl["er"][sl],
                                 fl["pi"][sl], fl["alpha"][sl], kw.pop("R", 4), **kw)


def _check_rows(hip, h, o, fl, rows, frames=(0, 1, 2), R=4):
    """Windows, genes and the expanded table of every row against the dense oracle form, in every frame."""
    ss = h.dump(1)
    for frame in frames:
        lay = hip.set_codons(fl["family"], frame)
        assert lay == dict(lp.codon_layout(ss, frame))
        res = _eval(hip, fl, R=R)
        for i, r in enumerate(rows):
            ll = _oracle_row(o, r, R)
            assert abs(res["loglik"][i] - ll) < 1e-9 * abs(ll)
            table, post = co.dense(o, frame)
            w, g, olay = co.window_inputs(o, table, post, frame)
            assert olay == lay
            ew, eg = np.max(np.abs(res["windows"][i] - w)), np.max(np.abs(res["genes"][i] - g))
            print("frame", frame, "row", i, "windows", ew, "genes", eg)
            assert ew < BOUND and eg < BOUND
            full = lp.codon_table(ss, res["windows"][i], res["genes"][i], lay)
            assert np.max(np.abs(full - table)) < BOUND
            assert np.max(np.abs(full.sum(axis=1) - 1.0)) < 1e-12


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_golden_families(tmp_path, case):
    meta = GOLD["PhyloHMM:" + case]["meta"]
    yaml_path, pdir, tree = os.path.join(D, case + ".yaml"), os.path.join(D, "hmm_params"), os.path.join(D, "newton.tree")
    R = meta["num_rates"]
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    h.initialize_phylo_parameters(tree, meta["er"], meta["pi"], meta["alpha"], R, is_path=True)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    # the same tree as a one-row table, for the raw device outputs
    newick = open(tree).read().strip()
    tsv = str(tmp_path / "one.tsv")
    cols = ["Iteration", "Posterior", "Likelihood", "Prior", "alpha"] + ["er[%d]" % i for i in range(1, 7)] + \
        ["pi[%d]" % i for i in range(1, 5)] + ["tree"]
    vals = ["0", "0", "0", "0", repr(meta["alpha"])] + [repr(x) for x in meta["er"]] + [repr(x) for x in meta["pi"]] + [newick]
    open(tsv, "w").write("\t".join(cols) + "\n" + "\t".join(vals) + "\n")
    row = dict(tree=newick, er=meta["er"], pi=meta["pi"], alpha=meta["alpha"])
    hip = _hip()
    fl = h.flatten_tsv(tsv, 1)
    _check_rows(hip, h, o, fl, [row], R=R)
    ss = h.dump(1)
    L = len(ss["msa"][0])
    sb, _ = h.naive_marginals()
    # K5's posteriors of the same row: K9's untagged recursion runs the same smoothing steps (lh_smooth.h)
    k5 = hip.eval_posterior_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"], fl["er"], fl["pi"],
                                  fl["alpha"], R, want=("posterior",))["posterior"]
    k5_genes = gene_entries(hip.events_layout(fl["family"]), k5[0])
    for frame in (0, 1, 2):
        table, aa = h.naive_codon_marginals(frame)
        _oracle_row(o, row, R)
        want, _ = co.dense(o, frame)
        assert np.max(np.abs(table - want)) < BOUND
        # the C++ expansion and fold against the Python ones, on the same device outputs
        lay = hip.set_codons(fl["family"], frame)
        res = _eval(hip, fl, R=R)
        assert np.array_equal(res["genes"][0], k5_genes)
        py = lp.codon_table(ss, res["windows"][0], res["genes"][0], lay)
        assert np.max(np.abs(table - py)) < 1e-13
        pa = lp.aa_table(py)
        assert len(aa) == len(pa)
        for c in range(len(pa)):
            assert set(aa[c]) == set(pa[c]), c
            assert max(abs(aa[c][a] - pa[c][a]) for a in pa[c]) < 1e-13
        # marginalised to sites: the same handle's K5 marginals
        cs = lp.codon_site_base(table, frame, L)
        cov = ~np.isnan(cs[:, 0])
        assert np.max(np.abs(cs[cov] - sb[cov])) < 1e-12


@pytest.mark.parametrize("locus,kw", [("igh", {}), ("igk", {}), ("igl", {}), ("igh", dict(ragged=4, ambiguous=0.02)),
                                      ("igh", dict(n_v=300, n_d=70, n_j=5)), ("igk", dict(n_v=150, n_j=70)),
                                      ("igh", dict(n_d=65, n_j=30))])
def test_synthetic_families(tmp_path, locus, kw):
    h, o, (_, _, tsv), rows = _synthetic(tmp_path, locus=locus, n_samples=2, **kw)
    fl = h.flatten_tsv(tsv, 2)
    _check_rows(_hip(), h, o, fl, rows[:2])


def test_extended_range_equals_default(tmp_path):
    h, o, (_, _, tsv), rows = _synthetic(tmp_path, locus="igh", n_samples=2)
    hip = _hip()
    fl = h.flatten_tsv(tsv, 2)
    hip.set_codons(fl["family"], 0)
    a = _eval(hip, fl)
    h.set_extended_range(True)
    b = _eval(hip, fl)
    assert np.all(np.isfinite(a["windows"])) and np.all(np.isfinite(a["genes"]))
    assert np.max(np.abs(a["windows"] - b["windows"])) < 1e-12
    assert np.max(np.abs(a["genes"] - b["genes"])) < 1e-12


def test_batches_and_weights(tmp_path):
    h, o, (_, _, tsv), rows = _synthetic(tmp_path, locus="igh", n_samples=300)
    hip = _hip()
    fl = h.flatten_tsv(tsv, 300)
    rb = np.array([r["likelihood"] for r in rows])
    hip.set_codons(fl["family"], 0)

    def run(sl):
        return _eval(hip, fl, sl, log_offset=rb[sl])
    full = run(slice(0, 300))  # crosses a slab boundary (256)
    lw = full["loglik"] - rb
    m = lw.max()
    w = np.exp(lw - m)
    st = full["weight_stats"]
    assert st[0] == m
    assert abs(st[1] - w.sum()) < 1e-13 * w.sum()
    assert abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    assert np.allclose(full["weighted_windows"], np.tensordot(w, full["windows"], axes=1), rtol=1e-12, atol=1e-300)
    assert np.allclose(full["weighted_genes"], w @ full["genes"], rtol=1e-12, atol=1e-300)
    # 100 + 200 combined on the host == the single call
    a, b = run(slice(0, 100)), run(slice(100, 300))
    for key in ("weighted_windows", "weighted_genes"):
        mean, mx, s1, s2 = lp.combine([(a[key], a["weight_stats"]), (b[key], b["weight_stats"])])
        assert np.allclose(mean, full[key] / st[1], rtol=1e-14, atol=1e-300)
        assert mx == m and abs(s1 - st[1]) < 1e-14 * st[1] and abs(s2 - st[2]) < 1e-14 * st[2]
    # every row: the same bits alone and as row 1 of a call of two
    for i in range(300):
        alone = run(slice(i, i + 1))
        pair = run(slice(i - 1, i + 1)) if i > 0 else None
        for key in ("windows", "genes", "loglik"):
            assert np.array_equal(alone[key][0], full[key][i]), (key, i)
            if pair is not None:
                assert np.array_equal(pair[key][1], full[key][i]), (key, i)


def test_device_entry_point():
    """lh_eval_codons_batch_device with device-resident inputs on a stream (tests/codon_device_worker.py, its own process):
    the bits of the host-pointer call; with one sample's device-resident schedule corrupted, that sample is NaN, is left
    out of the weighted sums and raises the handle's error word once."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "codon_device_worker.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(res["same_bits"].values()), res["same_bits"]
    assert res["status_clean"] == 0
    assert res["status"] != 0 and "malformed schedule" in res["message"], res
    assert res["second_status"] == 0
    assert res["victim_all_nan"] and res["others_equal_clean"] and res["finite_sums"]
    assert res["max_lw_equal"] and res["sum_w_rel"] < 1e-14 and res["sum_w2_rel"] < 1e-14
    assert res["weighted_windows_rel"] < 1e-13 and res["weighted_genes_rel"] < 1e-13


def _raw_eval_refused(hip, fl):
    """lh_eval_codons_batch itself (not the wrapper, which asks lh_codon_layout first) on a handle without a frame."""
    import ctypes as C
    from linearham_amd.capi import _CodonOutputs
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    a = {k: np.ascontiguousarray(fl[k][:1]) for k in ("ops", "brlen", "er", "pi", "alpha")}
    ll = np.zeros(1)
    outs = _CodonOutputs(None, ll.ctypes.data_as(f64), None, None, None, None, None)
    rc = hip.lib.lh_eval_codons_batch(fl["family"], 1, fl["n_tips"], fl["max_depth"], a["ops"].ctypes.data_as(i32),
                                      *[a[k].ctypes.data_as(f64) for k in ("brlen", "er", "pi", "alpha")], 4, C.byref(outs))
    assert rc != 0 and hip.error() == "lh_eval_codons_batch: lh_family_set_codons has not been called"


def test_refusals(tmp_path):
    h, o, (yaml_path, pdir, tsv), rows = _synthetic(tmp_path, locus="igh", n_samples=2)
    hip = _hip()
    fl = h.flatten_tsv(tsv, 2)
    with pytest.raises(RuntimeError, match="lh_codon_layout: lh_family_set_codons has not been called"):
        _eval(hip, fl)
    _raw_eval_refused(hip, fl)
    for frame in (-1, 3):
        with pytest.raises(RuntimeError, match="frame must be 0, 1 or 2"):
            hip.set_codons(fl["family"], frame)
    _raw_eval_refused(hip, fl)  # a refused frame leaves the handle without one
    # a family without sampler tables
    import linearham_amd
    from tests import desc_builder as db
    _oracle_row(o, rows[0])
    bare = linearham_amd.Family(db.build_family_desc(o), hip)
    with pytest.raises(RuntimeError, match="lh_family_set_sampler has not been called"):
        hip.set_codons(bare, 0)
    bare.close()
    hip.set_codons(fl["family"], 1)
    assert np.all(np.isfinite(_eval(hip, fl)["windows"]))


def _oracle_tables(o, rows, frame):
    lls, tables = [], []
    for r in rows:
        lls.append(_oracle_row(o, r))
        tables.append(co.dense(o, frame)[0])
    return np.array(lls), np.array(tables)


def test_pipeline_and_cli(tmp_path):
    """`linearham --codon-marginals-pipeline` on a 150-row table with burn-in, in frames 0 and 2, against the oracle's
    per-row tables aggregated by the R script's rules; the files do not depend on the batch size; the library call gives
    the same files."""
    h, o, (yaml_path, pdir, tsv), rows = _synthetic(tmp_path, locus="igh", n_samples=150)
    rb = np.array([r["likelihood"] for r in rows])
    b = 0.2
    aa_of = lp.codon_amino_acids()
    for frame in (0, 2):
        lls, tables = _oracle_tables(o, rows, frame)
        want, ess = po.weighted_marginals(lls, rb, tables, b)
        texts = {}
        for batch in ("64", "1000"):
            prefix = str(tmp_path / ("c%d_%s" % (frame, batch)))
            r = subprocess.run([_exe(), "--codon-marginals-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0",
                                "--hmm-param-dir", pdir, "--input-path", tsv, "--output-path", prefix, "--num-rates", "4",
                                "--burnin-frac", str(b), "--frame", str(frame)], capture_output=True, text=True,
                               timeout=300, env=dict(os.environ, LH_PIPELINE_BATCH=batch))
            assert r.returncode == 0, r.stderr
            texts[batch] = [open(prefix + ext).read() for ext in (".codons.tsv", ".aa.tsv", ".summary.tsv")]
        assert texts["64"] == texts["1000"]
        table, aa, summary = host.read_codon_marginals(prefix)
        assert table.shape == want.shape
        assert np.max(np.abs(table - want)) < BOUND
        pa = lp.aa_table(want, aa_of)
        for c in range(len(pa)):
            keys = set(pa[c]) | set(aa[c])
            assert max(abs(pa[c].get(a, 0.0) - aa[c].get(a, 0.0)) for a in keys) < BOUND
        assert summary["rows_used"] == 150 - int(math.floor(b * 150)) and summary["rows_skipped_nonfinite"] == 0
        assert summary["frame"] == frame and abs(summary["kish_ess"] - ess) < 1e-9 * ess
        lines = texts["64"][0].split("\n")
        assert lines[0] == "codon\tfirst_site\tbases\tprobability"
        for ln in lines[1:-1]:
            c, s, bases, p = ln.split("\t")
            assert int(s) == frame + 3 * int(c) and float(p) > 0 and p == host.repr_double(float(p))
        t2, aa2, s2 = h.run_codon_marginals_pipeline(tsv, str(tmp_path / "lib"), 4, burnin_frac=b, frame=frame)
        assert np.array_equal(t2, table) and aa2 == aa and s2 == summary
    # more than one device is refused
    r = subprocess.run([_exe(), "--codon-marginals-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0",
                        "--hmm-param-dir", pdir, "--input-path", "x", "--output-path", "y", "--devices", "0,1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one device" in r.stderr


def test_cli_codon_marginals_golden():
    """`linearham --codon-marginals [--frame f]` prints the numbers of PhyloHMM.naive_codon_marginals."""
    case = "phylo_hmm_input"
    meta = GOLD["PhyloHMM:" + case]["meta"]
    yaml_path, pdir, tree = os.path.join(D, case + ".yaml"), os.path.join(D, "hmm_params"), os.path.join(D, "newton.tree")
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    h.initialize_phylo_parameters(tree, meta["er"], meta["pi"], meta["alpha"], meta["num_rates"], is_path=True)
    for frame in (None, 1):
        args = [_exe(), "--codon-marginals", "--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir,
                "--newick-path", tree, "--num-rates", str(meta["num_rates"]), "--alpha", repr(meta["alpha"])]
        args += sum([["--er", repr(x)] for x in meta["er"]], []) + sum([["--pi", repr(x)] for x in meta["pi"]], [])
        args += [] if frame is None else ["--frame", str(frame)]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        codon_part, aa_part = r.stdout.split("\n\n")
        table, aa = host.parse_codon_tables(codon_part, aa_part)
        want, want_aa = h.naive_codon_marginals(frame or 0)
        assert np.array_equal(table, want) and aa == want_aa
