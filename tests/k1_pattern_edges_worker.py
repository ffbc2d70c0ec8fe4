"""Helper of tests/test_gpu_k1_pattern_edges.py: one process per set of K1 test hooks (read once per process), its verdict as
one JSON line.

    k1_pattern_edges_worker.py <rows> <workdir> <out.npz>

rows: "default" (the whole table of the test module) or "r4" (its R = 4 list on the 10-leaf family: what a hook process
runs).  Every row is evaluated through tests/test_gpu_parity.run_family and compared with the oracle by its compare, at its
bounds, in the default and in the extended-range mode (the latter as test_gpu_shape_edges.test_long_family_forward_matches_oracle
does it); then each of its two tree samples alone and as row 1 of a call of two, bit for bit.  The npz file keeps every
row's emissions and scaler counts for the comparison between processes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_rows(hip, desc, h, samples, R, extended):
    """ll, emissions, forward arrays and counts of `samples` in one call on a fresh handle."""
    import numpy as np
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    fam = linearham_amd.Family(desc, hip)
    if extended:
        fam.set_extended_range(True)
    T = h.msa.shape[0] + 1
    ops, brl, depth = [], [], 0
    for s in samples:
        children, root, brlen = db.tree_arrays(orc.parse_newick(s["tree"]), h.xmsa_labels)
        o, d = hip.schedule_tree(T, children, root)
        ops.append(o), brl.append(brlen)
        depth = max(depth, d)
    ll, res = fam.eval_batch(T, depth, np.stack(ops), np.stack(brl), [s["er"] for s in samples], [s["pi"] for s in samples],
                             [s["alpha"] for s in samples], R, want=("xmsa_emission", "forward", "scaler_counts"))
    info = fam.info()
    fam.close()
    return dict(ll=ll, em=res["xmsa_emission"], fwd=res["forward"], sco=res["scaler_counts"]), info


def rel(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.abs(b)
    d = np.where((a == b), 0.0, d)
    return float(np.max(d)) if d.size else 0.0


def run(which, workdir, out_path):
    import numpy as np
    import linearham_amd
    from tests import pattern_edge_cases as pe
    from tests import test_gpu_k1_pattern_edges as mod
    from tests import test_gpu_parity as tp
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    table = mod.TABLE if which == "default" else mod.r4_rows()
    hs, keep, report = {}, {}, []
    for row in table:
        case, R = row[0], row[1]
        h = hs[case.base] = pe.load_case(case, workdir, hs.get(case.base))
        samples = pe.samples(case.base, workdir)
        assert len(samples) == 2
        key = "%s_R%d" % (case.name, R)
        rec = dict(key=key, failures=[], figures={})
        fail, fig = rec["failures"], rec["figures"]
        # default mode: run_family / compare
        desc, ll, res, ref = tp.run_family(hip, h, samples, R)
        rec["form"], rec["n_patterns"], rec["depth"] = tp.LAST_RUN["form"], tp.LAST_RUN["n_patterns"], tp.LAST_RUN["max_depth"]
        rec["premises"] = [pe.check_premises(h, case, r["loglik"], r["xmsa_emission"]) for r in ref]
        for i, r in enumerate(ref):
            ex = tp.expand_forward(h, desc, res["forward"][i], res["scaler_counts"][i])
            fig["loglik"] = max(fig.get("loglik", 0.0), rel(ll[i], r["loglik"]))
            fig["rates"] = max(fig.get("rates", 0.0), rel(res["rates"][i], r["rates"]))
            fig["emission"] = max(fig.get("emission", 0.0), rel(res["xmsa_emission"][i], r["xmsa_emission"]))
            fig["forward"] = max([fig.get("forward", 0.0)] + [rel(ex[k], r[k]) for k in ex if k.endswith("_forward")])
            fig["counts_differ"] = fig.get("counts_differ", 0) + sum(ex[k] != r[k] for k in ex if "scaler" in k)
        try:
            tp.compare(h, desc, ll, res, ref)
        except AssertionError as e:
            fail.append("default mode against the oracle: %s" % str(e)[:400])
        # extended-range mode
        desc, llx, resx, ref = tp.run_family(hip, h, samples, R, extended=True)
        rec["form_ext"] = tp.LAST_RUN["form"]
        try:
            for i, r in enumerate(ref):
                fig["ext_loglik"] = max(fig.get("ext_loglik", 0.0), rel(llx[i], r["loglik"]))
                fig["ext_emission"] = max(fig.get("ext_emission", 0.0), rel(resx["xmsa_emission"][i], r["xmsa_emission"]))
                assert abs(llx[i] - r["loglik"]) <= 1e-10 * abs(r["loglik"]), (i, llx[i], r["loglik"])
                np.testing.assert_allclose(resx["xmsa_emission"][i], r["xmsa_emission"], rtol=1e-10)
                ex = tp.expand_forward(h, desc, resx["forward"][i], resx["scaler_counts"][i])
                got = np.log(ex["jgerm_forward"].sum()) - ex["jgerm_scaler_count"] * np.log(2.0 ** 256)
                assert abs(got - r["loglik"]) <= 1e-10 * abs(r["loglik"]), i
                big = r["jgerm_forward"] > r["jgerm_forward"].max() * 1e-100
                d = (ex["jgerm_scaler_count"] - r["jgerm_scaler_count"]) * 256
                fig["ext_forward"] = max(fig.get("ext_forward", 0.0), rel(ex["jgerm_forward"][big], np.ldexp(r["jgerm_forward"][big], d)))
                np.testing.assert_allclose(ex["jgerm_forward"][big], np.ldexp(r["jgerm_forward"][big], d), rtol=1e-9)
        except AssertionError as e:
            fail.append("extended-range mode against the oracle: %s" % str(e)[:400])
        # lh_family_info, and every row alone and as row 1 of a call of two
        for extended, full_ll, full in ((False, ll, res), (True, llx, resx)):
            tag = "extended" if extended else "default"
            swapped, info = device_rows(hip, desc, h, samples[::-1], R, extended)
            rec["info"] = list(info)
            if tuple(info) != pe.expected_info(h, case):
                fail.append("lh_family_info gives %s, the alignment has %s" % (info, pe.expected_info(h, case)))
            for i in range(2):
                alone, _ = device_rows(hip, desc, h, [samples[i]], R, extended)
                want = dict(ll=full_ll[i], em=full["xmsa_emission"][i], fwd=full["forward"][i], sco=full["scaler_counts"][i])
                second = swapped if i == 0 else dict(ll=full_ll, em=full["xmsa_emission"], fwd=full["forward"], sco=full["scaler_counts"])
                for k in want:
                    if not np.array_equal(alone[k][0], want[k]):
                        fail.append("%s mode: %s of row %d alone differs from the call of two" % (tag, k, i))
                    if not np.array_equal(second[k][1], alone[k][0]):
                        fail.append("%s mode: %s of row %d differs as row 1 of a call of two" % (tag, k, i))
        keep[key + "_em"], keep[key + "_sco"] = res["xmsa_emission"], res["scaler_counts"]
        keep[key + "_emx"], keep[key + "_scox"] = resx["xmsa_emission"], resx["scaler_counts"]
        report.append(rec)
    np.savez(out_path, **keep)
    return dict(rows=report)


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1], sys.argv[2], sys.argv[3])))
