"""Helper of tests/test_gpu_ext_deep_rows.py: every entry point that reads the extended-range forward arrays and K1's (value,
2^-256 count) columns, on the rows of tests/ext_deep_cases.py, in a process of its own per family.

  python tests/ext_deep_worker.py --cpu DIR [--jobs N]        CPU: DIR/ext_deep_<row>.npz (ext_deep_cases.build) and its report
  python tests/ext_deep_worker.py --gpu DIR --family F        GPU: the family's rows in one call, control and deep rows
                                                              alternating, in both range modes; one JSON line
                                                              {"failures": [..], "figures": [..], "rows": n, "checked": {..}}

The family is the one the host library reads (cadence_cases.write_family_files), its handle wrapped in linearham_amd.Family;
default K1 form only.  What is asserted: tests/test_gpu_ext_deep_rows.py's docstring."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FRAMES = (0, 1, 2)
K12_FULL = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
K12_LEAN = K12_FULL[1:]
K15_TABLES = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")
K14_TABLES = ("codons", "change")
PADDED = ("edge_change", "edge_load")          # [P + 1] tables: slots [0, P) and the naive edge's


def _far(a, b):
    with np.errstate(invalid="ignore"):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        same_shape = a.shape == b.shape or b.ndim == 0
        return float(np.abs(a - b).max()) if same_shape and np.isfinite(a).all() and np.isfinite(b).all() else float("inf")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class Batch:
    """The family's rows as the batched entry points take them, and every entry point on a selection of them."""

    def __init__(self, hip, family, out_dir, workdir):
        from linearham_amd import capi, host
        from tests import cadence_cases as cc
        from tests import ext_deep_cases as xd
        from tests import lineage_cadence_worker as lw
        from tests.ancestral_cases import write_table
        self.hip, self.family = hip, family
        self.h = h = cc.load_family(family, workdir)
        self.rows = xd.rows_of(family)
        self.ref = [np.load(os.path.join(out_dir, "ext_deep_%s.npz" % r[0])) for r in self.rows]
        self.d_ref = [json.loads(str(x["d_ref"])) for x in self.ref]
        samples = [cc.sample_of(r)[0] for r in self.rows]
        self.sched = sched = [cc.schedule(h, s) for s in samples]
        self.R = cc.FAMILIES[family]["R"]
        self.T, self.depth = sched[0][0], max(s[5] for s in sched)
        self.ops, self.brl = np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched])
        self.er, self.pi = np.array([s["er"] for s in samples]), np.array([s["pi"] for s in samples])
        self.alpha = np.array([s["alpha"] for s in samples])
        self.n, self.L = len(self.rows), h.msa.shape[1]
        yaml_path, pdir = cc.write_family_files(family, workdir, h)
        self.hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
        tsv = os.path.join(workdir, "rows.tsv")
        write_table(tsv, samples[:1])
        self.hfam = self.hh.flatten_tsv(tsv, 1)["family"]
        self.fam = capi.Family.borrow(self.hfam, hip)
        hip.set_ancestral_candidates(self.hfam, np.full((1, self.L), 4, dtype=np.uint8))
        self.ss = self.hh.dump(1)
        self.seeds = lw.SEEDS[family]
        self.paths = {si: [capi.seed_path(self.T, s[1], s[2], tip) for s in sched] for si, tip in enumerate(self.seeds)}
        self.words = np.stack([x["k4_words"] for x in self.ref])
        assert hip.lib.lh_sample_words(self.fam.handle) == self.words.shape[1]
        self.n_states = hip.sample_states(self.hfam)

    def set_mode(self, ext):
        self.hh.set_extended_range(bool(ext))
        self.fam.set_extended_range(bool(ext))

    def tree(self, sel):
        return self.T, self.depth, self.ops[sel], self.brl[sel], self.er[sel], self.pi[sel]

    def sample(self, sel):
        """lh_eval_sample_batch: (loglik, states)."""
        lib, n = self.hip.lib, len(sel)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (self.brl[sel], self.er[sel], self.pi[sel], self.alpha[sel])]
        ops, words = np.ascontiguousarray(self.ops[sel], dtype=np.int32), np.ascontiguousarray(self.words[sel], dtype=np.uint32)
        ll, st = np.zeros(n), np.zeros((n, self.n_states), dtype=np.int32)
        lib.lh_eval_sample_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)] + \
            [C.POINTER(C.c_double)] * 4 + [C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int32)]
        self.hip.check(lib.lh_eval_sample_batch(self.fam.handle, n, self.T, self.depth, p(ops, C.c_int32),
                                                *[p(a, C.c_double) for a in arrays], self.R, p(words, C.c_uint32), p(ll, C.c_double),
                                                None, p(st, C.c_int32)))
        return ll, st

    def first(self, sel):
        """K1 + K2, K5, K9 in three frames, K10, K8, K4 on the rows `sel`: {name: [per row]}."""
        from linearham_amd import posterior as lp
        hip, hfam, sel = self.hip, self.hfam, np.asarray(sel)
        a = self.tree(sel) + (self.alpha[sel], self.R)
        out = {}
        ll, ev = self.fam.eval_batch(*a, want=("rates", "forward", "scaler_counts"))
        out.update(loglik=ll, rates=ev["rates"], forward=ev["forward"], scaler_counts=ev["scaler_counts"])
        k5 = hip.eval_posterior_batch(hfam, *a, want=("loglik", "posterior"))
        out.update(k5_loglik=k5["loglik"], k5_posterior=k5["posterior"])
        for f in FRAMES:
            lay = hip.set_codons(hfam, f)
            k9 = hip.eval_codons_batch(hfam, *a, want=("loglik", "windows", "genes"))
            out.update({"k9_%d_loglik" % f: k9["loglik"], "k9_%d_windows" % f: k9["windows"], "k9_%d_genes" % f: k9["genes"]})
            out["k9_%d_table" % f] = [lp.codon_table(self.ss, k9["windows"][i], k9["genes"][i], lay)
                                      if np.isfinite(k9["windows"][i]).all() else np.full((lay["n_codons"], 125), np.nan)
                                      for i in range(len(sel))]
        k10 = hip.eval_events_batch(hfam, *a, want=("loglik", "events", "genes"))
        out.update(k10_loglik=k10["loglik"], k10_events=k10["events"], k10_genes=k10["genes"])
        k8 = hip.eval_viterbi_batch(hfam, *a, want=("loglik", "states", "log_path"))
        out.update(k8_loglik=k8["loglik"], k8_states=k8["states"], k8_log_path=k8["log_path"])
        out["k4_loglik"], out["k4_states"] = self.sample(sel)
        return {k: [v[i] for i in range(len(sel))] for k, v in out.items()}

    def lineage(self, sel, si, frame, log_offset=None, level="all"):
        """The evaluation forms of K11, K12 (full and lean), K14 (both nodes) and K15 on the rows `sel` for seed tip number si
        in `frame`: ({name: [per row, the path tables cut to the row's own slots]}, the calls' raw results)."""
        from linearham_amd import capi
        hip, hfam, sel = self.hip, self.hfam, np.asarray(sel)
        a = self.tree(sel) + (self.alpha[sel], self.R)
        tip = self.seeds[si]
        paths = [self.paths[si][i] for i in sel]
        padded = capi.pad_paths(paths)
        lo = dict(log_offset=log_offset) if log_offset is not None else {}
        w = lambda *names: names + ("weight_stats",) if log_offset is not None else ()
        raw, out = {}, {}
        hip.set_codons(hfam, frame)
        if level == "all":
            raw["k11"] = hip.eval_ancestral_batch(hfam, *a, padded, want=("loglik", "site_base", "marg", "rate_post") +
                                                  w("weighted_sum", "weighted_rate"), **lo)
            raw["k12"] = hip.eval_edges_batch(hfam, *a, padded, tip, want=("loglik",) + K12_FULL +
                                              w("weighted_counts", "weighted_naive_edge"), **lo)
            raw["k12lean"] = hip.eval_edges_batch(hfam, *a, padded, tip, want=("loglik",) + K12_LEAN + w(), **lo)
        for name, node in (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA)):
            raw["k14_" + name] = hip.eval_node_codons_batch(hfam, *a, padded, node, want=("loglik",) + K14_TABLES +
                                                            w("weighted_codons", "weighted_change"), **lo)
        raw["k15"] = hip.eval_codon_edges_batch(hfam, *a, padded, tip, want=("loglik",) + K15_TABLES +
                                                w("weighted_codon_counts", "weighted_aa_counts", "weighted_seed_change"), **lo)
        for call, res in raw.items():
            for k, v in res.items():
                if k.startswith("weight"):
                    continue
                rows = []
                for i in range(len(sel)):
                    P = len(paths[i])
                    x = v[i]
                    if k in ("marg", "edge"):
                        x = x[:P]
                    elif k in PADDED and x.shape[0] == padded.shape[1] + 1:
                        x = np.concatenate([x[:P], x[-1:]])
                    rows.append(x)
                out["%s_%s" % (call, k)] = rows
        return out, raw, paths


def run_gpu(out_dir, family, workdir):
    import linearham_amd
    from linearham_amd import capi
    from linearham_amd import posterior as lp
    from tests import cadence_worker as cw
    from tests import desc_builder as db
    from tests import ext_deep_cases as xd
    from tests import k4_draw_cases as k4
    from tests import test_gpu_parity as tp
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    B = Batch(hip, family, out_dir, workdir)
    h, rows, ref, n, L = B.h, B.rows, B.ref, B.n, B.L
    kinds = [xd.kind_of(r) for r in rows]
    everything = np.arange(n)
    failures, figures, checked = [], [], {}

    def note(cond, text):
        if not cond:
            failures.append(text)

    def held(where, key, got, want, d_ref, fig, bound=None):
        """One table against its reference at max(1e-10, 8 d_ref); counted per table."""
        d = _far(got, want)
        b = xd.bound(d_ref) if bound is None else bound
        fig[key] = dict(d=d, d_ref=float(d_ref), bound=b)
        checked[key.split("@")[0]] = checked.get(key.split("@")[0], 0) + 1
        note(d <= b, "%s: %s off the reference by %.3g (bound %.3g, d_ref %.3g)" % (where, key, d, b, d_ref))

    def lineage_keys(i, si, frame, level):
        """{device table name: (reference, d_ref)} of row i for one (seed tip, frame)."""
        x, dl = ref[i], B.d_ref[i]["lineage"][str(si)]
        out = {}
        if level == "all":
            out["k11_marg"] = (x["k11_%d_marg" % si], dl["k11_marg"])
            out["k11_rate_post"] = (x["k11_%d_rate_post" % si], dl["k11_rate_post"])
            out["k11_site_base"] = (x["site_base"], B.d_ref[i]["site_base"])
            for k in K12_FULL:
                out["k12_" + k] = (x["k12_%d_%s" % (si, k)], dl["k12_" + k])
            for k in K12_LEAN:
                out["k12lean_" + k] = (x["k12_%d_%s" % (si, k)], dl["k12_" + k])
        for k in K15_TABLES:
            out["k15_" + k] = (x["k15_%d_%d_%s" % (si, frame, k)], dl["k15_%d_%s" % (frame, k)])
        for node in ("parent", "mrca"):
            for k in K14_TABLES:
                out["k14_%s_%s" % (node, k)] = (x["k14_%d_%d_%s_%s" % (si, frame, node, k)], dl["k14_%d_%s_%s" % (frame, node, k)])
        # the device mixes with its own site_base and contracts with its own Q: their d_ref is part of every table's
        own = lambda key: B.d_ref[i]["site_base" if key.startswith(("k11", "k12")) else "Q"]
        return {key: (want, max(float(d), float(own(key)))) for key, (want, d) in out.items()}

    desc = db.build_family_desc(h)
    results = {}
    for ext in (True, False):
        mode = "extended" if ext else "default"
        B.set_mode(ext)
        got = B.first(everything)
        lin, lin_raw, lin_paths = {}, {}, {}
        for si, frame in xd.lw_combos():
            level = "all" if frame == 0 else "codons"
            lin[(si, frame)], lin_raw[(si, frame)], lin_paths[(si, frame)] = B.lineage(everything, si, frame, level=level)
        results[mode] = (got, lin)
        for i, r in enumerate(rows):
            where, x, dr, kind = "%s [%s]" % (r[0], mode), ref[i], B.d_ref[i], kinds[i]
            fig = dict(row=r[0], position=i, kind=kind, mode=mode)
            if not ext and kind != "control":
                # ---- default mode on a row that underflows: no finite log-likelihood, NaN tables, no path
                lls = [got[k][i] for k in got if k.endswith("loglik")] + [v[i] for d in lin.values() for k, v in d.items() if k.endswith("loglik")]
                note(not np.isfinite(lls).any(), "%s: a finite log-likelihood in default mode: %s" % (where, lls))
                tables = [got[k][i] for k in ("k5_posterior", "k10_events", "k10_genes") + tuple("k9_%d_windows" % f for f in FRAMES)]
                tables += [v[i] for d in lin.values() for k, v in d.items() if not k.endswith("loglik")]
                note(all(np.isnan(t).all() for t in tables), "%s: a table holds something other than NaN in default mode" % where)
                note((got["k8_states"][i] == -1).all(), "%s: K8's states are not -1 in default mode" % where)
                fig["default_nan_tables"] = len(tables)
                checked["default_nan_rows"] = checked.get("default_nan_rows", 0) + 1
                figures.append(fig)
                continue
            # ---- log-likelihood, every entry point's own
            want_ll = float(x["loglik"])
            b_ll = cw.ll_bound("control" if kind == "control" else r[2], float(x["d_c"]))
            for k in [k for k in got if k.endswith("loglik")]:
                d = abs(got[k][i] - want_ll) / abs(want_ll) if np.isfinite(got[k][i]) else float("inf")
                fig[k] = dict(d=d, bound=b_ll)
                note(d <= b_ll, "%s: %s %.15g, mpmath %.15g: %.3g relative, bound %.3g" % (where, k, got[k][i], want_ll, d, b_ll))
                note(_bits(got[k][i]) == _bits(got["loglik"][i]), "%s: %s is not lh_eval_batch's log-likelihood bit for bit" % (where, k))
            checked["loglik"] = checked.get("loglik", 0) + 1
            # ---- K5
            post = got["k5_posterior"][i]
            held(where, "k5_posterior", post, x["compact"], dr["posterior"], fig)
            ok = bool(np.isfinite(post).all())
            sb = lp.site_base(B.ss, post) if ok else np.full((L, 5), np.nan)
            held(where, "k5_site_base", sb, x["site_base"], dr["site_base"], fig)
            gp = lp.gene_posteriors(B.ss, post) if ok else {}
            genes = np.concatenate([[gp[s][g] for g in sorted(gp[s])] for s in ("V", "D", "J")]) if ok else np.full(len(x["genes"]), np.nan)
            held(where, "k5_genes", genes, x["genes"], dr["genes"], fig)
            fig["k5_sums"] = _far(sb.sum(axis=1), 1.0) if ok else float("inf")
            note(fig["k5_sums"] <= 1e-12, "%s: K5's site marginals do not sum to 1: %.3g" % (where, fig["k5_sums"]))
            # ---- K9
            for f in FRAMES:
                table = got["k9_%d_table" % f][i]
                held(where, "k9_table@%d" % f, table, x["Q%d" % f], dr["Q"], fig)
                s = _far(table.sum(axis=1), 1.0)
                fig["k9_sums@%d" % f] = s
                note(s <= 1e-12, "%s: K9's rows do not sum to 1 in frame %d: %.3g" % (where, f, s))
                note(_bits(got["k9_%d_genes" % f][i]) == _bits(got["k10_genes"][i]), "%s: K9's genes differ from K10's in frame %d" % (where, f))
            # ---- K10
            held(where, "k10_events", got["k10_events"][i], x["events"], dr["events"], fig)
            if np.isfinite(got["k10_events"][i]).all():
                rules = []
                for ex_, en, sp in capi.split_events(hip.events_layout(B.hfam), got["k10_events"][i]):
                    W = sp.shape[0] - 1
                    rules += [abs(ex_.sum() - 1.0), abs(en.sum() - 1.0), abs(sp.sum() - 1.0), float(np.abs(sp[np.tril_indices(W + 1, -1)]).max()),
                              float(np.abs(sp.sum(axis=1) - ex_.sum(axis=0)).max()), float(np.abs(sp.sum(axis=0) - en.sum(axis=0)).max())]
                fig["k10_rules"] = float(max(rules))
                note(fig["k10_rules"] < 1e-10, "%s: K10's sum rules: %s" % (where, rules))       # test_gpu_events.BOUND
            # ---- K8
            same = bool(np.array_equal(got["k8_states"][i], x["viterbi_states"]))
            lp_got, lp_want = float(got["k8_log_path"][i]), float(x["viterbi_log_path"])
            fig["k8_states_equal"], fig["k8_log_path"] = same, dict(d=abs(lp_got - lp_want), bound=1e-12 * (1 + abs(lp_want)))
            checked["k8"] = checked.get("k8", 0) + 1
            note(same, "%s: K8's states differ from the reference's: %s, %s" % (where, got["k8_states"][i].tolist(), x["viterbi_states"].tolist()))
            note(abs(lp_got - lp_want) <= 1e-12 * (1 + abs(lp_want)), "%s: K8's log_path %.15g, reference %.15g" % (where, lp_got, lp_want))
            # ---- K4: tier 1 on the row's own device forward arrays, tier 2 on the reference alpha rows where the margin allows
            fwd = tp.expand_forward(h, desc, got["forward"][i], got["scaler_counts"][i])
            t1, used, _ = k4.draws_on_forward(h, fwd, B.words[i])
            fig["k4_tier1"] = bool(used == B.words.shape[1] and np.array_equal(got["k4_states"][i], t1))
            note(fig["k4_tier1"], "%s: K4's states differ from the dense draw on the row's own forward arrays" % where)
            fig["k4_margin"] = float(x["k4_margin"])
            fig["k4_qualifies"] = bool(fig["k4_margin"] > xd.K4_MARGIN)
            if fig["k4_qualifies"]:
                fig["k4_tier2"] = bool(np.array_equal(got["k4_states"][i], x["k4_states"]))
                note(fig["k4_tier2"], "%s: K4's states differ from the draw on the reference alpha rows (margin %.3g)" % (where, fig["k4_margin"]))
            checked["k4"] = checked.get("k4", 0) + 1
            # ---- the evaluation forms
            for (si, frame), tabs in lin.items():
                if (si, frame) not in xd.combos_of(r):
                    continue
                level = "all" if frame == 0 else "codons"
                tag = "tip %d frame %d" % (B.seeds[si], frame)
                for key, (want, d_ref) in lineage_keys(i, si, frame, level).items():
                    held("%s %s" % (where, tag), "%s@%d_%d" % (key, si, frame), tabs[key][i], want, d_ref, fig)
                sums = [_far(tabs["k14_%s_%s" % (nd, k)][i].sum(axis=-1), 1.0) for nd in ("parent", "mrca") for k in K14_TABLES]
                if level == "all":
                    sums += [_far(tabs[k][i].sum(axis=-1), 1.0) for k in ("k11_marg", "k11_rate_post", "k12_rate_post", "k12lean_rate_post")]
                fig["lineage_sums@%d_%d" % (si, frame)] = max(sums)
                note(max(sums) <= 1e-12, "%s %s: tables of the evaluation forms do not sum to 1: %s" % (where, tag, sums))
                for k, v in tabs.items():
                    if k.endswith("loglik"):
                        note(_bits(v[i]) == _bits(got["loglik"][i]), "%s %s: %s is not lh_eval_batch's log-likelihood bit for bit" % (where, tag, k))
            figures.append(fig)

        # ---- every distinct row alone and as row 1 of a call of two: every output bit-identical
        if ext:
            first_at = {}
            for i, r in enumerate(rows):
                first_at.setdefault(r[0], i)
            for name, i in first_at.items():
                j = (i + 1) % n
                for what, sel, at in (("alone", [i], 0), ("as row 1 of two", [j, i], 1)):
                    one = B.first(sel)
                    bad = [k for k in one if k != "k9_0_table" and _bits(one[k][at]) != _bits(got[k][i])]
                    o2, _, _ = B.lineage(sel, 0, 0)
                    bad += [k for k in o2 if _bits(o2[k][at]) != _bits(lin[(0, 0)][k][i])]
                    note(not bad, "%s [extended] %s: not bit-identical with the batch: %s" % (name, what, bad))
                    checked["independence"] = checked.get("independence", 0) + 1

            # ---- the given-rates forms on the device's own rates, K5 site_base and K9 table: bit for bit
            a = B.tree(everything)
            rates = np.stack(got["rates"])
            for (si, frame), tabs in lin.items():
                padded = capi.pad_paths(lin_paths[(si, frame)])
                tip = B.seeds[si]
                raw = lin_raw[(si, frame)]
                same = {}
                if frame == 0:
                    q = raw["k11"]["site_base"]
                    marg, rp = B.fam.asr_marginals_batch(*a, rates, q, padded)
                    same["k11_marg"], same["k11_rate_post"] = _bits(marg) == _bits(raw["k11"]["marg"]), _bits(rp) == _bits(raw["k11"]["rate_post"])
                    full = B.fam.asr_edges_batch(*a, rates, q, padded, tip, want=K12_FULL)
                    lean = B.fam.asr_edges_batch(*a, rates, q, padded, tip, want=K12_LEAN)
                    same.update({"k12_" + k: _bits(full[k]) == _bits(raw["k12"][k]) for k in K12_FULL})
                    same.update({"k12lean_" + k: _bits(lean[k]) == _bits(raw["k12lean"][k]) for k in K12_LEAN})
                Q = np.stack(got["k9_%d_table" % frame])
                hip.set_codons(B.hfam, frame)
                given = B.fam.asr_codon_edges_batch(*a, rates, Q, padded, tip)
                same.update({"k15_" + k: _bits(given[k]) == _bits(raw["k15"][k]) for k in K15_TABLES})
                for name, node in (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA)):
                    g14 = dict(zip(K14_TABLES, B.fam.asr_node_codons_batch(*a, rates, Q, padded, node)))
                    same.update({"k14_%s_%s" % (name, k): _bits(g14[k]) == _bits(raw["k14_" + name][k]) for k in K14_TABLES})
                note(all(same.values()), "[extended] tip %d frame %d: the given-rates forms do not have the evaluation forms' bits: %s" %
                     (tip, frame, sorted(k for k, v in same.items() if not v)))
                checked["given_rates"] = checked.get("given_rates", 0) + len(same)

            # ---- with log_offset: the weighted sums over ALL rows (the deep rows carry weight in this mode) against numpy
            lo = np.array([float(x["loglik"]) for x in ref]) + 0.1 * np.arange(n)
            tabs, raw, paths = B.lineage(everything, 0, 0, log_offset=lo)
            lw_ = np.array(got["loglik"]) - lo
            w = np.exp(lw_ - lw_.max())
            worst = 0.0

            def rel(a_, b_):
                return float(np.max(np.abs(a_ - b_) / np.maximum(np.abs(b_), 1e-300))) if np.isfinite(a_).all() else float("inf")
            ends = np.stack([np.stack([raw["k11"]["marg"][i, 0], raw["k11"]["marg"][i, len(paths[i]) - 1]]) for i in range(n)])
            pairs = [(raw["k11"]["weighted_sum"], np.tensordot(w, ends, 1)), (raw["k11"]["weighted_rate"], np.tensordot(w, raw["k11"]["rate_post"], 1)),
                     (raw["k12"]["weighted_counts"], np.tensordot(w, raw["k12"]["chain_counts"], 1)),
                     (raw["k12"]["weighted_naive_edge"], np.tensordot(w, raw["k12"]["naive_edge"], 1)),
                     (raw["k15"]["weighted_codon_counts"], np.tensordot(w, raw["k15"]["codon_counts"], 1)),
                     (raw["k15"]["weighted_aa_counts"], np.tensordot(w, raw["k15"]["aa_counts"], 1)),
                     (raw["k15"]["weighted_seed_change"], np.tensordot(w, raw["k15"]["seed_change"], 1))]
            for nd in ("parent", "mrca"):
                pairs += [(raw["k14_" + nd]["weighted_codons"], np.tensordot(w, raw["k14_" + nd]["codons"], 1)),
                          (raw["k14_" + nd]["weighted_change"], np.tensordot(w, raw["k14_" + nd]["change"], 1))]
            for call in raw.values():
                if "weight_stats" in call:
                    pairs.append((call["weight_stats"], np.array([lw_.max(), w.sum(), (w * w).sum()])))
            for a_, b_ in pairs:
                mask = np.abs(b_) > 1e-200
                worst = max(worst, rel(a_[mask], b_[mask]), _far(a_[~mask], b_[~mask]) if (~mask).any() else 0.0)
            checked["weighted"] = len(pairs)
            note(worst <= 1e-12, "[extended] weighted outputs against numpy over all rows: %.3g relative" % worst)
            note(w.min() > 0.05, "[extended] a row carries no weight: %s" % w.tolist())
            figures.append(dict(row="(weighted sums)", mode=mode, weighted_rel=worst, smallest_weight=float(w.min())))

    # ---- the control rows in the two modes: K5, K9, K10 and the evaluation forms within 1e-12, K8 equal bits
    (ge, le), (gd, ld) = results["extended"], results["default"]
    for i, r in enumerate(rows):
        if kinds[i] != "control":
            continue
        far = {k: _far(ge[k][i], gd[k][i]) for k in ["k5_posterior", "k10_events"] + ["k9_%d_table" % f for f in FRAMES]}
        for key in le:
            far.update({"%s@%d_%d" % ((k,) + key): _far(le[key][k][i], ld[key][k][i]) for k in le[key] if not k.endswith("loglik")})
        note(max(far.values()) <= 1e-12, "%s at %d: the two modes differ by more than 1e-12: %s" % (r[0], i, {k: v for k, v in far.items() if v > 1e-12}))
        k8 = _bits(ge["k8_states"][i]) == _bits(gd["k8_states"][i]) and _bits(ge["k8_log_path"][i]) == _bits(gd["k8_log_path"][i])
        note(k8, "%s at %d: K8's bits differ between the modes" % (r[0], i))
        checked["modes"] = checked.get("modes", 0) + 1
        figures.append(dict(row=r[0], position=i, mode="both", modes_far=max(far.values()), k8_same_bits=bool(k8)))
    print(json.dumps({"failures": failures, "figures": figures, "rows": n, "checked": checked,
                      "kinds": kinds, "form": B.fam.k1_form()}))


def main(argv):
    import shutil
    import tempfile

    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    if "--cpu" in argv:
        from tests import ext_deep_cases as xd
        print(xd.report(xd.build(opt("--cpu"), int(opt("--jobs", "1")))))
        return 0
    work = tempfile.mkdtemp(prefix="lh_ext_deep_")
    try:
        run_gpu(opt("--gpu"), opt("--family"), work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
