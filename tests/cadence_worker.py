"""Helper of tests/test_gpu_rescaling_cadence.py and tests/test_cadence_cases_cpu.py: the rows of tests/cadence_cases.py made
concrete -- their exact side and references on the CPU, and, in a process of its own per K1 hook set (the launcher's hooks
are environment variables read once per process), their evaluation through the C ABI.

  python tests/cadence_worker.py --cpu DIR [--profile FILE] [--jobs N]
                                                               CPU: DIR/cadence_<family>.npz (per row: exact emissions and
                                                               per-rate values, the references of the log-likelihood, the C
                                                               restatement's deviation d_C, the numpy oracle's finiteness)
                                                               and the builder's figures as text
  python tests/cadence_worker.py --gpu DIR --tag NAME          GPU: every row in both range modes under the hooks of this
                                                               process's environment, row independence, K6b, K3;
                                                               DIR/gpu_<NAME>.npz and one JSON line
                                                               {"forms": .., "failures": [..], "figures": [..]}"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FAMILY = "cad190"
FAMILIES = ("cad190", "cmp180")
GROUPS = ("extended", "independence", "candidates", "default", "asr")
N_CANDIDATES = 6


def cpu_side(out_dir, workdir, profile=None, jobs=1):
    """Builds and checks every row of every family (tests/cadence_cases.py), measures the references against each other and
    writes DIR/cadence_<family>.npz.  Returns (text of the profile, dict of figures per row)."""
    from oracle import oracle_c
    from tests import cadence_cases as cc
    from tests import extreme_worker as xw
    families = cc.build_families(FAMILIES, workdir, jobs)
    figs, lines = {}, []
    os.makedirs(out_dir, exist_ok=True)
    for family in FAMILIES:
        h, built, seconds = families[family]
        R = cc.FAMILIES[family]["R"]
        ofam = oracle_c.COracleFamily(h, R)
        keep = {}
        lines.append("Rescaling cadence rows (tests/cadence_cases.py), CPU side: family %s, %d leaves, R = %d, %d xMSA columns; exact "
                     "side and restatements of its %d rows: %.1f s" % (family, h.msa.shape[0], R, h.xmsa.shape[1], len(built), seconds))
        lines.append("dev_*: largest |restated / exact - 1| of the per-rate site likelihood over the live categories of all "
                     "columns; w = walk ops between two rescaling tests (one rescaling per test at w = 1), until = after every op, "
                     "rescaled until the largest entry is back at 2^-256")
        for row, a in built:
            name, x = row[0], a["exact"]
            sample, _ = cc.sample_of(row)
            l2 = a["log2_emission"]
            ref = cc.mp_loglik(h, l2)
            with np.errstate(all="ignore"):
                ident = cc.reference_loglik(h, l2)
                tree = [(x["children"], x["root"], x["brlen"])]
                c_ext = float(ofam.eval(tree, [sample["er"]], [sample["pi"]], [sample["alpha"]], extended=True)[0])
                numpy_ll = xw.oracle_results(h, sample, R)["loglik"]
            d_ident = abs(ident - ref) / abs(ref) if np.isfinite(ident) else np.inf
            d_c = abs(c_ext - ref) / abs(ref)
            f = dict(cls=row[2], family=family, seconds=seconds, loglik=ref, identity=ident, d_identity=d_ident, c_ext=c_ext, d_c=d_c,
                     numpy_finite=bool(np.isfinite(numpy_ll)),
                     dev_w1=a["dev"]["w1"], dev_w4=a["dev"]["w4"], dev_w4_no_tables=a["dev"]["w4_no_tables"], dev_w1_flush=a["dev"]["w1_flush"],
                     dev_u1=a["dev"]["u1"], dev_u1_no_tables=a["dev"]["u1_no_tables"], dev_u1_flush=a["dev"]["u1_flush"],
                     zeroed_w1=a["zeroed"]["w1"], join_low_w1=a["join_low_w1"], join_low_u1=a["join_low_u1"], depth=a["depth"],
                     zeroed_w4=a["zeroed"]["w4"], zeroed_w4_no_tables=a["zeroed"]["w4_no_tables"], four_op_fall=a["four_op_fall"],
                     entry_fall=a["entry_fall"], low_w1=a["low_w1"], spread=a["spread"], deepest=a["deepest"], walk_ops=a["walk_ops"])
            figs[name] = f
            keep.update({"l2_" + name: l2, "pr_" + name: x["per_rate_log2"], "ll_" + name: ref, "dc_" + name: d_c,
                         "np_" + name: np.isfinite(numpy_ll), "rates_" + name: x["rates"]})
            lines.append("%-16s %-8s log-lik %.12f  identity+numpy %s (rel %.2g)  oc_eval_batch_ext %.12f (d_C %.2g)  numpy oracle %s" %
                         (name, row[2], ref, "%.12f" % ident if np.isfinite(ident) else "not finite", d_ident, c_ext, d_c,
                          "finite" if f["numpy_finite"] else "not finite"))
            lines.append("%-16s          deepest deep column 2^%.1f  dev_w1 %.2g  dev_w4 %.2g (no tables %.2g)  dev_w1 with subnormals "
                         "flushed %.2g  zeroed under w4: %s (no tables: %s)" %
                         ("", a["deepest"], f["dev_w1"], f["dev_w4"], f["dev_w4_no_tables"], f["dev_w1_flush"], f["zeroed_w4"], f["zeroed_w4_no_tables"]))
            lines.append("%-16s          dev_until %.2g (no tables %.2g, subnormals flushed %.2g)  zeroed under w1: %s  smallest largest entry an "
                         "op left: w1 2^%.0f, until 2^%.0f; stack depth %d" %
                         ("", f["dev_u1"], f["dev_u1_no_tables"], f["dev_u1_flush"], f["zeroed_w1"], f["join_low_w1"], f["join_low_u1"], f["depth"]))
            lines.append("%-16s          four-op fall of the largest entry %.0f binades, of any entry that can reach the result %.0f; "
                         "smallest positive entry of the every-op walk 2^%.0f; allele spread %.0f bits; %d walk ops" %
                         ("", a["four_op_fall"], a["entry_fall"], a["low_w1"], a["spread"], a["walk_ops"]))
        np.savez(os.path.join(out_dir, "cadence_%s.npz" % family), **keep)
    text = "\n".join(lines) + "\n"
    if profile:
        with open(profile, "w") as f_:
            f_.write(text)
    return text, figs


def ll_bound(cls, d_c):
    """test_gpu_parity.compare's log-likelihood bound, widened to 8 d_C where the double-precision C restatement is itself
    further than that from exact -- on the control and deep rows.  On the lossy and zeroed rows oc_eval_batch_ext is no
    restatement of the formula: it keeps ONE scaler per site for all rate categories (libpll's per-site scaling), the
    saturated category holds the scaler while the live one underflows, and it is 0.2 to 0.4 off; the bound there stays
    compare's own."""
    return max(1e-12, 8.0 * float(d_c)) if cls in ("control", "deep", "compound_control") else 1e-12


def candidates(h, sample, R):
    """A few naive sequences of finite prior: the numpy oracle's own draws on a control row."""
    with np.errstate(all="ignore"):
        h.initialize_phylo_parameters(sample["tree"], sample["er"], sample["pi"], sample["alpha"], R, is_path=False)
        h.initialize_phylo_emission()
        h.log_likelihood()
        seen = {}
        for _ in range(40):
            seen.setdefault(h.sample_naive_sequence(), None)
            if len(seen) == N_CANDIDATES:
                break
    return np.array([["ACGTN".index(c) for c in s] for s in seen], dtype=np.uint8)


def run_gpu(out_dir, tag, workdir):
    """Every family in turn (this process's hooks hold for all of them); the families' rows in one report."""
    import linearham_amd
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    forms, failures, figures, keep, n_rows = {}, {k: [] for k in GROUPS}, [], {}, 0
    for family in FAMILIES:
        fo, fl, fg, kp, n = run_gpu_family(hip, out_dir, family, os.path.join(workdir, family))
        forms.setdefault("families", {})[family] = fo
        for k in GROUPS:
            failures[k] += fl[k]
        figures += fg
        keep.update({"%s_%s" % (k, family): v for k, v in kp.items()})
        if family == FAMILY:                   # (cad190's also under the names they had before there was a second family)
            forms.update(fo)
            keep.update(kp)
        n_rows += n
    np.savez(os.path.join(out_dir, "gpu_%s.npz" % tag), **keep)
    print(json.dumps({"forms": forms, "failures": failures, "figures": figures, "rows": n_rows}))


def run_gpu_family(hip, out_dir, family, workdir):
    import linearham_amd
    from tests import cadence_cases as cc
    from tests import desc_builder as db
    from tests import test_gpu_parity as tp
    os.makedirs(workdir, exist_ok=True)
    x = np.load(os.path.join(out_dir, "cadence_%s.npz" % family))
    h = cc.load_family(family, workdir)
    R = cc.FAMILIES[family]["R"]
    rows = [r for r in cc.ROWS if r[1] == family]
    samples = [cc.sample_of(r)[0] for r in rows]
    sched = [cc.schedule(h, s) for s in samples]
    T, depth = sched[0][0], max(s[5] for s in sched)
    ops, brl = np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched])
    er, pi, al = [s["er"] for s in samples], [s["pi"] for s in samples], [s["alpha"] for s in samples]
    failures, figures, keep, forms = {k: [] for k in GROUPS}, [], {}, {}
    site = cc.kc.column_sites(h)
    desc = db.build_family_desc(h)

    def note(group, cond, text):
        if not cond:
            failures[group].append(text)

    # ---- extended range: all rows in one call, against the reference; then every row alone and as row 1 of two
    fam = linearham_amd.Family(desc, hip)
    fam.set_extended_range(True)
    ll_ext, res_ext = fam.eval_batch(T, depth, ops, brl, er, pi, al, R, want=("scaler_counts",))
    forms["extended"] = fam.k1_form()
    keep["ll_ext"], keep["sc_ext"] = ll_ext, res_ext["scaler_counts"]
    for i, r in enumerate(rows):
        ref, bound = float(x["ll_" + r[0]]), ll_bound(r[2], x["dc_" + r[0]])
        d = abs(ll_ext[i] - ref) / abs(ref) if np.isfinite(ll_ext[i]) else float("inf")
        figures.append(dict(row=r[0], family=family, cls=r[2], loglik_ext=float(ll_ext[i]), reference=ref, d_ll_ext=d, bound=bound))
        note("extended", d <= bound, "%s [%s]: extended-range log-likelihood %.15g, reference %.15g: %.3g relative, bound %.3g" %
             (r[0], forms["extended"], ll_ext[i], ref, d, bound))
    for i, r in enumerate(rows):
        one, _ = fam.eval_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], al[i:i + 1], R)
        j = (i + 1) % len(rows)
        two, _ = fam.eval_batch(T, depth, ops[[j, i]], brl[[j, i]], [er[j], er[i]], [pi[j], pi[i]], [al[j], al[i]], R)
        same = np.array([one[0], two[1]]).view(np.uint64) == np.array([ll_ext[i]] * 2).view(np.uint64)
        note("independence", bool(same.all()), "%s: extended range, not bit-identical alone / as row 1 of two: %r %r %r" % (r[0], ll_ext[i], one[0], two[1]))

    # ---- K6b in extended range: log_cand - prior + loglik = sum over sites of log E(s_t, t), per column exact
    ctrl = next(i for i, r in enumerate(rows) if r[2] in ("control", "compound_control"))
    cands = candidates(h, samples[ctrl], R)
    prior = hip.set_candidates(fam, cands, n_sites=h.msa.shape[1])
    res_c = hip.eval_candidates_batch(fam, T, depth, ops, brl, er, pi, al, R, len(cands), want=("loglik", "log_cand"))
    for i, r in enumerate(rows):
        l2, worst_c = x["l2_" + r[0]], 0.0
        for k, s in enumerate(cands):
            want = cc.LN2 * float(sum(l2[h.xmsa_ids[(int(b), t)]] for t, b in enumerate(s)))
            got = res_c["log_cand"][i, k] - prior[k] + res_c["loglik"][i]
            tol = 1e-10 + 1e-13 * abs(res_c["loglik"][i])                 # test_gpu_naive_probs._tol
            d = abs(got - want) if np.isfinite(got) else float("inf")
            worst_c = max(worst_c, d)
            note("candidates", np.isfinite(prior[k]) and d <= tol, "%s candidate %d: log_cand - prior + loglik %.15g, exact sum of log E %.15g "
                 "(off by %.3g, tolerance %.3g)" % (r[0], k, got, want, d, tol))
        figures[i]["d_candidates"] = worst_c
    fam.close()

    # ---- default mode: compare() on the control rows, the numpy oracle's non-finite mask, exact zeros
    with np.errstate(all="ignore"):
        desc_d, ll_def, res_def, ref_def = tp.run_family(hip, h, samples, R)
    forms["default"] = tp.LAST_RUN["form"]
    keep["ll_def"], keep["sc_def"], keep["em_def"] = ll_def, res_def["scaler_counts"], res_def["xmsa_emission"]
    for i, r in enumerate(rows):
        l2 = x["l2_" + r[0]]
        tiny = l2 < np.log2(1e-308)
        figures[i]["loglik_default"] = float(ll_def[i]) if np.isfinite(ll_def[i]) else repr(float(ll_def[i]))
        note("default", bool(np.all(res_def["xmsa_emission"][i][tiny] == 0)), "%s: an exact emission below 1e-308 is not 0 in default mode" % r[0])
        note("default", bool(np.isfinite(ll_def[i])) == bool(np.isfinite(ref_def[i]["loglik"])) == bool(x["np_" + r[0]]),
             "%s: default-mode log-likelihood %r, the numpy oracle's %r" % (r[0], ll_def[i], ref_def[i]["loglik"]))
        if r[2] in ("control", "compound_control"):
            try:
                tp.compare(h, desc_d, ll_def[i:i + 1], {k: v[i:i + 1] for k, v in res_def.items()}, ref_def[i:i + 1])
                note("default", abs(ll_def[i] - float(x["ll_" + r[0]])) <= ll_bound(r[2], x["dc_" + r[0]]) * abs(ll_def[i]),
                     "%s: default mode against the reference: %r %r" % (r[0], ll_def[i], float(x["ll_" + r[0]])))
            except AssertionError as err:
                failures["default"].append("%s [%s]: compare: %s" % (r[0], forms["default"], " ".join(str(err).split())[:500]))

    # ---- K3 on the lossy, zeroed, compound_lossy and compound_zeroed rows: every deep site draws the category the exact per-rate values make certain
    picked = [i for i, r in enumerate(rows) if r[2] in ("lossy", "zeroed", "compound_lossy", "compound_zeroed")]
    L = h.msa.shape[1]
    col_of = {}
    for c in range(len(site)):
        col_of.setdefault(int(site[c]), c)
    naive = np.array([[int(h.xmsa[0, col_of[t]]) for t in range(L)]] * len(picked), dtype=np.uint8)
    fam = linearham_amd.Family(desc, hip)
    rates = np.stack([x["rates_" + rows[i][0]] for i in picked])
    anc, choice = fam.asr_batch(T, depth, ops[picked], brl[picked], [er[i] for i in picked], [pi[i] for i in picked], rates, naive,
                                seed=4711, first_sample=0)
    forms["asr"] = fam.k1_form()
    fam.close()
    for n_, i in enumerate(picked):
        pr = x["pr_" + rows[i][0]]
        checked = wrong = 0
        for t in cc.deep_sites(family):
            v = pr[:, col_of[t]]
            best = int(np.argmax(v))
            if np.all(np.delete(v, best) <= v[best] - cc.LIVE_BITS):
                checked += 1
                wrong += int(choice[n_][t]) != best
                note("asr", int(choice[n_][t]) == best, "%s [%s]: K3 drew rate category %d on deep site %d; exact per-rate log2 %s" %
                     (rows[i][0], forms["asr"], int(choice[n_][t]), t, v.tolist()))
        note("asr", checked >= 3, "%s: fewer than three deep sites with a certain category" % rows[i][0])
        figures[i]["asr_sites"], figures[i]["asr_wrong"] = checked, wrong
    return forms, failures, figures, keep, len(rows)


def main(argv):
    import tempfile
    import shutil

    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    work = tempfile.mkdtemp(prefix="lh_cadence_")
    try:
        if "--cpu" in argv:
            text, _ = cpu_side(opt("--cpu"), work, opt("--profile"), int(opt("--jobs", "1")))
            print(text)
        else:
            run_gpu(opt("--gpu"), opt("--tag", "default"), work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
