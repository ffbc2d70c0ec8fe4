"""Helper of tests/test_gpu_k4_draws.py (its own process: LH_K4_NO_SAVE is an environment variable read once per process).

    k4_draws_worker.py REFERENCES.pkl OUT.npz [--report] family...

REFERENCES.pkl holds, per family, what the parent built on the CPU (tests/k4_draw_cases.py): the oracle object, the rows,
the identity log-likelihood of every case and the tier-2 states.  For every family named, with the extended-range mode off
and then on, all rows run as ONE lh_sample_forward_batch call and are checked as the module docstring of
test_gpu_k4_draws.py lists.  Prints one JSON line {family: {mode: {...}}} and writes every call's states to OUT.npz for the
parent's comparison between children.  --report (development) prints the failed checks instead of raising."""
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RTOL_LOGLIK = 1e-12
WANT = ("forward", "scaler_counts")


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _call(fam, rows, sel):
    ll, st, res = fam.sample_forward_batch(rows.em[sel], rows.words[sel], want=WANT)
    return ll, st, res["forward"], res["scaler_counts"]


def run_mode(hip, tp, k4, h, desc, tables, rows, identity, tier2, ext, default_run, fail):
    import linearham_amd
    fam = linearham_amd.Family(desc, hip)
    fam.set_sampler(*tables)
    if ext:
        fam.set_extended_range(True)
    assert hip.lib.lh_sample_words(fam.handle) == rows.n_words, (hip.lib.lh_sample_words(fam.handle), rows.n_words)
    n = rows.n
    everything = np.arange(n)
    ll, st, fwd, sco = _call(fam, rows, everything)
    info = {"n": n, "form": fam.k2_form(), "saved": bool(k4.saves_weights(h))}
    # 1. the forward sweep is lh_forward_batch's, bit for bit; the log-likelihood against the identity
    ll_f, res_f = fam.forward_batch(rows.em, want=WANT)
    if _bits(ll, fwd, sco) != _bits(ll_f, res_f["forward"], res_f["scaler_counts"]):
        fail("log-likelihood, forward arrays or counts differ from lh_forward_batch's on the same emissions")
    worst = 0.0
    for r, (c, p) in enumerate(rows.layout):
        case = rows.cases[c]
        if case.expect == "overflow" and not ext:
            if np.isfinite(ll[r]):
                fail("row %d (%s): finite on the device (%r), the reference overflows" % (r, case.name, ll[r]))
            continue
        want = identity[case.name]
        d = abs(ll[r] - want) / abs(want) if np.isfinite(ll[r]) else float("inf")
        worst = max(worst, d)
        if not d <= RTOL_LOGLIK:
            fail("row %d (%s): loglik %r, identity %r (%.2e)" % (r, case.name, ll[r], want, d))
    info["loglik"] = worst
    # 2. tier 1 on every row (the oracle's dense draws on this row's own forward arrays), tier 2 on its rows
    recorded, t1_bad, t2_bad, finite_rows = [], [], [], []
    for r in range(n):
        ex = tp.expand_forward(h, desc, fwd[r], sco[r])
        want, used, draws = k4.draws_on_forward(h, ex, rows.words[r], record=not ext)
        recorded.append(draws)
        finite_rows.append(bool(np.all(np.isfinite(fwd[r]))))
        if used != rows.n_words:
            fail("row %d: the reference consumed %d words, not %d" % (r, used, rows.n_words))
        if not np.array_equal(st[r], want):
            t1_bad.append(r)
            at = int(np.nonzero(st[r] != want)[0][0])
            fail("row %d (case %s, pattern %s): states differ from tier 1 from entry %d on: device %s, reference %s"
                 % (r, rows.cases[rows.layout[r][0]].name, k4.PATTERNS[rows.layout[r][1]], at, st[r][at:at + 4].tolist(),
                    want[at:at + 4].tolist()))
        if r in tier2 and not np.array_equal(st[r], tier2[r]):
            t2_bad.append(r)
            fail("row %d (case %s, pattern %s): states differ from tier 2 (the oracle end to end)"
                 % (r, rows.cases[rows.layout[r][0]].name, k4.PATTERNS[rows.layout[r][1]]))
    info.update(tier1_rows=n, tier1_bad=t1_bad, tier2_rows=len(tier2), tier2_bad=t2_bad,
                nonfinite_rows=int(n - sum(finite_rows)))
    if not ext:
        info["classes"] = k4.classes(h, rows, recorded)
    # 3. layout independence, bit for bit: reversed, rotated by 1, 2 and 3 rows (every row changes its group and its wave
    #    mates), the first 16 rows each alone
    def same(name, sel):
        l2, s2, f2, c2 = _call(fam, rows, sel)
        for i, r in enumerate(sel):
            if _bits(l2[i:i + 1], s2[i], f2[i], c2[i]) != _bits(ll[r:r + 1], st[r], fwd[r], sco[r]):
                what = [k for k, a, b in (("loglik", l2[i:i + 1], ll[r:r + 1]), ("states", s2[i], st[r]),
                                          ("forward", f2[i], fwd[r]), ("counts", c2[i], sco[r])) if _bits(a) != _bits(b)]
                fail("row %d differs in the call %s: %s" % (r, name, ", ".join(what)))
    same("reversed", everything[::-1])
    for k in (1, 2, 3):
        same("rotated by %d" % k, np.roll(everything, k))
    for r in range(16):
        same("of row %d alone" % r, np.array([r]))
    # 4. extended range: the states of the default mode on every row whose default forward arrays are finite
    if ext:
        d_st, d_finite = default_run
        differ = [r for r in range(n) if d_finite[r] and not np.array_equal(st[r], d_st[r])]
        info["equal_default_rows"] = int(sum(d_finite)) - len(differ)
        for r in differ:
            fail("row %d: extended-range states differ from the default mode's" % r)
        if not all(finite_rows):
            fail("non-finite forward arrays in the extended-range mode")
    fam.close()
    return info, st, finite_rows


def main(argv):
    report_only = "--report" in argv
    args = [a for a in argv if not a.startswith("--")]
    ref_path, out_path, names = args[0], args[1], args[2:]
    import linearham_amd
    from tests import desc_builder as db
    from tests import k4_draw_cases as k4
    from tests import test_gpu_parity as tp
    from tests import viterbi_oracle as vo
    with open(ref_path, "rb") as f:
        built = pickle.load(f)
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    report, arrays, problems = {}, {}, []
    for name in names:
        h, rows, identity, tier2 = built[name]
        desc = db.build_family_desc(h)
        tables = vo.sampler_tables(h)
        report[name] = {}
        default_run = None
        for ext in (False, True):
            mode = "extended" if ext else "default"
            t0 = time.time()
            info, st, finite = run_mode(hip, tp, k4, h, desc, tables, rows, identity, tier2, ext, default_run,
                                        lambda msg: problems.append("%s/%s: %s" % (name, mode, msg)))
            info["seconds"] = round(time.time() - t0, 2)
            if not ext:
                default_run = (st, finite)
            report[name][mode] = info
            arrays["%s|%s|states" % (name, mode)] = st
    np.savez(out_path, **arrays)
    if report_only:
        report["problems"] = problems
    print(json.dumps(report))
    if problems and not report_only:
        raise AssertionError("%d checks failed:\n%s" % (len(problems), "\n".join(problems[:40])))


if __name__ == "__main__":
    main(sys.argv[1:])
