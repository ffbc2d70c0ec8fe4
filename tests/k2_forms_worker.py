"""Helper of tests/test_gpu_k2_forms.py (its own process: the K2 form hooks LH_K2B_NO_PAIR / LH_K2B_VD_SINGLE are
environment variables read once per process, LH_K2A_DIRECT when a family is created).

    k2_forms_worker.py REFERENCES.pkl OUT.npz [--report] family...

REFERENCES.pkl holds, per family, what tests/k2_scaling_cases.py built on the CPU: the oracle object, the cases and their
references (the parent builds them once for all children).  For every family named, with the extended-range mode off and
then on, all cases run as ONE lh_forward_batch call (k2_scaling_cases.batch_order: `base` and a deep case alternate as the
two samples of a pair-form wave, in both orders; an odd number of rows, more than two K2b workgroups) and are checked as
the module docstring of test_gpu_k2_forms.py lists; every row is then run again alone and as the second row of a call of
two, and must come back bit for bit.  Prints one JSON line {family: {mode: {form, consensus_sets, n, deviation}}} and writes
every row's results to OUT.npz for the parent's comparison between children.  --report (development) prints the deviations
and the failed checks instead of raising."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RTOL_LOGLIK = 1e-12     # compare()'s bound (tests/test_gpu_parity.py)
RTOL_FORWARD = 1e-9


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _rel(a, b):
    """largest |a - b| / |b| over the entries where b != 0; inf where exactly one of the two is zero or either is not finite"""
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    if a.size == 0:
        return 0.0
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))) or np.any((a == 0) != (b == 0)):
        return float("inf")
    m = b != 0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def _pairs(ex, ref):
    """(name, device rows, device counts, oracle rows, oracle counts): every forward array as a list of rows, each with the
    cumulative ScaleMatrix count that belongs to it"""
    for k in ex:
        if not k.endswith("_forward"):
            continue
        if k.endswith("junction_forward"):
            ck = k.replace("_forward", "_scaler_counts")
            yield k, list(ex[k]), list(ex[ck]), list(ref[k]), list(ref[ck])
        else:
            ck = k.replace("_forward", "_scaler_count")
            yield k, [ex[k]], [ex[ck]], [ref[k]], [ref[ck]]


def check_default(tp, h, desc, case, ref, ll, fwd, sco, dev, fail):
    if case.expect == "overflow":
        if np.isfinite(ll):
            fail("%s: finite on the device (%r), the reference overflows" % (case.name, ll))
        return
    want = ref["identity"]
    d = abs(ll - want) / abs(want)
    dev["loglik"] = max(dev["loglik"], d)
    dev["loglik_by_case"][case.name] = d
    if not d <= RTOL_LOGLIK:
        fail("%s: loglik %r, identity %r (%.2e)" % (case.name, ll, want, d))
    ex = tp.expand_forward(h, desc, fwd, sco)
    for k in ex:
        if "scaler" in k:
            if not np.array_equal(np.asarray(ex[k]), np.asarray(ref["oracle"][k])):
                dev["counts_equal"] = False
                fail("%s: %s %r, oracle %r" % (case.name, k, ex[k], ref["oracle"][k]))
        else:
            d = _rel(ex[k], ref["oracle"][k])
            dev["forward"] = max(dev["forward"], d)
            if not d <= RTOL_FORWARD:
                fail("%s: %s deviates %.2e" % (case.name, k, d))


def check_extended(tp, h, desc, case, ref, ll, fwd, sco, dev, fail):
    want = ref["identity"]
    d = abs(ll - want) / abs(want) if np.isfinite(ll) else float("inf")
    dev["loglik"] = max(dev["loglik"], d)
    dev["loglik_by_case"][case.name] = d
    if not d <= RTOL_LOGLIK:
        fail("%s: loglik %r, identity %r (%.2e)" % (case.name, ll, want, d))
    if case.expect == "overflow":
        return  # (the reference's forward arrays are not finite: nothing to compare the rows with)
    ex = tp.expand_forward(h, desc, fwd, sco)
    for k, rows, counts, orows, ocounts in _pairs(ex, ref["oracle"]):
        for i, (a, ca, b, cb) in enumerate(zip(rows, counts, orows, ocounts)):
            a, b = np.asarray(a, float), np.asarray(b, float)
            # value * 2^(-256 count) on both sides: the device entry in the oracle's scaling
            a2 = np.ldexp(a, 256 * (int(cb) - int(ca)))
            gone = (a == 0) & (b > 0)
            # the mode rescales a row by its largest entry and lets entries far below it underflow: 2^-768 and more
            if gone.any() and not np.all(b[gone] <= np.ldexp(b.max(), -768)):
                fail("%s: %s row %d: a zero on the device where the oracle holds %.3e of its row's largest entry"
                     % (case.name, k, i, float((b[gone] / b.max()).max())))
            m = ~gone
            d = _rel(a2[m], b[m])
            dev["forward"] = max(dev["forward"], d)
            if not d <= RTOL_FORWARD:
                fail("%s: %s row %d deviates %.2e" % (case.name, k, i, d))


def run_mode(hip, tp, kc, h, desc, cases, refs, ext, fail):
    import linearham_amd
    fam = linearham_amd.Family(desc, hip)
    if ext:
        fam.set_extended_range(True)
    want = ("forward", "scaler_counts")
    by = {c.name: c for c in cases}
    order = kc.batch_order(cases)
    ll, res = fam.forward_batch(np.stack([by[n].em for n in order]), want=want)
    info = {"form": fam.k2_form(), "consensus_sets": int(fam.consensus_sets), "n": len(order)}
    fwd, sco = res["forward"], res["scaler_counts"]
    dev = {"loglik": 0.0, "forward": 0.0, "counts_equal": True, "loglik_by_case": {}}
    first = {}
    for i, name in enumerate(order):
        j = first.setdefault(name, i)
        if j != i and _bits(ll[i:i + 1], fwd[i], sco[i]) != _bits(ll[j:j + 1], fwd[j], sco[j]):
            fail("%s: rows %d and %d of the one call differ" % (name, j, i))
    for name, i in first.items():
        (check_extended if ext else check_default)(tp, h, desc, by[name], refs[name], float(ll[i]), fwd[i], sco[i], dev, fail)
    # isolation: the same emission vector alone, and as the second sample of a wave behind `base` -- the half-wave
    # reductions and the `valid` lane of the pair forms must not let a neighbour, or its absence, show
    for name, i in first.items():
        l1, r1 = fam.forward_batch(by[name].em[None], want=want)
        l2, r2 = fam.forward_batch(np.stack([by["base"].em, by[name].em]), want=want)
        mine = _bits(ll[i:i + 1], fwd[i], sco[i])
        if _bits(l1[0:1], r1["forward"][0], r1["scaler_counts"][0]) != mine:
            fail("%s: differs when run alone (n = 1)" % name)
        if _bits(l2[1:2], r2["forward"][1], r2["scaler_counts"][1]) != mine:
            fail("%s: differs as row 1 of a call of two" % name)
    fam.close()
    info["deviation"] = dev
    rows = {name: (ll[i], fwd[i], sco[i]) for name, i in first.items()}
    return info, rows


def main(argv):
    report_only = "--report" in argv
    args = [a for a in argv if not a.startswith("--")]
    ref_path, out_path, names = args[0], args[1], args[2:]
    import linearham_amd
    from tests import desc_builder as db
    from tests import k2_scaling_cases as kc
    from tests import test_gpu_parity as tp
    with open(ref_path, "rb") as f:
        built = pickle.load(f)
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    report, arrays, problems = {}, {}, []
    for name in names:
        h, cases, refs = built[name]
        desc = db.build_family_desc(h)
        report[name] = {}
        for ext in (False, True):
            mode = "extended" if ext else "default"
            info, rows = run_mode(hip, tp, kc, h, desc, cases, refs, ext,
                                  lambda msg: problems.append("%s/%s: %s" % (name, mode, msg)))
            report[name][mode] = info
            for case, (ll, fwd, sco) in rows.items():
                key = "%s|%s|%s|" % (name, mode, case)
                arrays[key + "ll"], arrays[key + "forward"], arrays[key + "counts"] = np.array([ll]), fwd, sco
    np.savez(out_path, **arrays)
    if report_only:
        report["problems"] = problems
    print(json.dumps(report))
    if problems and not report_only:
        raise AssertionError("%d checks failed:\n%s" % (len(problems), "\n".join(problems[:40])))


if __name__ == "__main__":
    main(sys.argv[1:])
