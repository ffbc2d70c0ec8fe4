"""Helper of tests/test_gpu_k2b_dj_quad.py (its own process: the hook LH_K2B_DJ_PAIR is an environment variable read once
per process).

    k2b_dj_quad_worker.py REFERENCES.pkl OUT.npz

REFERENCES.pkl holds, per family, what tests/k2_scaling_cases.py built on the CPU (oracle object, cases, references) and the
least number of rows of its one call.  For every family, with the extended-range mode off and then on:
  * all cases run as ONE lh_forward_batch call in wave_order's row order -- every wave of four samples holds one deep case
    and three `base` rows, the deep case in each of the four positions in turn, so that on the rows where the deep case
    rescales it is the only sample of its wave that does -- and every distinct case is checked against the identity and the
    numpy oracle with the checks and bounds of tests/k2_forms_worker.py (log-likelihood 1e-12, forward entries 1e-9, counts
    exactly);
  * the first n rows of that order are run again as calls of n = 1, 2, 3, 4, 5, 7, 8, 9 (absent samples in every position
    of a wave) and 15, 16, 17 (across the boundary of a workgroup of four waves), every distinct case alone, and must come
    back bit for bit;
  * a family whose one call has 129 rows or more (workgroups of 8 and 16 waves: 32 and 64 samples each, so that the call
    spans three of the largest) likewise at n = 31, 32, 33, 63, 64, 65.
Prints one JSON line {family: {mode: {form, dj_samples, dj_waves, n, deviation}}} and writes every row of the one call to
OUT.npz for the parent's comparison between the two children."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
WIDE_SIZES = (31, 32, 33, 63, 64, 65)     # across the boundaries of workgroups of 8 and 16 waves


def wave_order(cases, n_min=33):
    """Row order of the one call: wave w = rows 4w .. 4w + 3 holds deep case w (cyclically) in position w % 4 and `base` in
    the other three; then waves of four different deep cases (four different row factors in one wave); at least n_min rows
    and a last wave of one sample."""
    deep = [c.name for c in cases if c.name != "base"]
    order = []
    w = 0
    while w < len(deep) or len(order) < n_min - 1:
        wave = ["base"] * 4
        wave[w % 4] = deep[w % len(deep)]
        order += wave
        w += 1
    for i in range(0, len(deep) - 3, 4):
        order += deep[i:i + 4]
    return order + [deep[0]]


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def run_mode(hip, fw, tp, h, desc, cases, refs, n_min, ext, fail):
    import linearham_amd
    fam = linearham_amd.Family(desc, hip)
    if ext:
        fam.set_extended_range(True)
    want = ("forward", "scaler_counts")
    by = {c.name: c for c in cases}
    order = wave_order(cases, n_min)
    em = np.stack([by[n].em for n in order])
    ll, res = fam.forward_batch(em, want=want)
    fwd, sco = res["forward"], res["scaler_counts"]
    info = {"form": fam.k2_form(), "dj_samples": fam.k2_dj_samples(), "dj_waves": fam.k2_dj_waves(), "n": len(order)}
    dev = {"loglik": 0.0, "forward": 0.0, "counts_equal": True, "loglik_by_case": {}}
    first = {}
    for i, name in enumerate(order):
        j = first.setdefault(name, i)
        if j != i and _bits(ll[i:i + 1], fwd[i], sco[i]) != _bits(ll[j:j + 1], fwd[j], sco[j]):
            fail("%s: rows %d and %d of the one call differ" % (name, j, i))
    for name, i in first.items():
        (fw.check_extended if ext else fw.check_default)(tp, h, desc, by[name], refs[name], float(ll[i]), fwd[i], sco[i], dev,
                                                         fail)
    for n in SIZES + (WIDE_SIZES if len(order) >= 129 else ()):
        l1, r1 = fam.forward_batch(em[:n], want=want)
        if _bits(l1, r1["forward"], r1["scaler_counts"]) != _bits(ll[:n], fwd[:n], sco[:n]):
            fail("the first %d rows differ when they are the whole call" % n)
    for name, i in first.items():
        l1, r1 = fam.forward_batch(by[name].em[None], want=want)
        if _bits(l1[0:1], r1["forward"][0], r1["scaler_counts"][0]) != _bits(ll[i:i + 1], fwd[i], sco[i]):
            fail("%s: differs when run alone (n = 1)" % name)
    if (fam.k2_dj_samples(), fam.k2_dj_waves()) != (info["dj_samples"], info["dj_waves"]):
        fail("the D-J layout changed with the batch size")
    fam.close()
    info["deviation"] = {"loglik": dev["loglik"], "forward": dev["forward"]}
    return info, (ll, fwd, sco)


def main(argv):
    ref_path, out_path = argv[0], argv[1]
    import linearham_amd
    from tests import desc_builder as db
    from tests import k2_forms_worker as fw
    from tests import test_gpu_parity as tp
    with open(ref_path, "rb") as f:
        built = pickle.load(f)
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    report, arrays, problems = {}, {}, []
    for name, (h, cases, refs, n_min) in built.items():
        desc = db.build_family_desc(h)
        report[name] = {}
        for ext in (False, True):
            mode = "extended" if ext else "default"
            info, (ll, fwd, sco) = run_mode(hip, fw, tp, h, desc, cases, refs, n_min, ext,
                                            lambda msg: problems.append("%s/%s: %s" % (name, mode, msg)))
            report[name][mode] = info
            key = "%s|%s|" % (name, mode)
            arrays[key + "ll"], arrays[key + "forward"], arrays[key + "counts"] = ll, fwd, sco
    np.savez(out_path, **arrays)
    print(json.dumps(report))
    if problems:
        raise AssertionError("%d checks failed:\n%s" % (len(problems), "\n".join(problems[:40])))


if __name__ == "__main__":
    main(sys.argv[1:])
