"""Every form of K2 (lh_forward.hip) at its rescaling edges, by design rather than by accident of the emissions.

K2b picks among four launch shapes (launch_junction_g: junction_vd2_kernel + junction_dj_kernel, two samples per wave with a
ScaleMatrix count per half; junction_vd_kernel + junction_dj_kernel beyond 256 V alleles; junction_kernel<GA, GB> for light
chains and for more than 32 D or J alleles; the hooks LH_K2B_NO_PAIR and LH_K2B_VD_SINGLE), K2a among four product walks
(fill_segments with its chunk fast path and its step-by-step path, fill_segments_wave, fill_consensus, fill_segments_ext)
and a per-sample fallback out of the consensus form (em_bad).  The wide germline sets pick the register chunks: GA = 1, 2,
4, 8, 16 for up to 64, 128, 256, 512, 1024 V alleles, GB = 1, 2, 4 for up to 64, 128, 256 D or J alleles, and K2a's gene
slots per thread (1, 2, 4 for up to 256, 512, 1024 alleles in a set); K2B below names a family for every GA of the pair
forms and of junction<GA,1>, for GB = 2 and 4 with GA below, equal to and above GB, and for a light chain with GB = 2.

Which branch a row takes depends on its emissions, and
lh_forward_batch takes the caller's: tests/k2_scaling_cases.py builds emission vectors that reach each branch, with a
reference that shares nothing with ScaleMatrix -- multiplying every column of alignment site t by 2^-k_t moves the
log-likelihood by exactly -ln 2 * sum(k) (checked on the oracle in tests/test_k2_scaling_cases_cpu.py).

One child process per hook setting (tests/k2_forms_worker.py).  Per family, extended-range mode off and then on, all cases
run as one call of an odd number of rows >= 17 in which `base` and a deep case alternate as the two samples of a wave:
  default mode    log-likelihood against the identity 1e-12; forward arrays against the numpy oracle on the same emissions
                  1e-9; every ScaleMatrix count exactly; `delta4` (the reference's pow(2^256, 4) = inf) not finite
  extended mode   every case, delta4 included, against the identity 1e-12 -- the independent reference this mode lacked;
                  forward entries as value * 2^(-256 count) against the oracle's 1e-9; an entry that is 0 on the device at
                  least 2^-768 below its row's largest in the oracle
  isolation       every row bit-identical to the same vector run alone and as row 1 of a call of two behind `base`
  form            lh_family_forward_form names the kernels the family and hook are meant to reach
and the parent compares the children per (family, mode, case): counts equal, log-likelihood 1e-12, forward arrays 1e-11 (the
bounds of test_consensus_products_equal_the_factor_walk between two forms), the `zero` rows of the default child bit for
bit those of the LH_K2A_DIRECT child (the per-sample fallback walks factor by factor)."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import k2_scaling_cases as kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "k2_forms_worker.py")
HOOKS = ("LH_K2B_NO_PAIR", "LH_K2B_VD_SINGLE", "LH_K2A_DIRECT")

# K2b's kernels per family: by itself, with one sample per wave (LH_K2B_NO_PAIR), with one sample per V-D wave
# (LH_K2B_VD_SINGLE); GA = ceil(V alleles / 64) rounded up to 1, 2, 4, 8, 16
K2B = {
    "toy": (r"vd2<1>\+dj", r"junction<1,1>", r"vd<1>\+dj"),
    "small_igh": (r"vd2<1>\+dj", r"junction<1,1>", r"vd<1>\+dj"),
    "small_igk": (r"junction<1,1>",) * 3,                                    # light chain: no D, one junction
    "igh_70_33_5": (r"junction<2,1>",) * 3,                                  # 33 D alleles: one wave per sample
    "igh_v260": (r"vd<8>\+dj", r"junction<8,1>", r"vd<8>\+dj"),              # more than 256 V alleles
    "igh_cons": (r"vd2<1>\+dj", r"junction<1,1>", r"vd<1>\+dj"),
    # the wide germline sets; GB = ceil(max(D alleles, J alleles) / 64) rounded up to 1, 2, 4
    "igh_v70": (r"vd2<2>\+dj", r"junction<2,1>", r"vd<2>\+dj"),
    "igh_v130_d30_j12": (r"vd2<4>\+dj", r"junction<4,1>", r"vd<4>\+dj"),       # the benchmark workload's kernels
    "igh_v520": (r"vd<16>\+dj", r"junction<16,1>", r"vd<16>\+dj"),
    "igh_d65": (r"junction<1,2>",) * 3,
    "igh_j130": (r"junction<1,4>",) * 3,                                      # GA < GB
    "igh_v130_d70": (r"junction<4,2>",) * 3,
    "igk_v70_j70": (r"junction<2,2>",) * 3,                                   # light chain with GB > 1
    "igh_v520_j130": (r"junction<16,4>",) * 3,
}
# gene slots per K2a thread (more than 256, more than 512 alleles in a set): 1 everywhere else
K2A_SLOTS = {"igh_v260": 2, "igh_v520": 4, "igh_v520_j130": 4}
# more than 64 D or J alleles: the small sets walk on the whole workgroup, not a wave each
SMALL_BY_BLOCK = ("igh_d65", "igh_j130", "igh_v130_d70", "igk_v70_j70", "igh_v520_j130")
SETTINGS = {
    "default": ({}, list(K2B)),
    "no_pair": ({"LH_K2B_NO_PAIR": "1"}, ["toy", "small_igh", "igh_v260", "igh_cons", "igh_v70", "igh_v130_d30_j12",
                                          "igh_v520"]),
    "vd_single": ({"LH_K2B_VD_SINGLE": "1"}, ["toy", "small_igh", "igh_cons", "igh_v70", "igh_v130_d30_j12"]),
    "k2a_direct": ({"LH_K2A_DIRECT": "1"}, ["toy", "small_igh", "igh_70_33_5", "igh_cons", "igh_v130_d30_j12", "igh_j130",
                                            "igk_v70_j70"]),
}


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """Cases and references of every family, built once on the CPU and handed to the children as a file."""
    work = tmp_path_factory.mktemp("k2_forms")
    built = {}
    for name in K2B:
        h = kc.load_family(name, work)
        _, cases = kc.build_cases(h, kc.SEEDS[name])
        refs = kc.references(h, cases)
        kc.check_conditions(h, cases, refs, need=kc.NEED[name])
        built[name] = (h, cases, refs)
    path = str(work / "references.pkl")
    with open(path, "wb") as f:
        pickle.dump(built, f)
    return {"path": path, "work": work, "built": built, "children": {}}


def _child(references, setting):
    """runs the child of one hook setting once per module; -> (report, arrays)"""
    done = references["children"]
    if setting not in done:
        hook, families = SETTINGS[setting]
        env = {k: v for k, v in os.environ.items() if k not in HOOKS}
        env.update(hook)
        out = str(references["work"] / (setting + ".npz"))
        r = subprocess.run([sys.executable, WORKER, references["path"], out] + families, capture_output=True, text=True,
                           timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, "%s\n%s" % (r.stdout[-2000:], r.stderr[-6000:])
        with np.load(out) as z:
            arrays = {k: z[k] for k in z.files}
        done[setting] = (json.loads(r.stdout.strip().splitlines()[-1]), arrays)
    return done[setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_k2_forms_at_the_rescaling_edges(references, setting):
    """the child's own checks (it exits nonzero when one fails), and the form each family ran in each mode"""
    report, _ = _child(references, setting)
    col = {"default": 0, "no_pair": 1, "vd_single": 2, "k2a_direct": 0}[setting]
    for family in SETTINGS[setting][1]:
        for mode in ("default", "extended"):
            info = report[family][mode]
            dev = info["deviation"]
            print("%s %s %s: %s, log-likelihood against the identity %.2e, forward arrays against the oracle %.2e"
                  % (setting, family, mode, info["form"], dev["loglik"], dev["forward"]))
            assert info["n"] >= 17 and info["n"] % 2 == 1
            ext = mode == "extended"
            # the extended-range mode walks every set with its counts (fill_segments_ext): no consensus form, no waves
            k2a = r"emission<%d,caller,(byte|index)%s> cons=%s small=%s" % (
                K2A_SLOTS.get(family, 1), ",ext" if ext else "", "0" if ext else r"\d+",
                "block" if ext or family in SMALL_BY_BLOCK else r"(wave|block)")
            pattern = k2a + r" \| " + K2B[family][col]
            assert re.fullmatch(pattern, info["form"]), (family, mode, info["form"], pattern)
            cons = int(re.search(r"cons=(\d+)", info["form"]).group(1))
            assert ext or cons == info["consensus_sets"]
            if setting == "k2a_direct":
                assert info["consensus_sets"] == 0 and cons == 0, (family, info)
            elif family == "igh_cons":
                assert info["consensus_sets"] & 2, "the V germline set of this family should be in consensus form"
            if not ext and info["consensus_sets"] == 0 and family not in SMALL_BY_BLOCK:
                assert "small=wave" in info["form"], (family, info["form"])   # at most 64 D and J alleles


def test_k2_forms_agree_with_each_other(references):
    """per (family, mode, case): any two children's ScaleMatrix counts equal, log-likelihoods within 1e-12, forward arrays
    within 1e-11; the `zero` rows of the default child bit for bit those of the LH_K2A_DIRECT child"""
    ran = {s: _child(references, s)[1] for s in SETTINGS}
    base = ran["default"]
    compared = 0
    for setting in ("no_pair", "vd_single", "k2a_direct"):
        other = ran[setting]
        for key in other:
            if not key.endswith("|ll"):
                continue
            stem = key[:-2]
            a, b = float(base[key][0]), float(other[key][0])
            assert np.isfinite(a) == np.isfinite(b), (setting, key, a, b)
            if not np.isfinite(a):
                continue
            assert abs(a - b) <= 1e-12 * abs(a), (setting, key, a, b)
            np.testing.assert_array_equal(base[stem + "counts"], other[stem + "counts"], err_msg=setting + " " + stem)
            np.testing.assert_allclose(other[stem + "forward"], base[stem + "forward"], rtol=1e-11, atol=0,
                                       err_msg=setting + " " + stem)
            compared += 1
    assert compared >= 100
    direct = ran["k2a_direct"]
    zero_rows = [k[:-2] for k in direct if k.endswith("|zero|ll")]
    assert any(k.startswith("igh_cons|default") for k in zero_rows)
    for stem in zero_rows:
        for part in ("ll", "forward", "counts"):
            assert base[stem + part].tobytes() == direct[stem + part].tobytes(), (stem, part)
