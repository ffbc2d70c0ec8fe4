"""K2b's D-J sweep with four samples per wave (junction_dj4_kernel, lh_forward.hip) against the two-sample form it replaces.

A family in the pair form with at most 32 D and 16 J alleles sweeps its D-J junctions with one DPP row of 16 lanes per
sample: lane = 16 * (sample in wave) + l, right gene l, left genes l and 16 + l (GL = 1 register slot for at most 16 D
alleles, 2 beyond).  Per sample the floating-point operations and their order are those of junction_pair, so every output
keeps its bits; LH_K2B_DJ_PAIR=1 puts junction_dj_kernel back, and lh_family_forward_dj_samples says which layout ran.

Families (tools.synth_family.Spec.small, (D alleles, J alleles)): (1, 1); (16, 16) GL = 1 and every right lane used;
(17, 16) the first with GL = 2; (32, 16) both limits; (30, 12) configs[2]'s counts on a small tree; (30, 17) keeps the
two-sample form (the diagnostic says 2).

Workgroups of 8 and 16 waves (WIDE): the launcher (dj4_waves) takes the smallest of 4, 8, 16 waves at which four emission
slices of n_jcols + 1 doubles per wave leave a SIMD the pair form's four resident waves within 160 KB of LDS: 4 waves up to
303 junction columns, 8 up to 311, 16 up to 315, the two-sample kernel beyond.  With one pattern per site a family has four
junction columns per junction site, and Spec.small(len_v=70, n_sites=112, v_r_width=w) has w + 16 such sites: w = 59 .. 63
gives 300, 304, 308, 312, 316 columns, one family on each side of every threshold.  lh_family_forward_dj_waves must say 4,
8, 8, 16 (GL = 2 and GL = 1) and the two-sample kernel's 4.  A workgroup of 16 waves holds 64 samples: these families' one
call has at least 129 rows (three such workgroups, the last wave with one sample), calls of 31 .. 33 and 63 .. 65 rows
must come back bit for bit as well, and their case `row3_dj` rescales one D-J row three times at once (their `row3` lands
in the wide V-D junction).

One child process per hook setting (tests/k2b_dj_quad_worker.py, which lists what it checks by itself: every case of
tests/k2_scaling_cases.py against the identity and the numpy oracle at the bounds of tests/test_gpu_k2_forms.py, calls of
1 .. 17 rows bit for bit the rows of the one large call, in both range modes), and the parent compares the two children:
log-likelihoods, forward arrays and ScaleMatrix counts bit-identical.

Which cases rescale INSIDE the D-J junction is checked on the CPU (test_the_cases_rescale_inside_the_dj_junction): `single`,
`double`, `zero` (a row's count rises by one or more on several rows) and `row3` (one D-J row that rescales three times at
once) in every family; `base` in none.  The worker's row order gives each of them a wave whose other three samples are
`base`: on those rows one sample of the wave rescales and three do not, which is the per-lane RowScale of the rare
branch."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import k2_scaling_cases as kc
from tests import k2b_dj_quad_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "k2b_dj_quad_worker.py")
HOOKS = ("LH_K2B_DJ_PAIR", "LH_K2B_NO_PAIR", "LH_K2B_VD_SINGLE", "LH_K2A_DIRECT")

# name -> (D alleles, J alleles, samples per D-J wave without the hook)
FAMILIES = {
    "d1_j1": (1, 1, 4),
    "d16_j16": (16, 16, 4),
    "d17_j16": (17, 16, 4),
    "d32_j16": (32, 16, 4),
    "d30_j12": (30, 12, 4),
    "d30_j17": (30, 17, 2),
}
# name -> (v_r_width, D alleles, J alleles, junction columns, waves per D-J workgroup, samples per D-J wave)
WIDE = {
    "w59_d17_j16": (59, 17, 16, 300, 4, 4),      # the last width with 4 waves
    "w60_d16_j16": (60, 16, 16, 304, 8, 4),      # the first with 8
    "w61_d32_j16": (61, 32, 16, 308, 8, 4),
    "w62_d32_j16": (62, 32, 16, 312, 16, 4),     # 16 waves, GL = 2
    "w62_d16_j16": (62, 16, 16, 312, 16, 4),     # 16 waves, GL = 1
    "w63_d3_j3": (63, 3, 3, 316, 4, 2),          # no workgroup size fits: junction_dj_kernel's four waves of two samples
}
PAIR_WAVES = 4                                   # (junction_dj_kernel's workgroup)
NEED = ("single", "double", "zero", "row3")      # the cases whose D-J rows rescale
SETTINGS = {"default": {}, "dj_pair": {"LH_K2B_DJ_PAIR": "1"}}


def load_family(n_d, n_j, workdir, width=None):
    """k2_scaling_cases.load_family for a spec of this module: every site a pattern of its own"""
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    out = os.path.join(str(workdir), "d%d_j%d_w%s" % (n_d, n_j, width))
    wide = {} if width is None else dict(len_v=70, n_sites=112, v_r_width=width)
    sf.generate(sf.Spec.small(n_d=n_d, n_j=n_j, n_leaves=6, n_samples=1, seed=100 + n_d + n_j, **wide), out)
    h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
    n, L = h.msa.shape
    assert 4 ** n >= L
    h.msa = np.array([[(j // 4 ** i) % 4 for j in range(L)] for i in range(n)], dtype=np.int32)
    h._initialize_xmsa_structs()
    return h


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """Cases and references of every family, built once on the CPU and handed to the children as a file."""
    work = tmp_path_factory.mktemp("k2b_dj_quad")
    built = {}
    for name, (n_d, n_j, _) in FAMILIES.items():
        h = load_family(n_d, n_j, work)
        assert len(h.dgerm.ggene_ranges) == n_d and len(h.jgerm.ggene_ranges) == n_j
        _, cases = kc.build_cases(h, 1)
        refs = kc.references(h, cases)
        kc.check_conditions(h, cases, refs, need=NEED)
        built[name] = (h, cases, refs, 33)
    for name, (width, n_d, n_j, _, _, _) in WIDE.items():
        h = load_family(n_d, n_j, work, width)
        assert len(h.dgerm.ggene_ranges) == n_d and len(h.jgerm.ggene_ranges) == n_j
        _, cases = kc.build_cases(h, 1)
        refs = kc.references(h, cases)
        kc.check_conditions(h, cases, refs, need=NEED + ("row3_dj",))
        built[name] = (h, cases, refs, 129)
    path = str(work / "references.pkl")
    with open(path, "wb") as f:
        pickle.dump(built, f)
    return {"path": path, "work": work, "built": built, "children": {}}


def _child(references, setting):
    """runs the child of one hook setting once per module; -> (report, arrays)"""
    done = references["children"]
    if setting not in done:
        env = {k: v for k, v in os.environ.items() if k not in HOOKS}
        env.update(SETTINGS[setting])
        out = str(references["work"] / (setting + ".npz"))
        r = subprocess.run([sys.executable, WORKER, references["path"], out], capture_output=True, text=True, timeout=600,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, "%s\n%s" % (r.stdout[-2000:], r.stderr[-6000:])
        with np.load(out) as z:
            arrays = {k: z[k] for k in z.files}
        done[setting] = (json.loads(r.stdout.strip().splitlines()[-1]), arrays)
    return done[setting]


def junction_columns(h):
    """distinct xMSA columns the junction tables read: the device's n_jcols where every site has a pattern of its own"""
    return len({int(x) for inds in (h.vd_junction_xmsa_inds, h.dj_junction_xmsa_inds) for x in inds.ravel() if x >= 0})


def test_the_cases_rescale_inside_the_dj_junction(references):
    """on the numpy oracle: `single`, `double`, `zero` and `row3` rescale D-J rows (row3 three times on one row), `base`
    none; and the worker's row order puts each of them into a wave with three `base` rows, in every position.  The wide
    families (whose `row3` lies in the V-D junction) likewise with `row3_dj`, and their junction columns are counted"""
    for name, (h, cases, refs, n_min) in references["built"].items():
        steps = {c.name: kc.dj_increments(refs[c.name]["oracle"]) for c in cases if c.expect == "finite"}
        assert not any(steps["base"]), (name, steps["base"])
        need = NEED if name in FAMILIES else ("single", "double", "zero", "row3_dj")
        for case in need:
            assert any(steps[case]), (name, case, steps[case])
        assert 3 in steps[need[3]], (name, steps[need[3]])
        assert sum(1 for s in steps["double"] if s) >= 3, (name, steps["double"])
        if name in WIDE:
            assert sum(1 for s in steps["double"] if s) >= 5, (name, steps["double"])
            assert junction_columns(h) == WIDE[name][3], (name, junction_columns(h))
        order = worker.wave_order(cases, n_min)
        assert len(order) >= n_min and len(order) % 4 == 1
        waves = [order[i:i + 4] for i in range(0, len(order) - 1, 4)]
        for case in need:
            assert any(w.count("base") == 3 and case in w for w in waves), (name, case)
        assert {w.index(c) for w in waves for c in w if c != "base" and w.count("base") == 3} == {0, 1, 2, 3}
        assert any("base" not in w for w in waves)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_dj_sweep_against_the_oracle(references, setting):
    """the child's own checks (it exits nonzero when one fails), the K2b form and the D-J layout of every family"""
    report, _ = _child(references, setting)
    for name, (_, _, samples) in FAMILIES.items():
        for mode in ("default", "extended"):
            info = report[name][mode]
            assert info["form"].endswith("| vd2<1>+dj"), (name, mode, info["form"])
            assert info["dj_samples"] == (2 if setting == "dj_pair" else samples), (name, mode, info)
            assert info["n"] >= 33
    for name, (_, _, _, n_jcols, waves, samples) in WIDE.items():
        for mode in ("default", "extended"):
            info = report[name][mode]
            print("%s %s %s: %d junction columns, %d samples per wave, %d waves per workgroup, %d rows" %
                  (setting, name, mode, n_jcols, info["dj_samples"], info["dj_waves"], info["n"]))
            assert info["form"].endswith("| vd2<1>+dj"), (name, mode, info["form"])
            assert info["dj_samples"] == (2 if setting == "dj_pair" else samples), (name, mode, info)
            assert info["dj_waves"] == (PAIR_WAVES if setting == "dj_pair" else waves), (name, mode, info)
            assert info["n"] >= 129
    for name in report:
        for mode in ("default", "extended"):
            dev = report[name][mode]["deviation"]
            print("%s %s %s: log-likelihood against the identity %.2e, forward arrays against the oracle %.2e"
                  % (setting, name, mode, dev["loglik"], dev["forward"]))


@pytest.mark.gpu
def test_four_samples_per_wave_keep_every_bit(references):
    """log-likelihoods, forward arrays and ScaleMatrix counts of the two children, per family and range mode"""
    quad, pair = _child(references, "default")[1], _child(references, "dj_pair")[1]
    assert set(quad) == set(pair) and len(quad) == 6 * (len(FAMILIES) + len(WIDE))
    for key in sorted(quad):
        assert quad[key].shape == pair[key].shape and quad[key].dtype == pair[key].dtype, key
        assert np.array_equal(quad[key].view(np.uint8), pair[key].view(np.uint8)), key
