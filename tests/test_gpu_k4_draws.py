"""K4 (lh_sample.hip) on crafted emissions with unlike rows in one wave.

K4 draws four samples per wave, sixteen lanes each, and shares control flow across the wave: the `nz` chunk mask is a ballot
over all four groups, the partial-sum loops end when EVERY group has its answer, a group past the end of the batch walks the
last sample along, a zero chunk advances `below` without touching the sums, and a NaN or zero sum sends one group to kFirst
while its neighbours go on.  lh_sample_forward_batch takes the caller's emissions and engine words: tests/k4_draw_cases.py
builds calls of n = 8 |C| + 1 rows (the cases of tests/k2_scaling_cases.py x eight word patterns) whose wave mates differ in
emissions and in words, with two references (tier 1: the oracle's dense draws on the row's own device forward arrays, exact
on every row; tier 2: the oracle end to end, on the rows where a 1e-9 difference of the forward arrays cannot move an
answer); tests/test_k4_draw_cases_cpu.py checks the rows and what they reach without a GPU.

One child process per hook setting (tests/k4_draws_worker.py): no hook, and LH_K4_NO_SAVE=1 (every family in the recompute
form of group_draw, which only families wider than 256 genes -- igh_v260 here -- take by themselves).  Per family, in the
default and in the extended-range mode:
  1. log-likelihood against the identity 1e-12 where finite (delta4 not finite in the default mode, finite in the extended
     one); log-likelihood, forward arrays and counts bit-equal to lh_forward_batch's on the same emissions, so that the
     coverage of tests/test_gpu_k2_forms.py carries over;
  2. states equal to tier 1 on every row, the NaN rows included, and to tier 2 on its rows;
  3. layout independence, bit for bit: the call reversed, rotated by 1, 2 and 3 rows, the first 16 rows each alone;
  4. extended range: the default mode's states on every row whose default forward arrays are finite (delta4's rows match
     tier 1 on the mode's own arrays, as every row does);
and the parent compares the children: states bit-equal on all rows of all families and both modes."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import k2_scaling_cases as kc
from tests import k4_draw_cases as k4

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "k4_draws_worker.py")
HOOK = "LH_K4_NO_SAVE"
SETTINGS = {"default": {}, "no_save": {HOOK: "1"}}


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """Rows and references of every family, built once on the CPU and handed to the children as a file."""
    work = tmp_path_factory.mktemp("k4_draws")
    built = {}
    for name in k4.FAMILIES:
        h, rows = k4.build_rows(name, work)
        refs = kc.references(h, rows.cases)
        _, tier2 = k4.check_margins(h, rows)
        built[name] = (h, rows, {c.name: refs[c.name]["identity"] for c in rows.cases}, tier2)
    path = str(work / "references.pkl")
    with open(path, "wb") as f:
        pickle.dump(built, f)
    return {"path": path, "work": work, "built": built, "children": {}}


def _child(references, setting):
    """runs the child of one hook setting once per module; -> (report, arrays)"""
    done = references["children"]
    if setting not in done:
        env = {k: v for k, v in os.environ.items() if k != HOOK}
        env.update(SETTINGS[setting])
        out = str(references["work"] / (setting + ".npz"))
        r = subprocess.run([sys.executable, WORKER, references["path"], out] + list(k4.FAMILIES), capture_output=True,
                           text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, "%s\n%s" % (r.stdout[-2000:], r.stderr[-6000:])
        with np.load(out) as z:
            arrays = {k: z[k] for k in z.files}
        done[setting] = (json.loads(r.stdout.strip().splitlines()[-1]), arrays)
    return done[setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_draws_of_unlike_rows_in_one_wave(references, setting):
    """the child's own checks (it exits nonzero when one fails); every row was compared, and reached what it is for"""
    report, _ = _child(references, setting)
    for name in k4.FAMILIES:
        h, rows, _, tier2 = references["built"][name]
        for mode in ("default", "extended"):
            info = report[name][mode]
            print(setting, name, mode, json.dumps(info))
            assert info["n"] == rows.n == 8 * len(rows.cases) + 1 and info["n"] % 4 == 1 and info["n"] <= 137
            assert info["tier1_rows"] == rows.n and info["tier1_bad"] == []
            assert info["tier2_rows"] == len(tier2) >= 3 and info["tier2_bad"] == []
            assert info["loglik"] <= 1e-12
        has_delta4 = any(c.expect == "overflow" for c in rows.cases)
        assert report[name]["default"]["nonfinite_rows"] == (8 if has_delta4 else 0)
        assert report[name]["extended"]["nonfinite_rows"] == 0
        assert report[name]["extended"]["equal_default_rows"] == rows.n - (8 if has_delta4 else 0)
        # what the device's rows reached, counted on tier 1 (the conditions of tests/test_k4_draw_cases_cpu.py, here on the
        # device's own forward arrays)
        cl = report[name]["default"]["classes"]
        assert cl["a"] >= 1 and cl["c"] >= 1 and cl["e_zero"] >= 1, cl
        if h.locus == "igh":  # (light chains: test_k4_draw_cases_cpu.LIGHT)
            assert cl["a_finite"] >= 1, cl
        if k4.widest_draw(h) > k4.kG:
            assert cl["d"] >= 1, cl
        assert (cl["f"] >= 1) == has_delta4, cl
        # launch_sample's rule on the family's widths: igh_v260 alone takes the recompute form by itself
        assert report[name]["default"]["saved"] == (name != "igh_v260")
    assert not k4.saves_weights(references["built"]["igh_v260"][0])
    assert k4.widest_draw(references["built"]["igh_v260"][0]) == 272


def test_recompute_form_equals_saved_form(references):
    """LH_K4_NO_SAVE=1: states bit-equal to the default process's on all rows of all families, in both modes"""
    base, other = _child(references, "default")[1], _child(references, "no_save")[1]
    assert set(base) == set(other) == {"%s|%s|states" % (n, m) for n in k4.FAMILIES for m in ("default", "extended")}
    for key in sorted(base):
        differ = np.nonzero(np.any(base[key] != other[key], axis=1))[0]
        assert base[key].dtype == np.int32 and base[key].tobytes() == other[key].tobytes(), (key, differ[:10].tolist())


def test_refusals(references):
    """a handle without sampler tables is refused with a message, as the tree-driven twins refuse it; n = 0 is a no-op"""
    import linearham_amd
    from tests import desc_builder as db
    from tests import viterbi_oracle as vo
    h, rows, _, _ = references["built"]["toy"]
    hip = linearham_amd.load_library()
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    with pytest.raises(RuntimeError, match="lh_sample_forward_batch: lh_family_set_sampler has not been called"):
        hip.sample_forward_batch(fam, rows.em[:2], np.zeros((2, 0), np.uint32))
    with pytest.raises(RuntimeError, match="lh_posterior_forward_batch: lh_family_set_sampler has not been called"):
        fam.posterior_forward_batch(rows.em[:2])
    fam.set_sampler(*vo.sampler_tables(h))
    ll, st, _ = fam.sample_forward_batch(rows.em[:0], rows.words[:0])
    assert ll.shape == (0,) and st.shape == (0, len(k4.draw_sizes(h)))
    fam.close()
