"""K8 (the most probable state path, lh_viterbi.hip) and candidate paths on the device against tests/viterbi_oracle.py.

Families exist as oracle objects; their device handles are built from them (tests/desc_builder.py) with sampler tables
(viterbi_oracle.sampler_tables), so every family the oracle can express runs here, those of tests/k2_scaling_cases.py
with their rewritten alignments included."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import k2_scaling_cases as kc
from tests import viterbi_cases as vc
from tests import viterbi_oracle as vo

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-10        # log_path against the oracle: BOUND * (1 + |log_path|)
MIN_MARGIN = 1e-6    # the oracle's best path must lead its runner-up by this much at every step (else: another seed)
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def hip():
    from linearham_amd.capi import load_library
    lib = load_library()
    assert lib.device_count() >= 1
    return lib


def _close(a, b, bound=BOUND):
    return abs(a - b) <= bound * (1.0 + abs(b))


def _check_rows(o, refs, res):
    """every row: states equal the oracle's, log_path within the bound, and the oracle's joint of the DEVICE's path equals
    the oracle's maximum within the same bound"""
    for i, ref in enumerate(refs):
        assert ref["margin"] > MIN_MARGIN, (i, ref["margin"])
    for i, ref in enumerate(refs):
        assert np.array_equal(res["states"][i], ref["states"]), (i, res["states"][i], ref["states"])
        assert _close(res["log_path"][i], ref["log_path"]), (i, res["log_path"][i], ref["log_path"])
        assert _close(res["loglik"][i], ref["loglik"], 1e-9), i
        assert res["log_path"][i] <= res["loglik"][i]
        joint = vo.path_log_joint(o, vo.from_states(o, res["states"][i]), ref["ec"], ref["rows"])
        assert _close(joint, ref["log_path"]), (i, joint, ref["log_path"])


# ---- against the oracle ----

@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_golden_families(hip, case):
    o, rows = vc.golden_rows(case)
    refs = [vc.oracle_row(o, r, keep_rows=True) for r in rows]
    w, p, n_paths = vo.brute_force_max(o, refs[0]["ec"])    # (o still holds the row)
    assert p == refs[0]["path"] and _close(w, refs[0]["log_path"], 1e-13) and n_paths > 1000
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    _check_rows(o, refs, vc.run_viterbi(hip, fam, inp))
    fam.close()


@pytest.mark.parametrize("n_rows,kw", [(3, dict(locus="igh")), (3, dict(locus="igk")), (3, dict(locus="igl")),
                                       (3, dict(locus="igh", ragged=4, ambiguous=0.02)),
                                       (2, dict(locus="igh", n_v=300, n_d=70, n_j=5)),
                                       (2, dict(locus="igk", n_v=150, n_j=70)),
                                       (40, dict(locus="igh", n_d=65, n_j=30))])
def test_synthetic_families(hip, tmp_path, n_rows, kw):
    o, rows, _ = vc.synthetic_rows(tmp_path, n_rows, **kw)
    refs = [vc.oracle_row(o, r, keep_rows=True) for r in rows]
    if n_rows == 40:
        assert len({tuple(r["path"]) for r in refs}) >= 4
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    _check_rows(o, refs, vc.run_viterbi(hip, fam, inp))
    fam.close()


# ---- crafted emissions through lh_viterbi_forward_batch ----

N_RANDOM = 23
MIN_PATHS = 7


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    """family -> (oracle object, cases, random vectors, {vector name: oracle Viterbi}) built once (CPU)."""
    work = tmp_path_factory.mktemp("viterbi_crafted")
    cache = {}

    def get(name):
        if name not in cache:
            h = kc.load_family(name, work)
            _, cases = kc.build_cases(h, kc.SEEDS[name])
            # (a family's random vectors go by its place among the sorted names; the wide germline sets, added later,
            # stand behind the others so that no earlier family's vectors moved)
            order = sorted(n for n in kc.family_specs() if n not in kc.WIDE) + sorted(kc.WIDE)
            rng = np.random.default_rng(1000 + order.index(name))
            rand = rng.uniform(0.05, 1.0, size=(N_RANDOM, len(cases[0].em)))
            refs = {}
            for nm, em in [(c.name, c.em) for c in cases if c.sum_k == 0] + [("random%d" % i, e) for i, e in enumerate(rand)]:
                ec = vo.set_emissions(h, em)
                refs[nm] = vo.viterbi(h, ec)
                refs[nm]["states"] = vo.to_states(h, refs[nm]["path"])
            cache[name] = (h, cases, rand, refs)
        return cache[name]
    return get


# (every family but the two of 520 V alleles: the numpy Viterbi of their 26 vectors alone takes eleven seconds apiece)
@pytest.mark.parametrize("name", sorted(n for n in kc.family_specs() if n not in ("igh_v520", "igh_v520_j130")))
def test_crafted_emissions(hip, crafted, name):
    h, cases, rand, refs = crafted(name)
    for nm, ref in refs.items():
        assert ref["margin"] > MIN_MARGIN, (nm, ref["margin"])
    names = [c.name for c in cases] + ["random%d" % i for i in range(N_RANDOM)]
    em = np.concatenate([np.stack([c.em for c in cases]), rand])
    by = {c.name: c for c in cases}
    # what every row must give: the path of its base, and log_path on the identity
    want_states = [refs[by[n].base if n in by else n]["states"] for n in names]
    want_lp = [refs[by[n].base]["log_path"] - LN2 * by[n].sum_k if n in by else refs[n]["log_path"] for n in names]
    assert len({tuple(s) for s in want_states}) >= MIN_PATHS
    fam = vc.device_family(hip, h)
    results = {}
    for ext in (False, True):
        fam.set_extended_range(ext)
        lp, st = fam.viterbi_forward_batch(em)
        results[ext] = (lp, st)
        for i, n in enumerate(names):
            if n == "delta4" and not ext:
                assert not np.isfinite(lp[i]) and np.all(st[i] == -1), (n, lp[i])
                continue
            assert np.array_equal(st[i], want_states[i]), (n, ext)
            tol = 1e-12 if n in by else BOUND      # the identity; the random vectors stand against the oracle alone
            assert abs(lp[i] - want_lp[i]) <= tol * (1.0 + abs(want_lp[i])), (n, ext, lp[i], want_lp[i])
        # every row bit-identical to the same vector alone and as row 1 of two
        base = by["base"].em
        for i in range(len(names)):
            l1, s1 = fam.viterbi_forward_batch(em[i][None])
            l2, s2 = fam.viterbi_forward_batch(np.stack([base, em[i]]))
            mine = lp[i:i + 1].tobytes() + st[i].tobytes()
            assert l1.tobytes() + s1[0].tobytes() == mine, (names[i], ext, "alone")
            assert l2[1:2].tobytes() + s2[1].tobytes() == mine, (names[i], ext, "row 1 of two")
    # the two range modes agree bit for bit wherever the default mode has a result
    ok = np.isfinite(results[False][0])
    assert ok.sum() >= len(names) - 1
    assert results[False][0][ok].tobytes() == results[True][0][ok].tobytes()
    assert np.array_equal(results[False][1][ok], results[True][1][ok])
    fam.close()


# ---- ties ----

def test_ties(hip):
    """The toy family with every emission 0.5 (all products of emissions exact, whatever their order): the device's path
    has the oracle's maximum, is the same alone, inside a batch and in both range modes, and is the path of
    viterbi_oracle.emulate_viterbi, the documented rule written out in numpy.  Every path emits every site once, so equal
    emissions alone leave the transitions to decide; the second half makes the ties: the same family with NTI tables that
    are constant over the bases (viterbi_cases.tied_desc), where the opposite rule -- the last of equals -- gives another
    path of the same value, and the device must give the documented one."""
    import linearham_amd
    from tests import desc_builder as db
    h = kc.load_family("toy", None)
    em = np.full(len(kc.column_sites(h)), 0.5)
    ec = vo.set_emissions(h, em)
    ref = vo.viterbi(h, ec)
    rows = vo.chain_rows(h)
    sampler = vo.sampler_tables(h)
    rng = np.random.default_rng(5)
    other = rng.uniform(0.05, 1.0, size=(4, len(em)))

    def stable(fam):
        """the all-0.5 row alone, as rows 2 and 4 of five, in both range modes: one result"""
        seen = set()
        for ext in (False, True):
            fam.set_extended_range(ext)
            l1, s1 = fam.viterbi_forward_batch(em[None])
            l5, s5 = fam.viterbi_forward_batch(np.stack([other[0], other[1], em, other[2], em]))
            assert l5[2:3].tobytes() == l1.tobytes() == l5[4:5].tobytes()
            assert np.array_equal(s5[2], s1[0]) and np.array_equal(s5[4], s1[0])
            seen.add(l1.tobytes() + s1.tobytes())
        assert len(seen) == 1
        return l1[0], s1[0]

    fam = vc.device_family(hip, h)
    lp, st = stable(fam)
    fam.close()
    by_rule, lp_rule = vo.emulate_viterbi(db.build_family_desc(h), sampler, em)
    assert np.array_equal(st, by_rule) and _close(lp, lp_rule, 1e-13)
    assert _close(vo.path_log_joint(h, vo.from_states(h, st), ec, rows), ref["log_path"]) and _close(lp, ref["log_path"])

    desc = vc.tied_desc(h)
    first, lp_first = vo.emulate_viterbi(desc, sampler, em)
    last, lp_last = vo.emulate_viterbi(desc, sampler, em, prefer_last=True)
    assert lp_first == lp_last and not np.array_equal(first, last)      # there are ties, and the rule matters
    fam = linearham_amd.Family(desc, hip)
    fam.set_sampler(*sampler)
    lp, st = stable(fam)
    fam.close()
    assert np.array_equal(st, first), (st, first, last)
    assert _close(lp, lp_first, 1e-13)


# ---- candidate paths ----

def _not_a_path(o, paths):
    """a state vector with every index in range that differs from a path in one junction row and is not a path"""
    n_states = [len(r[2]) for r in vo.chain_rows(o)]
    for p in paths:
        for t in range(1, len(p) - 1):
            for k in range(n_states[t]):
                q = p[:t] + [k] + p[t + 1:]
                if k != p[t] and not vo.is_path(o, q):
                    return q
    raise AssertionError("every single-state change of every path is a path")


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_candidate_paths(hip, case):
    o, rows = vc.golden_rows(case)
    ref = vc.oracle_row(o, rows[0])
    paths = vo.enumerate_paths(o, ref["ec"])
    states = np.stack([vo.to_states(o, p) for _, p in paths])
    want_prior = np.array([vo.log_path_prior(o, p) for _, p in paths])
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    vit = vc.run_viterbi(hip, fam, inp)
    prior = hip.set_candidate_paths(fam, states)
    assert np.max(np.abs(prior - want_prior) / (1.0 + np.abs(want_prior))) < 1e-12
    K = len(paths)
    assert hip.candidates_info(fam)[0] == K

    def score():
        return hip.eval_candidates_batch(fam, inp["n_tips"], inp["max_depth"], inp["ops"], inp["brlen"], inp["er"],
                                         inp["pi"], inp["alpha"], inp["R"], want=("loglik", "log_cand"))
    res = score()
    lc = res["log_cand"][0]
    # every path of the model is registered: their posteriors sum to 1
    assert abs(np.exp(lc).sum() - 1.0) < 1e-10
    # the oracle's joint of every path
    want = np.array([w for w, _ in paths]) - ref["loglik"]
    assert np.max(np.abs(lc - want)) < 1e-9
    # the arg-max candidate is K8's path and its posterior is log_path - loglik
    k = int(np.argmax(lc))
    assert np.array_equal(states[k], vit["states"][0])
    assert abs(lc[k] - (vit["log_path"][0] - vit["loglik"][0])) <= 1e-12 * (1.0 + abs(vit["loglik"][0]))
    # grouped by naive sequence they are K6's candidates
    seqs, _ = hip.naive_sequences(fam, states)
    uniq, inv = np.unique(seqs, axis=0, return_inverse=True)
    inv = np.asarray(inv).ravel()
    grouped = np.array([np.log(np.exp(lc[inv == g]).sum()) for g in range(len(uniq))])
    hip.set_candidates(fam, uniq)
    by_seq = score()["log_cand"][0]
    assert np.max(np.abs(grouped - by_seq)) < 1e-10
    # a vector that is not a path is refused, and leaves the handle without candidates
    bad = states[:3].copy()
    bad[1, 0] = 1 << 20                                       # an index out of range
    with pytest.raises(RuntimeError, match="not a path"):
        hip.set_candidate_paths(fam, bad)
    assert hip.candidates_info(fam)[0] == 0
    bad = states[:3].copy()
    bad[2] = vo.to_states(o, _not_a_path(o, [p for _, p in paths]))   # indices in range, a transition of probability 0
    with pytest.raises(RuntimeError, match="vector 2 is not a path"):
        hip.set_candidate_paths(fam, bad)
    assert np.array_equal(hip.set_candidate_paths(fam, states[:5]), prior[:5])
    fam.close()


# ---- batches ----

@pytest.fixture(scope="module")
def batch_family(hip, tmp_path_factory):
    o, rows, _ = vc.synthetic_rows(tmp_path_factory.mktemp("viterbi_batch"), 257, locus="igh", seed=77)
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    yield o, rows, fam, inp
    fam.close()


def test_batches(hip, batch_family):
    o, rows, fam, inp = batch_family
    rb = np.array([r["likelihood"] for r in rows])
    full = vc.run_viterbi(hip, fam, inp, log_offset=rb, want=("loglik", "states", "log_path", "weight_stats"))
    assert np.all(np.isfinite(full["log_path"])) and np.all(full["states"] >= 0)
    assert len({tuple(s) for s in full["states"]}) > 1
    for i in (0, 1, 2, 255, 256):
        _check_rows(o, [vc.oracle_row(o, rows[i], keep_rows=True)],
                    {k: full[k][i:i + 1] for k in ("loglik", "states", "log_path")})
    lw = full["loglik"] - rb
    w = np.exp(lw - lw.max())
    st = full["weight_stats"]
    assert st[0] == lw.max() and abs(st[1] - w.sum()) < 1e-13 * w.sum() and abs(st[2] - (w * w).sum()) < 1e-13 * (w * w).sum()
    for n in (1, 3, 5):
        for first in (0, 257 - n):
            sl = slice(first, first + n)
            part = vc.run_viterbi(hip, fam, inp, sl)
            for k in ("loglik", "states", "log_path"):
                assert part[k].tobytes() == full[k][sl].tobytes(), (n, first, k)
    # only what is asked for comes back
    assert set(vc.run_viterbi(hip, fam, inp, slice(0, 3), want=("log_path",))) == {"log_path"}
    # extended range equals default wherever default is finite
    fam.set_extended_range(True)
    ext = vc.run_viterbi(hip, fam, inp)
    fam.set_extended_range(False)
    assert np.array_equal(ext["states"], full["states"])
    assert np.max(np.abs(ext["log_path"] - full["log_path"]) / (1.0 + np.abs(full["log_path"]))) < 1e-12


def test_launch_groups(hip, batch_family, tmp_path):
    """The same 257 rows in launch groups of 256 and 1 (LH_CHUNK = 256, the hook's smallest, read once per process:
    tests/viterbi_device_worker.py --groups): K8 runs behind every group's forward sweep on that group's hand-off
    buffers; every output comes back bit for bit."""
    import hashlib
    o, rows, fam, inp = batch_family
    rb = np.array([r["likelihood"] for r in rows])
    full = vc.run_viterbi(hip, fam, inp, log_offset=rb, want=("loglik", "states", "log_path", "weight_stats"))
    want = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in full.items()}
    worker = os.path.join(HERE, "viterbi_device_worker.py")
    r = subprocess.run([sys.executable, worker, "--groups", str(tmp_path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LH_CHUNK="256"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("loglik", "states", "log_path"):
        assert got[k] == want[k], k
    # (weight_stats' sums are taken over the whole batch after the last group: the same kernel on the same array)
    assert got["weight_stats"] == want["weight_stats"]


def test_malformed_host_schedule(hip, batch_family):
    o, rows, fam, inp = batch_family
    ops = inp["ops"][:4].copy()
    ops[2, 0, 1] = 1 << 20
    with pytest.raises(RuntimeError, match="malformed schedule"):
        hip.eval_viterbi_batch(fam, inp["n_tips"], inp["max_depth"], ops, inp["brlen"][:4], inp["er"][:4], inp["pi"][:4],
                               inp["alpha"][:4], inp["R"])
    fam.status()                                              # reported once
    assert np.all(np.isfinite(vc.run_viterbi(hip, fam, inp, slice(0, 4))["log_path"]))


def test_device_entry_point_and_rejected_schedule():
    """lh_eval_viterbi_batch_device on a stream of torch's (tests/viterbi_device_worker.py, its own process): equal to the
    host-pointer call bit for bit; with one sample's DEVICE-RESIDENT schedule corrupted K0c rejects it: states -1, log_path
    NaN, the handle's error word raised once, the other rows untouched."""
    worker = os.path.join(HERE, "viterbi_device_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["clean_status"] == 0 and res["clean_equal_host"], res
    assert res["status"] != 0 and "malformed schedule" in res["message"], res
    assert res["second_status"] == 0
    assert res["victim_states_minus_one"] and res["victim_log_path_nan"] and res["victim_loglik_nan"]
    assert res["others_equal_clean"]
    assert res["max_lw_equal"] and res["sum_w_rel"] < 1e-14 and res["sum_w2_rel"] < 1e-14


# ---- pipeline and CLI ----

N_PIPE = 150
FILES = (".annotations.tsv", ".best.tsv", ".rows.tsv", ".summary.tsv")


def _exe():
    from linearham_amd import host
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _rewrite_likelihood(tsv, out, values):
    """The RevBayes table `tsv` with its Likelihood column replaced by `values` (%.17g)."""
    lines = open(tsv).read().rstrip("\n").split("\n")
    head = lines[0].split("\t")
    c = head.index("Likelihood")
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == len(values)
    for r, v in zip(rows, values):
        r[c] = "%.17g" % v
    open(out, "w").write("\n".join(["\t".join(head)] + ["\t".join(r) for r in rows]) + "\n")
    return out


class Pipeline:
    """The 150-row synthetic table shared by the pipeline tests: the oracle's most probable path, log-likelihood and chain
    of every row (computed once), prescribed log-weights g on a grid that makes Likelihood_i = ll_i - g_i print exactly
    (tests/test_gpu_weighted_lineage.py's _grid_table), and the library run on that table."""

    def __init__(self, tmp):
        from linearham_amd import host
        self.tmp = tmp
        self.o, self.rows, (self.yaml, self.pdir, self.tsv) = vc.synthetic_rows(tmp, N_PIPE, locus="igh", seed=11)
        self.refs = [vc.oracle_row(self.o, r, keep_rows=True) for r in self.rows]
        self.h = host.PhyloHMM(self.yaml, 0, self.pdir, 0)
        fl = self.h.flatten_tsv(self.tsv, N_PIPE)
        from linearham_amd.capi import load_library
        self.ll = load_library().eval_viterbi_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"],
                                                    fl["er"], fl["pi"], fl["alpha"], 4, want=("loglik",))["loglik"]
        rng = np.random.default_rng(3)
        self.g = np.round(rng.uniform(-3.0, 3.0, N_PIPE) * 1024.0) / 1024.0
        u = min(math.ulp(x) for x in self.ll)
        assert u <= 2.0 ** -10 and max(abs(self.g)) + 3.0 < 2.0 ** 53 * u
        self.table = self.grid("grid.tsv")
        self.got = self.h.run_annotations_pipeline(self.table, str(tmp / "lib"), 4)

    def grid(self, name, shift=0.0):
        vals = [round((ll - g) * 1024.0) / 1024.0 + shift for ll, g in zip(self.ll, self.g)]
        return _rewrite_likelihood(self.tsv, str(self.tmp / name), vals)

    def cli(self, prefix, table=None, env=None, extra=()):
        args = [_exe(), "--annotations-pipeline", "--yaml-path", self.yaml, "--cluster-ind", "0", "--hmm-param-dir", self.pdir,
                "--input-path", table or self.table, "--output-path", str(self.tmp / prefix), "--num-rates", "4"] + list(extra)
        return subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))

    def same(self, a, b, files=FILES):
        for f in files:
            assert open(str(self.tmp / a) + f, "rb").read() == open(str(self.tmp / b) + f, "rb").read(), (a, b, f)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    return Pipeline(tmp_path_factory.mktemp("viterbi_pipeline"))


def test_pipeline_against_the_oracle(pipe):
    got, refs, o = pipe.got, pipe.refs, pipe.o
    assert all(r["margin"] > MIN_MARGIN for r in refs)
    # the weights the table prescribes: lw_i = ll_i - Likelihood_i = g_i up to the grid's rounding of Likelihood_i
    lw = np.array([x["log_weight"] for x in got["rows"]])
    assert np.max(np.abs(lw - pipe.g)) < 2.0 ** -10
    w = np.exp(lw - lw.max())
    # the distinct MAP paths of the oracle, by first appearance, and the annotation each formats to
    paths, path_of_row = [], []
    for r in refs:
        if r["path"] not in paths:
            paths.append(r["path"])
        path_of_row.append(paths.index(r["path"]))
    cols = pipe.h.annotation_columns(np.stack([vo.to_states(o, p) for p in paths]))
    # the oracle's P(path k | data, tree i) on every row, weighted
    post = np.array([[math.exp(vo.path_log_joint(o, p, r["ec"], r["rows"]) - r["loglik"]) for p in paths] for r in refs])
    prob = (w[:, None] * post).sum(axis=0) / w.sum()
    want = {}
    for k, c in enumerate(cols):
        want[c] = want.get(c, 0.0) + prob[k]
    ann = got["annotations"]
    head = open(str(pipe.tmp / "lib") + ".annotations.tsv").readline().rstrip("\n").split("\t")
    assert head[:6] == ["rank", "probability", "log_probability", "log_prior", "map_rows", "map_weight_share"]
    key = lambda a: "\t".join(a[h] for h in head[6:])
    assert sorted(key(a) for a in ann) == sorted(want)
    for a in ann:
        assert abs(a["probability"] - want[key(a)]) < 1e-10, (a["rank"], a["probability"], want[key(a)])
        assert abs(a["log_probability"] - math.log(a["probability"])) < 1e-12
    assert [a["rank"] for a in ann] == list(range(1, len(ann) + 1))
    assert all(x["probability"] >= y["probability"] for x, y in zip(ann, ann[1:]))
    assert got["best"] == ann[0]
    # priors, MAP rows and MAP weight shares
    prior, n_map, share = {}, {}, {}
    for k, c in enumerate(cols):
        prior[c] = prior.get(c, 0.0) + math.exp(vo.log_path_prior(o, paths[k]))
    for i, k in enumerate(path_of_row):
        n_map[cols[k]] = n_map.get(cols[k], 0) + 1
        share[cols[k]] = share.get(cols[k], 0.0) + w[i] / w.sum()
    for a in ann:
        assert abs(a["log_prior"] - math.log(prior[key(a)])) < 1e-11 * (1.0 + abs(a["log_prior"]))
        assert a["map_rows"] == n_map[key(a)] and abs(a["map_weight_share"] - share[key(a)]) < 1e-12
    # rows
    rank = {key(a): a["rank"] for a in ann}
    assert [x["row"] for x in got["rows"]] == list(range(N_PIPE))
    for i, (x, r) in enumerate(zip(got["rows"], refs)):
        assert _close(x["lh_loglik"], r["loglik"], 1e-9), i
        assert _close(x["log_path_posterior"], r["log_path"] - r["loglik"]), i
        assert x["annotation"] == rank[cols[path_of_row[i]]], i
    s = got["summary"]
    assert (s["rows_used"], s["rows_skipped_nonfinite"], s["distinct_paths"], s["paths_scored"]) == (N_PIPE, 0, len(paths), len(paths))
    assert s["annotations"] == len(want)
    assert abs(s["covered_mass"] - sum(want.values())) < 1e-10 and s["covered_mass"] <= 1.0 + 1e-12
    ess = w.sum() ** 2 / (w * w).sum()
    assert abs(s["kish_ess"] - ess) < 1e-9 * ess


def test_pipeline_invariances(pipe):
    """The CLI writes the library call's bytes, whatever LH_PIPELINE_BATCH cuts the table into; a constant added to every
    Likelihood moves the rows' log-weights by exactly that and changes nothing else; the burn-in drops the first rows;
    max-candidates keeps the paths of largest MAP weight."""
    from linearham_amd import host
    r = pipe.cli("cli")
    assert r.returncode == 0, r.stderr
    pipe.same("cli", "lib")
    for b in ("1", "7", "64"):
        r = pipe.cli("b" + b, env={"LH_PIPELINE_BATCH": b})
        assert r.returncode == 0, r.stderr
        pipe.same("b" + b, "lib")
    shifted = pipe.h.run_annotations_pipeline(pipe.grid("shift.tsv", shift=2.0), str(pipe.tmp / "shift"), 4)
    pipe.same("shift", "lib", (".annotations.tsv", ".best.tsv", ".summary.tsv"))
    for x, y in zip(pipe.got["rows"], shifted["rows"]):
        assert x["log_weight"] - y["log_weight"] == 2.0
        assert {k: v for k, v in x.items() if k != "log_weight"} == {k: v for k, v in y.items() if k != "log_weight"}
    burn = pipe.h.run_annotations_pipeline(pipe.table, str(pipe.tmp / "burn"), 4, burnin_frac=0.2)
    assert [x["row"] for x in burn["rows"]] == list(range(30, N_PIPE)) and burn["summary"]["rows_used"] == N_PIPE - 30
    assert [x["lh_loglik"] for x in burn["rows"]] == [x["lh_loglik"] for x in pipe.got["rows"][30:]]
    two = pipe.h.run_annotations_pipeline(pipe.table, str(pipe.tmp / "two"), 4, max_candidates=2)
    assert two["summary"]["paths_scored"] == 2 and two["summary"]["distinct_paths"] == pipe.got["summary"]["distinct_paths"]
    assert two["summary"]["covered_mass"] < pipe.got["summary"]["covered_mass"] and len(two["annotations"]) <= 2
    assert any(x["annotation"] is None for x in two["rows"])
    r = pipe.cli("e", extra=["--devices", "0,1"])
    assert r.returncode != 0 and "one device" in r.stderr
    with pytest.raises(RuntimeError, match="max-candidates"):
        pipe.h.run_annotations_pipeline(pipe.table, str(pipe.tmp / "e"), 4, max_candidates=0)
    assert host.read_annotations(str(pipe.tmp / "cli")) == pipe.got


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_cli_viterbi_golden(hip, case):
    """`linearham --viterbi` on a golden family prints PhyloHMM::ViterbiAnnotation's line: the oracle's path and values."""
    from linearham_amd import host
    o, rows = vc.golden_rows(case)
    ref = vc.oracle_row(o, rows[0])
    r0 = rows[0]
    h = host.PhyloHMM(os.path.join(vc.D, case + ".yaml"), 0, os.path.join(vc.D, "hmm_params"), 0)
    h.initialize_phylo_parameters(r0["tree"], r0["er"], r0["pi"], r0["alpha"], r0["R"])
    ann, lp, ll = h.viterbi_annotation()
    assert _close(lp, ref["log_path"]) and _close(ll, ref["loglik"], 1e-9)
    want_cols = h.annotation_columns(ref["states"][None])[0]
    assert "\t".join(ann[k] for k in ann) == want_cols
    args = [_exe(), "--viterbi", "--yaml-path", os.path.join(vc.D, case + ".yaml"), "--cluster-ind", "0", "--hmm-param-dir",
            os.path.join(vc.D, "hmm_params"), "--newick-path", r0["tree"], "--num-rates", str(r0["R"]), "--alpha", repr(r0["alpha"])]
    args += sum([["--er", repr(x)] for x in r0["er"]], []) + sum([["--pi", repr(x)] for x in r0["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    head, line = r.stdout.rstrip("\n").split("\n")
    assert head.split("\t")[:4] == ["log_path", "log_path_posterior", "lh_loglik", "NaiveSequence"]
    f = line.split("\t")
    assert float(f[0]) == lp and float(f[2]) == ll and float(f[1]) == lp - ll
    assert "\t".join(f[3:]) == want_cols.rstrip("\t") or "\t".join(f[3:]) == want_cols


def test_simple_hmm_viterbi_path():
    """SimpleHMM::ViterbiPath (lh_viterbi_forward_batch on the star-tree emissions) against the oracle's SimpleHMM."""
    from linearham_amd import host
    from oracle import linearham_oracle as orc
    from tests import posterior_oracle as po
    for case in ("simple_hmm_input", "simple_hmm_input_extra"):
        o = orc.SimpleHMM(os.path.join(vc.D, case + ".yaml"), 0, os.path.join(vc.D, "hmm_params"), 0)
        ec = po.emission_count(o)
        ref = vo.viterbi(o, ec)
        assert ref["margin"] > MIN_MARGIN
        h = host.SimpleHMM(os.path.join(vc.D, case + ".yaml"), 0, os.path.join(vc.D, "hmm_params"), 0)
        seq, lp = h.viterbi_path()
        assert _close(lp, ref["log_path"]), (case, lp, ref["log_path"])
        assert len(seq) == o.msa.shape[1] and set(seq) <= set("ACGTN")
