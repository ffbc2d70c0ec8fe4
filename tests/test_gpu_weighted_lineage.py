"""Importance-weighted lineage tables in one pass.  The chain lh_eval_lineage_batch (K0-K2, K4, K6c, K3 with D ancestral draws
per row, K7 behind ONE unmixed K1 launch) against the same work composed from the existing entry points, bit for bit;
its bases against oracle/asr_oracle.py; PhyloHMM::RunWeightedLineagePipeline / `linearham --weighted-lineage-pipeline`
against tests/weighted_lineage_oracle.py on tables built from the existing calls; its invariances and refusals."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from linearham_amd import capi, host
from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import weighted_lineage_oracle as wlo
from tests.test_gpu_lineage import BASES, _chain, _family
from tests.test_lineage_cpu import FILES, something_to_count
from tests.test_weighted_lineage_cpu import compare_weighted

pytestmark = pytest.mark.gpu

FAMILIES = [dict(n_leaves=8), dict(n_leaves=12, locus="igk", seed=43), dict(n_leaves=20, seed=42, ragged=6, ambiguous=0.02)]


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def mt_words(seed, n_rows, per_row, skip_rows=0):
    """The std::mt19937(seed) outputs rows skip_rows .. skip_rows + n_rows - 1 of `--pipeline --seed seed` consume."""
    rng = orc.MT19937(seed)
    for _ in range(skip_rows * per_row):
        rng()
    return np.array([rng() for _ in range(n_rows * per_row)], dtype=np.uint32).reshape(n_rows, per_row)


class Case:
    """A synthetic family, its tree samples as device inputs, the lineage paths of its last tip and a borrowed handle
    of the host's family (which has the sampler tables)."""

    def __init__(self, hip, tmp_path, n, **kw):
        self.yaml, self.pdir, self.tsv, self.rows = _family(tmp_path, n_samples=n, **kw)
        self.h = host.PhyloHMM(self.yaml, 0, self.pdir, 3)
        self.o = orc.PhyloHMM(self.yaml, 0, self.pdir, 3)
        self.fam = capi.Family.borrow(self.h.flatten_tsv(self.tsv, 1)["family"], hip)
        self.hip = hip
        self.T, self.L = self.o.msa.shape[0] + 1, self.o.msa.shape[1]
        T = self.T
        ops, brl, self.chains, self.trees, self.depth = [], [], [], [], 0
        for s in self.rows:
            # the host's own arrays: a draw's Philox index holds the inner node's number, and the pipeline numbers the
            # nodes as the host's parser does (the oracle's parser numbers them differently)
            children, root, brlen = host.newick_arrays(s["tree"], list(self.o.xmsa_labels))
            o, d = hip.schedule_tree(T, children, root)
            ops.append(o)
            brl.append(brlen)
            self.depth = max(self.depth, d)
            self.trees.append((children, root, brlen))
            self.chains.append(_chain(np.asarray(children).ravel(), root, T, T - 1))
        self.P = max(len(c) for c in self.chains)
        self.path = np.full((n, self.P), -1, dtype=np.int32)
        for i, c in enumerate(self.chains):
            self.path[i, :len(c)] = c
        self.ops, self.brl = np.stack(ops), np.stack(brl)
        self.er = np.array([s["er"] for s in self.rows])
        self.pi = np.array([s["pi"] for s in self.rows])
        self.alpha = np.array([s["alpha"] for s in self.rows])
        self.NW = hip.lib.lh_sample_words(self.fam.handle)
        self.NS = hip.lib.lh_sample_states(self.fam.handle)

    def chain(self, R, words, seed, draws, first_sample=0, sel=slice(None)):
        return self.fam.eval_lineage_batch(self.T, self.depth, self.ops[sel], self.brl[sel], self.er[sel], self.pi[sel],
                                           self.alpha[sel], R, words, seed, self.path[sel], draws, first_sample)

    def sample_states(self, R, words):
        """lh_eval_sample_batch: (loglik, states)."""
        n = len(self.rows)
        ll, st = np.zeros(n), np.zeros((n, self.NS), dtype=np.int32)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        lib = self.hip.lib
        lib.lh_eval_sample_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)] + \
            [C.POINTER(C.c_double)] * 4 + [C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_int32)]
        w = np.ascontiguousarray(words, dtype=np.uint32)
        self.hip.check(lib.lh_eval_sample_batch(self.fam.handle, n, self.T, self.depth, p(self.ops, C.c_int32),
                                                p(self.brl, C.c_double), p(self.er, C.c_double), p(self.pi, C.c_double),
                                                p(self.alpha, C.c_double), R, p(w, C.c_uint32), p(ll, C.c_double), None,
                                                p(st, C.c_int32)))
        return ll, st


def _call_refused(hip, fam, n, T, P, draws, first_sample=0, R=4):
    """lh_eval_lineage_batch on shapes alone (the arrays are never read: the call is refused first): the message."""
    z = C.c_void_p(8)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    outs = capi._LineageEvalOutputs()
    rc = hip.lib.lh_eval_lineage_batch(fam.handle, n, T, 4, C.cast(z, i32), C.cast(z, f64), C.cast(z, f64), C.cast(z, f64),
                                       C.cast(z, f64), R, C.cast(z, C.POINTER(C.c_uint32)), 1, first_sample, draws,
                                       C.cast(z, i32), P, C.byref(outs))
    assert rc != 0
    return hip.error()


# ---- 1. the chain = the composition of the existing entry points, bit for bit ----

@pytest.mark.parametrize("kw,D,R", [(FAMILIES[0], 1, 4), (FAMILIES[0], 3, 4), (FAMILIES[1], 3, 4), (FAMILIES[2], 3, 4),
                                    (FAMILIES[2], 1, 4), (FAMILIES[1], 3, 3)],
                         ids=["igh-D1", "igh-D3", "igk-D3", "ragged_n-D3", "ragged_n-D1", "igk-D3-R3"])
def test_chain_equals_the_composition(hip, tmp_path, kw, D, R):
    n, seed, first = 37, 20261017, 5
    c = Case(hip, tmp_path, n, **kw)
    words = np.random.default_rng(D * 10 + R).integers(0, 2 ** 32, size=(n, c.NW), dtype=np.uint64).astype(np.uint32)
    got = c.chain(R, words, seed, D, first)
    ll, res = c.fam.eval_batch(c.T, c.depth, c.ops, c.brl, c.er, c.pi, c.alpha, R, want=("rates",))
    for i in range(n):
        print("row %d loglik chain %.17g eval %.17g" % (i, got["loglik"][i], ll[i]))
        assert abs(got["loglik"][i] - ll[i]) <= 1e-12 * abs(ll[i]), i
    assert np.array_equal(got["rates"], res["rates"])
    _, states = c.sample_states(R, words)
    assert np.array_equal(got["states"], states)   # exact across fused and unfused K1
    seqs, hsh = hip.naive_sequences(c.fam, got["states"])
    assert np.array_equal(got["naive"], seqs) and np.array_equal(got["naive_hash"], hsh)
    assert got["naive"].max() <= 4
    assert got["nt_hash"].shape == (n, D, c.P + 1)
    # draw 2 (or the only one) read back from the chain's batch before another call replaces it
    d_read = D - 1
    slots = [(i * D + d_read) * (c.P + 1) + s for i in range(n) for s in range(len(c.chains[i]))]
    rows_read = c.fam.lineage_rows_read(slots)
    naive_read = c.fam.lineage_rows_read([(i * D + d_read) * (c.P + 1) + c.P for i in range(n)])
    assert np.array_equal(naive_read, got["naive"])
    for d in range(D):
        nt, aa = c.fam.lineage_batch(c.T, c.depth, c.ops, c.brl, c.er, c.pi, got["rates"], got["naive"], seed, c.path,
                                     first + (d << 32))
        assert np.array_equal(got["nt_hash"][:, d], nt), d
        assert np.array_equal(got["aa_hash"][:, d], aa), d
        assert np.array_equal(nt[:, c.P], got["naive_hash"])   # slot P: the row's naive sequence, whatever d
    anc, _ = c.fam.asr_batch(c.T, c.depth, c.ops, c.brl, c.er, c.pi, got["rates"], got["naive"], seed,
                             first + (d_read << 32))
    want = [anc[i][v - c.T] for i in range(n) for v in c.chains[i]]
    assert np.array_equal(rows_read, np.stack(want))
    c.fam.close()


def test_chain_sub_batch_and_the_store(hip, tmp_path):
    """Draws are a function of (seed, sample number, draw), not of the batch: rows 10.. as a batch of their own with
    first_sample moved give the same hashes; the store resolves the n * D * (P + 1) slots of the batch."""
    n, D, R, seed = 37, 3, 4, 7
    c = Case(hip, tmp_path, n, **FAMILIES[0])
    words = mt_words(3, n, c.NW)
    whole = c.chain(R, words, seed, D, 0)
    part = c.chain(R, words[10:], seed, D, 10, slice(10, None))
    P1 = c.P + 1
    for k in ("loglik", "rates", "states", "naive", "naive_hash", "nt_hash", "aa_hash"):
        assert np.array_equal(part[k], whole[k][10:]), k
    # ids by sequence over every valid slot of the sub-batch: nothing differs, and the store holds them in order
    m = n - 10
    ids = np.full((m, D, P1), -1, dtype=np.int32)
    order = {}
    for i in range(m):
        for d in range(D):
            for s in list(range(len(c.chains[10 + i]))) + [c.P]:
                ids[i, d, s] = order.setdefault(int(part["nt_hash"][i, d, s]), len(order))
    assert len(c.fam.lineage_resolve(ids)) == 0
    with pytest.raises(RuntimeError, match="n_slots"):
        c.fam.lineage_resolve(ids[:, 0])
    assert c.fam.lineage_store_read().shape == (len(order), c.L)
    c.fam.lineage_reset()
    c.fam.close()


# ---- 2. the oracle ----

def test_chain_bases_against_the_asr_oracle(hip, tmp_path):
    """Every lineage slot's bases against oracle/asr_oracle.py on the ORACLE's naive draw (the same std::mt19937 stream)
    and the oracle's rates, sample number row + (d << 32)."""
    n, D, R, seed, mt_seed = 24, 2, 4, 99, 3
    c = Case(hip, tmp_path, n, **FAMILIES[0])
    got = c.chain(R, mt_words(mt_seed, n, c.NW), seed, D, 0)
    o = c.o
    slots, want = [], []
    for i, r in enumerate(c.rows):
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        naive = o.sample_naive_sequence()
        assert "".join(BASES[b] for b in got["naive"][i]) == naive, i
        nv = np.array([BASES.index(ch) for ch in naive], dtype=np.uint8)
        children, root, brlen = c.trees[i]
        for d in range(D):
            _, a_ref, _ = ao.asr_sample(children, root, brlen, c.T, o.msa, nv, r["er"], np.asarray(r["pi"]),
                                        orc.gamma_rates_mean(r["alpha"], R), seed, i + (d << 32))
            for s, v in enumerate(c.chains[i]):
                slots.append((i * D + d) * (c.P + 1) + s)
                want.append(a_ref[v - c.T])
    assert np.array_equal(c.fam.lineage_rows_read(slots), np.stack(want).astype(np.uint8))
    c.fam.close()


# ---- 5. refusals of the entry point (shapes alone; nothing is allocated) ----

def test_entry_point_refusals(hip, tmp_path):
    c = Case(hip, tmp_path, 2, **FAMILIES[0])
    T, L = c.T, c.L
    assert "draws must be in 1 .. 64" in _call_refused(hip, c.fam, 2, T, 1, 0)
    assert "draws must be in 1 .. 64" in _call_refused(hip, c.fam, 2, T, 1, 65)
    assert "2^32" in _call_refused(hip, c.fam, 2, T, 1, 2, first_sample=2 ** 32 - 1)
    assert "path length" in _call_refused(hip, c.fam, 2, T, T - 1, 1)
    for D in (1, 8):
        most = min((1 << 30) // ((T - 2) * L), (2 ** 31 - 1) // 2) // D
        assert ("at most %d samples" % most) in _call_refused(hip, c.fam, most + 1, T, 1, D)
    c.fam.close()


# ---- 6. the device entry point and a schedule K0c rejects (its own process: torch first) ----

def test_device_entry_point_and_a_rejected_schedule():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "weighted_lineage_device_worker.py")],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["clean_status"] == "" and res["stream_equals_host"], res
    assert "malformed schedule" in res["bad_status"]
    assert res["victim_loglik_nan"] and res["victim_all_ones_in_every_draw"] and res["others_unchanged"], res


# ---- the pipeline ----

ALL_FILES = FILES + (".rows.tsv",)
MT_SEED, PHILOX_SEED, N_ROWS = 3, 77, 120


def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _rewrite_likelihood(tsv, out, values):
    """The RevBayes table `tsv` with its Likelihood column replaced by `values` (%.17g, or the text given)."""
    lines = open(tsv).read().rstrip("\n").split("\n")
    head = lines[0].split("\t")
    c = head.index("Likelihood")
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == len(values)
    for r, v in zip(rows, values):
        r[c] = v if isinstance(v, str) else "%.17g" % v
    open(out, "w").write("\n".join(["\t".join(head)] + ["\t".join(r) for r in rows]) + "\n")
    return out


class Tables:
    """What the pipeline tests share, computed once: the igh family of 8 leaves with 120 tree samples, the rows'
    log-likelihoods and rates (lh_eval_batch), their naive sequences (run_pipeline's NaiveSequence column, seed 3), the
    prescribed log-weights g, and per draw the lineage sequences of every row from lh_lineage_batch + lineage_rows_read."""

    def __init__(self, hip, tmp):
        self.tmp = tmp
        c = self.c = Case(hip, tmp, N_ROWS, **FAMILIES[0])
        self.seed_name = list(c.o.xmsa_labels)[-1]
        self.ll, res = c.fam.eval_batch(c.T, c.depth, c.ops, c.brl, c.er, c.pi, c.alpha, 4, want=("rates",))
        self.rates = res["rates"]
        assert np.isfinite(self.ll).all()
        self.g = 1.5 * np.random.default_rng(20261017).standard_normal(N_ROWS)
        self.table = _rewrite_likelihood(c.tsv, str(tmp / "weighted.tsv"), (self.ll - self.g).tolist())
        out = str(tmp / "pipeline.tsv")
        host.PhyloHMM(c.yaml, 0, c.pdir, MT_SEED).run_pipeline(c.tsv, out, 4)
        lines = [ln.rstrip("\n").split("\t") for ln in open(out)]
        k = lines[0].index("NaiveSequence")
        self.naive_text = [ln[k] for ln in lines[1:]]
        self.naive = np.array([[BASES.index(ch) for ch in s] for s in self.naive_text], dtype=np.uint8)
        self.seed_nt = "".join(BASES[b] for b in c.o.msa[c.T - 2])
        self._draws = {}

    def lineages(self, d):
        """Per row the lineage naive, root .. seed's parent, seed of draw d (sample number row + (d << 32))."""
        if d not in self._draws:
            c = self.c
            c.fam.lineage_batch(c.T, c.depth, c.ops, c.brl, c.er, c.pi, self.rates, self.naive, PHILOX_SEED, c.path, d << 32)
            slots = [i * (c.P + 1) + s for i in range(N_ROWS) for s in range(len(c.chains[i]))]
            seqs = iter(c.fam.lineage_rows_read(slots))
            out = []
            for i in range(N_ROWS):
                inner = ["".join(BASES[b] for b in next(seqs)) for _ in c.chains[i]]
                out.append([self.naive_text[i]] + inner[::-1] + [self.seed_nt])
            self._draws[d] = out
        return self._draws[d]

    def expected(self, D, log_weights):
        """The weighted oracle's tables for D draws per row: every (row, draw) one tree of its row's weight, in (row,
        draw) order; rows whose log-weight is not finite left out.  Also the Kish ESS of the used rows."""
        w, ess = wlo.weights_of(list(log_weights))
        trees, weights = [], []
        for i in range(N_ROWS):
            if w[i] is None:
                continue
            for d in range(D):
                trees.append(self.lineages(d)[i])
                weights.append(w[i])
        return wlo.tabulate(trees, self.seed_name, weights), ess

    def run(self, prefix, D, table=None, burnin=0.0, philox=PHILOX_SEED, mt=MT_SEED):
        h = host.PhyloHMM(self.c.yaml, 0, self.c.pdir, mt)
        return h.run_weighted_lineage_pipeline(table or self.table, self.seed_name, str(self.tmp / prefix), 4, burnin, D,
                                               philox)

    def cli(self, prefix, D, table=None, env=None, extra=(), seed=PHILOX_SEED):
        e = dict(os.environ)
        e.update(env or {})
        return subprocess.run([_exe(), "--weighted-lineage-pipeline", "--yaml-path", self.c.yaml, "--cluster-ind", "0",
                               "--hmm-param-dir", self.c.pdir, "--input-path", table or self.table, "--output-path",
                               str(self.tmp / prefix), "--seed-seq", self.seed_name, "--num-rates", "4", "--draws-per-row",
                               str(D), "--seed", str(seed)] + list(extra), capture_output=True, text=True, timeout=600,
                              env=e)

    def same(self, a, b, files=ALL_FILES):
        for ext in files:
            assert open(str(self.tmp / a) + ext, "rb").read() == open(str(self.tmp / b) + ext, "rb").read(), (a, b, ext)


@pytest.fixture(scope="module")
def tables(hip, tmp_path_factory):
    return Tables(hip, tmp_path_factory.mktemp("weighted_lineage"))


# ---- 3. the pipeline against the weighted oracle ----

def test_the_prescribed_weights_matter(tables):
    """On the CPU, from g alone: the Kish ESS is neither the row count nor a handful; and the unweighted tables of draw 0
    exercise the counting rules (test_lineage_cpu.something_to_count)."""
    _, ess = wlo.weights_of(tables.g.tolist())
    print("kish ess %.6g of %d rows" % (ess, N_ROWS))
    assert 0.2 * N_ROWS < ess < 0.8 * N_ROWS
    from tests import lineage_oracle as lo
    something_to_count(lo.tabulate(tables.lineages(0), tables.seed_name), [len(ch) for ch in tables.c.chains])


@pytest.mark.parametrize("D", [1, 4])
def test_pipeline_matches_the_weighted_oracle(tables, D):
    """Order, kinds and sequences exactly; sums and fractions (those inside names too) to 1e-9: g_i is reproduced to
    about 1e-12 (a log-likelihood of a few hundred, rounded twice) and the sums are short."""
    got = tables.run("lib_d%d" % D, D)
    want, ess = tables.expected(D, tables.g)
    compare_weighted(str(tables.tmp / ("lib_d%d" % D)), want, 1e-9)
    s = got["summary"]
    assert (s["rows"], s["rows_used"], s["rows_skipped_nonfinite"], s["draws_per_row"]) == (N_ROWS * D, N_ROWS, 0, D)
    assert s["longest_path"] == max(len(ch) for ch in tables.c.chains)
    assert abs(s["kish_ess"] - ess) <= 1e-9 * ess
    rows = got["rows"]
    assert [r["row"] for r in rows] == list(range(N_ROWS))
    for r, g, ll, ch in zip(rows, tables.g, tables.ll, tables.c.chains):
        assert abs(r["log_weight"] - g) <= 1e-9 and abs(r["lh_loglik"] - ll) <= 1e-12 * abs(ll), r
        assert r["path_len"] == len(ch)
    top = max(tables.g)
    assert all(abs(r["weight"] - math.exp(g - top)) <= 1e-9 for r, g in zip(rows, tables.g))
    # naive_id numbers the rows' naive sequences (`--pipeline --seed 3` prints them) by first appearance
    order = {}
    assert [r["naive_id"] for r in rows] == [order.setdefault(s, len(order)) for s in tables.naive_text]


# ---- 4. invariances, byte for byte ----

def _grid_table(tables, name, shift=0.0):
    """The table with Likelihood_i = ll_i - g_i rounded to a multiple of 2^-10, plus `shift` (a small whole number).  Such
    values print exactly.  Let u be the smallest ulp among the log-likelihoods (a power of two, far below 2^-10): every
    ll_i and every Likelihood_i is a multiple of u, so ll_i - Likelihood_i is one too, and it is exact while it stays below
    2^53 u in magnitude.  With |g_i| + shift inside that range the shift moves every log-weight by exactly that number and
    leaves lw_i - max lw, hence every weight, as it was."""
    u = min(math.ulp(x) for x in tables.ll)
    assert u <= 2.0 ** -10 and max(abs(tables.g)) + shift + 1.0 < 2.0 ** 53 * u
    vals = [round((ll - g) * 1024.0) / 1024.0 + shift for ll, g in zip(tables.ll, tables.g)]
    return _rewrite_likelihood(tables.c.tsv, str(tables.tmp / name), vals)


def test_cli_batch_size_and_hash_width(tables):
    """`linearham --weighted-lineage-pipeline` writes the library call's bytes; LH_LINEAGE_BATCH=7 (18 batches, the
    largest log-weight met in a late one) and LH_COLLECT_HASH_BITS=6 change nothing but the collision count."""
    D = 2
    tables.run("inv_lib", D, mt=PHILOX_SEED)     # (the CLI has one --seed for both streams)
    r = tables.cli("inv_cli", D)
    assert r.returncode == 0, r.stderr
    tables.same("inv_cli", "inv_lib")
    r = tables.cli("inv_b7", D, env={"LH_LINEAGE_BATCH": "7"})
    assert r.returncode == 0, r.stderr
    tables.same("inv_b7", "inv_lib")
    r = tables.cli("inv_h6", D, env={"LH_COLLECT_HASH_BITS": "6", "LH_LINEAGE_BATCH": "7"})
    assert r.returncode == 0, r.stderr
    tables.same("inv_h6", "inv_lib", ALL_FILES[:4] + (".rows.tsv",))
    s = host.read_lineage(str(tables.tmp / "inv_h6"))["summary"]
    assert s["hash_collisions_resolved"] > 0, s
    assert dict(s, hash_collisions_resolved=0) == host.read_lineage(str(tables.tmp / "inv_lib"))["summary"]
    # another --seed: other naive draws and other ancestral draws
    r = tables.cli("inv_seed", D, seed=78)
    assert r.returncode == 0, r.stderr
    assert open(str(tables.tmp / "inv_seed.dnamap"), "rb").read() != open(str(tables.tmp / "inv_lib.dnamap"), "rb").read()


def test_burn_in_keeps_the_rows_their_draws(tables):
    """--burnin-frac 0.25 drops rows 0 .. 29.  The same table with those rows' Likelihood = inf (log-weight -inf: skipped)
    and no burn-in uses the same rows with the same sample numbers and the same engine words: the four tables are equal
    byte for byte, the per-row lines too; and they are the oracle's tables of rows 30 .. 119."""
    D = 2
    got = tables.run("burn", D, burnin=0.25)
    skipped = _rewrite_likelihood(tables.c.tsv, str(tables.tmp / "skipped.tsv"),
                                  ["inf"] * 30 + (tables.ll - tables.g).tolist()[30:])
    ref = tables.run("burn_ref", D, table=skipped)
    tables.same("burn", "burn_ref", ALL_FILES[:4])
    assert (got["summary"]["rows_used"], got["summary"]["rows_skipped_nonfinite"]) == (90, 0)
    assert (ref["summary"]["rows_used"], ref["summary"]["rows_skipped_nonfinite"]) == (90, 30)
    assert [r["row"] for r in got["rows"]] == list(range(30, N_ROWS))
    a = open(str(tables.tmp / "burn.rows.tsv")).read().split("\n")[1:]
    b = open(str(tables.tmp / "burn_ref.rows.tsv")).read().split("\n")[31:]
    assert a == b
    assert all(r["naive_id"] == -1 and r["weight"] == 0.0 for r in ref["rows"][:30])
    lw = np.concatenate([np.full(30, -np.inf), tables.g[30:]])
    want, ess = tables.expected(D, lw)
    compare_weighted(str(tables.tmp / "burn"), want, 1e-9)
    assert abs(got["summary"]["kish_ess"] - ess) <= 1e-9 * ess


def test_a_constant_added_to_every_likelihood_changes_only_the_rows_table(tables):
    D = 2
    tables.run("grid", D, table=_grid_table(tables, "grid.tsv"))
    tables.run("grid_shift", D, table=_grid_table(tables, "grid_shift.tsv", shift=2.0))
    tables.same("grid", "grid_shift", FILES)
    a, b = (host.read_lineage(str(tables.tmp / p))["rows"] for p in ("grid", "grid_shift"))
    assert all(x["log_weight"] - y["log_weight"] == 2.0 and x["weight"] == y["weight"] for x, y in zip(a, b))


# ---- 5. edges ----

def test_one_row_with_an_infinite_likelihood_is_skipped(tables):
    D, k = 1, 17
    vals = (tables.ll - tables.g).tolist()
    vals[k] = "inf"
    got = tables.run("one_inf", D, table=_rewrite_likelihood(tables.c.tsv, str(tables.tmp / "one_inf.tsv"), vals))
    s = got["summary"]
    assert (s["rows_skipped_nonfinite"], s["rows_used"], s["rows"]) == (1, N_ROWS - 1, N_ROWS - 1)
    lw = tables.g.copy()
    lw[k] = -np.inf
    want, ess = tables.expected(D, lw)     # the other rows keep their words and sample numbers
    compare_weighted(str(tables.tmp / "one_inf"), want, 1e-9)
    assert abs(s["kish_ess"] - ess) <= 1e-9 * ess
    assert got["rows"][k]["naive_id"] == -1 and got["rows"][k]["log_weight"] == -math.inf


def test_pipeline_refusals(tables):
    r = tables.cli("e", 1, extra=["--devices", "0,1"])
    assert r.returncode != 0 and "one device" in r.stderr
    r = tables.cli("e", 65)
    assert r.returncode != 0 and "draws-per-row must be in 1 .. 64" in r.stderr
    r = tables.cli("e", 0)
    assert r.returncode != 0 and "draws-per-row must be in 1 .. 64" in r.stderr
    h = host.PhyloHMM(tables.c.yaml, 0, tables.c.pdir, 3)
    with pytest.raises(RuntimeError, match="nobody"):
        h.run_weighted_lineage_pipeline(tables.table, "nobody", str(tables.tmp / "e"), 4)
    with pytest.raises(RuntimeError, match="naive"):
        h.run_weighted_lineage_pipeline(tables.table, "naive", str(tables.tmp / "e"), 4)
    all_inf = _rewrite_likelihood(tables.c.tsv, str(tables.tmp / "all_inf.tsv"), ["inf"] * N_ROWS)
    with pytest.raises(RuntimeError, match="finite"):
        h.run_weighted_lineage_pipeline(all_inf, tables.seed_name, str(tables.tmp / "e"), 4)
