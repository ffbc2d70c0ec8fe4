"""Helper of tests/test_gpu_batch_boundaries.py: one case per process (LH_CHUNK and LH_HOST_SUB are read once per process,
and the device-pointer entry points take torch tensors, whose HIP runtime has to come up first).

    python -m tests.batch_boundaries_worker CASE DIR [key=value ...]

DIR holds the families and anchors.npz, both written by the test module's fixture (build_anchors below, in the pytest
process).  A case makes its large calls, compares them as the module's docstring says and prints one JSON line:
{"failures": [...], "info": {...}}.  A failure names the entry point, the output, the first bad row, row % group and
row // group."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SETS = 23            # prime to every boundary
MT_SEED = 3            # the std::mt19937 stream of the anchors' naive draws
PHILOX = 20261017
BASES = "ACGTN"
EVAL_KEYS = ("loglik", "rates", "xmsa_emission", "forward", "scaler_counts")
ALL4 = EVAL_KEYS[1:]
TOY = os.path.join(ROOT, "tests", "golden", "data")


def pick(n, G):
    """Row i of a batch is anchor row pick[i]: position p of group k and of group k + 1 hold different rows."""
    i = np.arange(n)
    return (i * 7 + i // G) % N_SETS


def p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def mt_words(seed, n_rows, per_row):
    from oracle import linearham_oracle as orc
    rng = orc.MT19937(seed)
    return np.array([rng() for _ in range(n_rows * per_row)], dtype=np.uint32).reshape(n_rows, per_row)


class Fam:
    """A synthetic family (tools.synth_family.Spec.small, ragged reads and ambiguous bases), its 23 tree samples as
    device inputs, the lineage paths of its last tip and a borrowed handle of the host's family (sampler tables)."""

    def __init__(self, d, locus="igh"):
        import linearham_amd
        from linearham_amd import host
        from oracle import linearham_oracle as orc
        from tools import synth_family as sf
        self.hip = hip = linearham_amd.load_library()
        out = os.path.join(d, locus)
        if not os.path.exists(os.path.join(out, "trees.tsv")):
            sf.generate(sf.Spec.small(locus=locus, n_samples=N_SETS, ragged=4, ambiguous=0.02), out)
        self.yaml, self.pdir, self.tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
        self.rows = sf.read_trees_tsv(self.tsv)
        assert len(self.rows) == N_SETS
        self.o = orc.PhyloHMM(self.yaml, 0, self.pdir, MT_SEED)
        self.labels = list(self.o.xmsa_labels)
        self.T, self.L = self.o.msa.shape[0] + 1, self.o.msa.shape[1]
        T = self.T
        ops, brl, self.chains, self.trees, self.depth = [], [], [], [], 0
        for s in self.rows:
            children, root, brlen = host.newick_arrays(s["tree"], self.labels)   # the host parser's node numbers
            o, dep = hip.schedule_tree(T, children, root)
            ops.append(o), brl.append(brlen)
            self.depth = max(self.depth, dep)
            self.trees.append((children, root, brlen))
            ch = np.asarray(children).ravel()
            parent = {}
            for v in range(T, 2 * T - 2):
                parent[int(ch[2 * (v - T)])] = parent[int(ch[2 * (v - T) + 1])] = v
            c = [parent[T - 1]]
            while c[-1] != root:
                c.append(parent[c[-1]])
            self.chains.append(c)
        self.P = max(len(c) for c in self.chains)
        self.path = np.full((N_SETS, self.P), -1, dtype=np.int32)
        for i, c in enumerate(self.chains):
            self.path[i, :len(c)] = c
        self.ops, self.brl = np.stack(ops).astype(np.int32), np.stack(brl)
        self.er = np.array([s["er"] for s in self.rows])
        self.pi = np.array([s["pi"] for s in self.rows])
        self.alpha = np.array([s["alpha"] for s in self.rows])
        self.rb = np.array([s["likelihood"] for s in self.rows])
        self.open()

    def open(self):
        """A fresh host object and family handle (the old ones, if any, stay alive until close)."""
        from linearham_amd import capi, host
        self.h = host.PhyloHMM(self.yaml, 0, self.pdir, MT_SEED)
        self.fam = capi.Family.borrow(self.h.flatten_tsv(self.tsv, 1)["family"], self.hip)
        self.fam.n_xmsa = self.h.sizes()["n_xmsa"]
        lib = self.hip.lib
        self.NW, self.NS = lib.lh_sample_words(self.fam.handle), lib.lh_sample_states(self.fam.handle)
        self.FS, self.SS = self.fam.forward_size, self.fam.scaler_size
        f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lib.lh_eval_sample_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, i32] + [f64] * 4 + \
            [C.c_int32, C.POINTER(C.c_uint32), f64, f64, i32]

    def inputs(self, pk):
        return [np.ascontiguousarray(a[pk]) for a in (self.ops, self.brl, self.er, self.pi, self.alpha)]

    # ---- the entry points, host pointers ----
    def eval(self, pk, R, want=ALL4):
        ll, res = self.fam.eval_batch(self.T, self.depth, *self.inputs(pk), R, want=want)
        return dict(res, loglik=ll)

    def sample(self, pk, words, R=4):
        n = len(pk)
        ops, brl, er, pi, alpha = self.inputs(pk)
        ll, st = np.zeros(n), np.zeros((n, self.NS), dtype=np.int32)
        w = np.ascontiguousarray(words, dtype=np.uint32)
        assert w.shape == (n, self.NW)
        self.hip.check(self.hip.lib.lh_eval_sample_batch(
            self.fam.handle, n, self.T, self.depth, p(ops, C.c_int32), p(brl, C.c_double), p(er, C.c_double),
            p(pi, C.c_double), p(alpha, C.c_double), R, p(w, C.c_uint32), p(ll, C.c_double), None, p(st, C.c_int32)))
        return dict(loglik=ll, states=st)

    def posterior(self, pk, R=4):
        ops, brl, er, pi, alpha = self.inputs(pk)
        return self.hip.eval_posterior_batch(self.fam, self.T, self.depth, ops, brl, er, pi, alpha, R,
                                             log_offset=np.ascontiguousarray(self.rb[pk]))

    def asr(self, pk, rates, naive, first, seed=PHILOX):
        ops, brl, er, pi, _ = self.inputs(pk)
        anc, choice = self.fam.asr_batch(self.T, self.depth, ops, brl, er, pi, np.ascontiguousarray(rates[pk]),
                                         np.ascontiguousarray(naive[pk]), seed, first)
        return dict(anc=anc, rate_choice=choice)

    def lineage(self, pk, rates, naive, first, seed=PHILOX, per_row=False):
        """rates and naive: of the 23 anchor rows, or (per_row) of the batch's rows."""
        ops, brl, er, pi, _ = self.inputs(pk)
        if not per_row:
            rates, naive = rates[pk], naive[pk]
        nt, aa = self.fam.lineage_batch(self.T, self.depth, ops, brl, er, pi, np.ascontiguousarray(rates),
                                        np.ascontiguousarray(naive), seed, np.ascontiguousarray(self.path[pk]), first)
        return dict(nt_hash=nt, aa_hash=aa)

    def chain(self, pk, words, D, first, R=4, seed=PHILOX):
        ops, brl, er, pi, alpha = self.inputs(pk)
        return self.fam.eval_lineage_batch(self.T, self.depth, ops, brl, er, pi, alpha, R, words, seed,
                                           np.ascontiguousarray(self.path[pk]), D, first)

    def oracle_rates(self, R):
        from oracle import linearham_oracle as orc
        return np.stack([orc.gamma_rates_mean(a, R) for a in self.alpha])

    def asr_oracle_mismatches(self, j, naive, rates, sample_no, anc=None, choice=None, slots=None, seed=PHILOX):
        """Sites at which oracle/asr_oracle.py's draw of anchor row j at `sample_no` differs from the device's: the rate
        category, and -- where that agrees -- any node (anc [T-2][L]) or any of the path's nodes (slots [len][L])."""
        from oracle import asr_oracle as ao
        children, root, brlen = self.trees[j]
        c_ref, a_ref, _ = ao.asr_sample(children, root, brlen, self.T, self.o.msa, naive, self.rows[j]["er"],
                                        np.asarray(self.rows[j]["pi"]), rates, seed, sample_no)
        if slots is not None:
            want = np.stack([a_ref[v - self.T] for v in self.chains[j]])
            return int((want != slots).any(axis=0).sum())
        same = c_ref == choice if choice is not None else np.ones(self.L, dtype=bool)
        return int((~same).sum()) + int((a_ref[:, same] != anc[:, same]).any(axis=0).sum())

    def close(self):
        self.fam.close()
        self.h.close()


class Report:
    def __init__(self):
        self.failures, self.info = [], {}

    def bits(self, what, key, got, want, G):
        """got == want bit for bit, row by row; the first bad row otherwise."""
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            self.failures.append("%s %s: shape %s, expected %s" % (what, key, got.shape, want.shape))
            return
        a = got.reshape(got.shape[0], -1)
        b = want.reshape(want.shape[0], -1)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a != b).any(axis=1))[0]
        if len(bad):
            i = int(bad[0])
            self.failures.append("%s %s: %d rows differ, first bad row %d (row %% group %d, row // group %d of group %d)"
                                 % (what, key, len(bad), i, i % G, i // G, G))

    def all_bits(self, what, got, want, G, keys=None):
        for k in keys or sorted(want):
            self.bits(what, k, got[k], want[k], G)

    def check(self, cond, msg):
        if not cond:
            self.failures.append(msg)

    def done(self):
        print(json.dumps({"failures": self.failures, "info": self.info}))


def anchors_of(A, prefix, pk):
    return {k[len(prefix):]: A[k][pk] for k in A.files if k.startswith(prefix)}


# ---- the anchors: the 23 rows as one 23-row call (in the pytest process; the test module checks them on the CPU) ----

def toy_family():
    """The toy heavy-chain family of tests/golden with 23 varied models, every sequence of non-zero prior as the
    candidate set: (oracle, handle, inputs, candidates [K][L])."""
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tests import naive_probs_oracle as npo
    hip = linearham_amd.load_library()
    o = orc.PhyloHMM(os.path.join(TOY, "phylo_hmm_input.yaml"), 0, os.path.join(TOY, "hmm_params"), 0)
    rng = np.random.default_rng(5)
    sets = []
    for _ in range(N_SETS):
        bl = rng.exponential(0.2, size=5) + 1e-6
        sets.append(dict(tree="((0:%.17g,1:%.17g):%.17g,naive:%.17g,2:%.17g);" % tuple(bl),
                         er=rng.dirichlet(np.ones(6)).tolist(), pi=rng.dirichlet(np.ones(4) * 2).tolist(),
                         alpha=float(max(rng.exponential(1.0), 0.05))))
    T = o.msa.shape[0] + 1
    ops, brl, depth = [], [], 0
    for s in sets:
        children, root, brlen = db.tree_arrays(orc.parse_newick(s["tree"]), o.xmsa_labels)
        op, d = hip.schedule_tree(T, children, root)
        ops.append(op), brl.append(brlen)
        depth = max(depth, d)
    s = sets[0]
    o.initialize_phylo_parameters(s["tree"], s["er"], s["pi"], s["alpha"], 4, is_path=False)
    o.initialize_phylo_emission()
    o.log_likelihood()
    cands = np.array(sorted(npo.by_enumeration(o)), dtype=np.uint8)
    fam = linearham_amd.Family(db.build_family_desc(o), hip)
    hip.set_candidates(fam, cands, n_sites=o.msa.shape[1])
    inp = dict(T=T, depth=depth, ops=np.stack(ops).astype(np.int32), brl=np.stack(brl),
               er=np.array([s["er"] for s in sets]), pi=np.array([s["pi"] for s in sets]),
               alpha=np.array([s["alpha"] for s in sets]), log_offset=rng.normal(-60.0, 2.0, size=N_SETS))
    return o, fam, sets, inp, cands


def toy_candidates(hip, fam, inp, pk):
    return hip.eval_candidates_batch(fam, inp["T"], inp["depth"], inp["ops"][pk], inp["brl"][pk], inp["er"][pk],
                                     inp["pi"][pk], inp["alpha"][pk], 4, log_offset=np.ascontiguousarray(inp["log_offset"][pk]))


def build_anchors(d):
    """Writes d/anchors.npz and returns its contents as a dict."""
    F = Fam(d, "igh")
    ident = np.arange(N_SETS)
    A = {}
    for R in (4, 8):
        for ext in (0, 1):
            F.fam.set_extended_range(bool(ext))
            for k, v in F.eval(ident, R).items():
                A["eval_R%d_x%d_%s" % (R, ext, k)] = v
    F.fam.set_extended_range(False)
    for k, v in F.sample(ident, mt_words(MT_SEED, N_SETS, F.NW)).items():
        A["sample_" + k] = v
    A["naive"], A["naive_hash"] = F.hip.naive_sequences(F.fam, A["sample_states"])
    res = F.posterior(ident)
    A["post_posterior"], A["post_loglik"] = res["posterior"], res["loglik"]
    F.close()
    K = Fam(d, "igk")
    for k, v in K.eval(ident, 4).items():
        A["igk_eval_" + k] = v
    K.close()
    o, fam, sets, inp, cands = toy_family()
    res = toy_candidates(fam.hip, fam, inp, ident)
    A["cand_log_cand"], A["cand_loglik"] = res["log_cand"], res["loglik"]
    fam.close()
    np.savez(os.path.join(d, "anchors.npz"), **A)
    return A


# ---- the cases ----

def case_eval_host(d, rep, n, G, R=4, ext=0, locus="igh"):
    """a, b: lh_eval_batch on host pointers, all four optional outputs."""
    F = Fam(d, locus)
    A = np.load(os.path.join(d, "anchors.npz"))
    F.fam.set_extended_range(bool(ext))
    pk = pick(n, G)
    prefix = "igk_eval_" if locus == "igk" else "eval_R%d_x%d_" % (R, ext)
    rep.all_bits("lh_eval_batch n=%d R=%d ext=%d %s" % (n, R, ext, locus), F.eval(pk, R), anchors_of(A, prefix, pk), G,
                 EVAL_KEYS)
    rep.info["k1_form"] = F.fam.k1_form()
    F.close()


def case_eval_device(d, rep, n, G, R=4):
    """c: lh_eval_batch_device on torch tensors, the null stream and a stream of torch's."""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    from linearham_amd.capi import _EvalOutputs
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    pk = pick(n, G)
    want = anchors_of(A, "eval_R%d_x0_" % R, pk)
    ts = [torch.from_numpy(a).to(dev) for a in F.inputs(pk)]
    dp = lambda t: C.c_void_p(t.data_ptr())
    for name, stream in (("null stream", None), ("torch stream", torch.cuda.Stream(device=dev))):
        out = dict(loglik=torch.full((n,), 0.5, dtype=torch.float64, device=dev),
                   rates=torch.zeros((n, R), dtype=torch.float64, device=dev),
                   xmsa_emission=torch.zeros((n, F.fam.n_xmsa), dtype=torch.float64, device=dev),
                   forward=torch.zeros((n, F.FS), dtype=torch.float64, device=dev),
                   scaler_counts=torch.full((n, F.SS), -7, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        f64 = lambda t: C.cast(dp(t), C.POINTER(C.c_double))
        outs = _EvalOutputs(f64(out["rates"]), f64(out["xmsa_emission"]), f64(out["forward"]),
                            C.cast(dp(out["scaler_counts"]), C.POINTER(C.c_int32)))
        F.hip.check(F.hip.lib.lh_eval_batch_device(F.fam.handle, n, F.T, F.depth, *[dp(t) for t in ts], R,
                                                   dp(out["loglik"]), C.byref(outs),
                                                   C.c_void_p(stream.cuda_stream if stream else 0)))
        torch.cuda.synchronize()
        F.fam.status()
        rep.all_bits("lh_eval_batch_device n=%d %s" % (n, name), {k: v.cpu().numpy() for k, v in out.items()}, want, G,
                     EVAL_KEYS)
    F.close()


def _row_words(F, n, seed=1):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=(n, F.NW), dtype=np.uint64).astype(np.uint32)


def _sample_reference(F, pk, words):
    """Every row in a 23-row call of its own neighbourhood, keeping its words."""
    n = len(pk)
    ll, st = np.zeros(n), np.zeros((n, F.NS), dtype=np.int32)
    for s in range(0, n, N_SETS):
        sl = slice(s, min(s + N_SETS, n))
        r = F.sample(pk[sl], words[sl])
        ll[sl], st[sl] = r["loglik"], r["states"]
    return dict(loglik=ll, states=st)


def case_sample(d, rep, n, G):
    """d: lh_eval_sample_batch and lh_eval_sample_batch_device, every row its own engine words."""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    # the 23-row call of this process reproduces the anchors (which the oracle's draws pinned)
    rep.all_bits("lh_eval_sample_batch 23 rows", F.sample(np.arange(N_SETS), mt_words(MT_SEED, N_SETS, F.NW)),
                 anchors_of(A, "sample_", np.arange(N_SETS)), N_SETS)
    pk = pick(n, G)
    words = _row_words(F, n)
    want = _sample_reference(F, pk, words)
    got = F.sample(pk, words)
    rep.all_bits("lh_eval_sample_batch n=%d" % n, got, want, G)
    rep.check(len({r.tobytes() for r in want["states"][pk == 0]}) > 1, "rows of one anchor row with different words all "
              "drew the same states: the words do not reach the draw")
    ts = [torch.from_numpy(a).to(dev) for a in F.inputs(pk)]
    w = torch.from_numpy(words.view(np.int32)).to(dev)
    ll = torch.full((n,), 0.5, dtype=torch.float64, device=dev)
    st = torch.full((n, F.NS), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    dp = lambda t: C.c_void_p(t.data_ptr())
    F.hip.check(F.hip.lib.lh_eval_sample_batch_device(F.fam.handle, n, F.T, F.depth, *[dp(t) for t in ts], 4, dp(w),
                                                      dp(ll), None, dp(st), C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize()
    rep.all_bits("lh_eval_sample_batch_device n=%d" % n, dict(loglik=ll.cpu().numpy(), states=st.cpu().numpy()), want, G)
    F.close()


def _host_sums(rows, loglik, log_offset):
    """(max lw, weights, weighted column sums, sum w, sum w^2) in long double from the call's own per-row outputs."""
    lw = loglik - log_offset
    w = np.exp((lw - lw.max()).astype(np.longdouble))
    return lw.max(), (w[:, None] * rows.astype(np.longdouble)).sum(axis=0), w.sum(), (w * w).sum()


def _check_reduction(rep, what, n, res, rows, log_offset):
    """weighted_sum and weight_stats against the long-double host sum: n * 2^-52 relative per entry.  Every term is
    non-negative, so (n - 1) 2^-53 bounds the error of ANY summation order; the rest of the bound covers the weight's
    exp and the product's rounding."""
    mx, ws, s1, s2 = _host_sums(rows, res["loglik"], log_offset)
    bound = n * 2.0 ** -52
    got = res["weighted_sum"].astype(np.longdouble)
    rel = np.abs(got - ws) / np.where(ws > 0, ws, 1)
    rel = np.where(ws > 0, rel, np.abs(got))
    rep.info[what + " weighted_sum worst relative error / bound"] = float(rel.max() / bound)
    rep.check(bool((rel <= bound).all()), "%s weighted_sum: entry %d is off by %.3g relative, bound %.3g"
              % (what, int(rel.argmax()), float(rel.max()), bound))
    st = res["weight_stats"]
    rep.check(st[0] == mx, "%s weight_stats[0] = %.17g, max lw = %.17g" % (what, st[0], mx))
    for k, s in ((1, s1), (2, s2)):
        rep.check(abs(st[k] - s) <= bound * s, "%s weight_stats[%d] = %.17g, host sum %.17g" % (what, k, st[k], float(s)))


def case_posterior(d, rep, ns, G):
    """e: lh_eval_posterior_batch; group (1024) and slab (256) edges that coincide and miss."""
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    for n in ns:
        pk = pick(n, G)
        what = "lh_eval_posterior_batch n=%d" % n
        res = F.posterior(pk)
        rep.bits(what, "posterior", res["posterior"], A["post_posterior"][pk], G)
        rep.bits(what, "loglik", res["loglik"], A["post_loglik"][pk], G)
        _check_reduction(rep, what, n, res, res["posterior"], F.rb[pk])
        again = F.posterior(pk)
        for k in ("weighted_sum", "weight_stats"):
            rep.check(np.array_equal(again[k], res[k]), "%s %s: the same call twice gives different bits" % (what, k))
    F.close()


def case_candidates(d, rep, ns, G):
    """f: lh_eval_candidates_batch on an enumerated-complete candidate set."""
    A = np.load(os.path.join(d, "anchors.npz"))
    o, fam, sets, inp, cands = toy_family()
    for n in ns:
        pk = pick(n, G)
        what = "lh_eval_candidates_batch n=%d" % n
        res = toy_candidates(fam.hip, fam, inp, pk)
        rep.bits(what, "log_cand", res["log_cand"], A["cand_log_cand"][pk], G)
        rep.bits(what, "loglik", res["loglik"], A["cand_loglik"][pk], G)
        prob = np.exp(res["log_cand"])
        worst = np.abs(prob.sum(axis=1) - 1.0)
        rep.check(bool((worst < 1e-12).all()), "%s: row %d sums to 1 %+.3g" % (what, int(worst.argmax()), worst.max()))
        _check_reduction(rep, what, n, res, prob, inp["log_offset"][pk])
        again = toy_candidates(fam.hip, fam, inp, pk)
        for k in ("weighted_sum", "weight_stats"):
            rep.check(np.array_equal(again[k], res[k]), "%s %s: the same call twice gives different bits" % (what, k))
    fam.close()


def case_draw(d, rep, n, G):
    """g: lh_eval_draw_batch against lh_naive_sequences of lh_eval_sample_batch's states (case d pins those)."""
    F = Fam(d)
    pk = pick(n, G)
    words = _row_words(F, n)
    smp = F.sample(pk, words)
    seqs, hsh = F.hip.naive_sequences(F.fam, smp["states"])
    ll, got_hash, st = F.hip.eval_draw_batch(F.fam, F.T, F.depth, *F.inputs(pk), 4, words, want_states=True)
    what = "lh_eval_draw_batch n=%d" % n
    rep.bits(what, "states", st, smp["states"], G)
    rep.bits(what, "loglik", ll, smp["loglik"], G)
    rep.bits(what, "hash", got_hash, hsh, G)
    rows = sorted({0, n - 1} | {b + k for b in range(G, n, G) for k in (-1, 0, 1) if b + k < n})
    rep.bits("lh_draws_rows_read after " + what, "bases of rows %s" % rows, F.hip.draws_rows_read(F.fam, rows), seqs[rows],
             1)
    rep.check(len({s.tobytes() for s in seqs}) > N_SETS, "the draws hardly vary: %d distinct sequences"
              % len({s.tobytes() for s in seqs}))
    F.close()


def _boundary_rows(n, G):
    return sorted({0, n - 1} | {b + k for b in range(G, n, G) for k in (-2, -1, 0, 1, 2) if 0 <= b + k < n})


def case_asr(d, rep, n, G, first=5):
    """h: lh_asr_batch and lh_asr_batch_device (rate_choice null) past the 8192-row group."""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    naive = A["naive"]
    pk = pick(n, G)
    b = (n // G) * G if n % G else n - G
    for R in (4, 3):
        rates = F.oracle_rates(R)
        what = "lh_asr_batch n=%d R=%d" % (n, R)
        big = F.asr(pk, rates, naive, first)
        rep.check(int(big["anc"].max()) <= 3 and int(big["rate_choice"].max()) < R, what + ": a state out of range")
        mism = sites = 0
        for i in _boundary_rows(n, G):
            j = int(pk[i])
            mism += F.asr_oracle_mismatches(j, naive[j], rates[j], first + i, big["anc"][i], big["rate_choice"][i])
            sites += F.L
        rep.info[what + " oracle mismatches / sites"] = [mism, sites]
        # tests/test_gpu_asr.py's bound: a uniform within rounding distance of a category boundary, a handful per million
        rep.check(mism <= max(1, sites // 200000), "%s: %d of %d sites of rows %s differ from asr_oracle at sample "
                  "number first_sample + row" % (what, mism, sites, _boundary_rows(n, G)))
        tail = F.asr(pk[b - 2:], rates, naive, first + b - 2)
        head = F.asr(pk[:N_SETS], rates, naive, first)
        for k in ("anc", "rate_choice"):
            rep.bits(what + " against rows [%d, n) alone" % (b - 2), k, big[k][b - 2:], tail[k], 1)
            rep.bits(what + " against rows [0, 23) alone", k, big[k][:N_SETS], head[k], 1)
        for j in range(N_SETS):
            rep.check(len({a.tobytes() for a in big["anc"][pk == j]}) > 1,
                      "%s: every row of anchor row %d drew the same states whatever its sample number" % (what, j))
        if R != 4:
            continue
        ops, brl, er, pi, _ = [torch.from_numpy(a).to(dev) for a in F.inputs(pk)]
        rt, nv = torch.from_numpy(np.ascontiguousarray(rates[pk])).to(dev), torch.from_numpy(naive[pk]).to(dev)
        anc = torch.full((n, F.T - 2, F.L), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        dp = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        F.hip.check(F.hip.lib.lh_asr_batch_device(F.fam.handle, n, F.T, F.depth, dp(ops), dp(brl), dp(er), dp(pi), dp(rt), R,
                                                  dp(nv), PHILOX, first, dp(anc), None, C.c_void_p(stream)))
        torch.cuda.synchronize()
        F.fam.status()
        rep.bits("lh_asr_batch_device n=%d, rate_choice null" % n, "anc", anc.cpu().numpy(), big["anc"], G)
    F.close()


def _hash_classes(rep, what, seqs, nt, aa):
    """Two slots have equal hashes exactly when their sequences (their translations) are equal."""
    from tests import lineage_oracle as lo
    by_nt, by_aa = {}, {}
    for s, a, b in zip(seqs, nt.tolist(), aa.tolist()):
        key = s.tobytes()
        if key not in by_nt:
            by_nt[key] = a
            t = lo.translate("".join(BASES[x] for x in s))
            if by_aa.setdefault(t, b) != b:
                rep.failures.append(what + ": one translation, two aa hashes")
                return by_nt
        elif by_nt[key] != a:
            rep.failures.append(what + ": one sequence, two nt hashes")
            return by_nt
    rep.check(len(set(by_nt.values())) == len(by_nt), what + ": two sequences share an nt hash")
    rep.check(len(set(by_aa.values())) == len(by_aa), what + ": two translations share an aa hash")
    return by_nt


def case_lineage(d, rep, n, G, first=5):
    """i: lh_lineage_batch past the 8192-row group, on case h's inputs."""
    from linearham_amd import capi
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    naive, rates = A["naive"], F.oracle_rates(4)
    pk = pick(n, G)
    b = (n // G) * G if n % G else n - G
    what = "lh_lineage_batch n=%d" % n
    anc = F.asr(pk, rates, naive, first)["anc"]          # case h pins these
    big = F.lineage(pk, rates, naive, first)
    nt, aa = big["nt_hash"], big["aa_hash"]
    P, T = F.P, F.T
    rep.bits(what, "slot P against K6c's hash of the naive sequence", nt[:, P], A["naive_hash"][pk], G)
    length = np.array([len(F.chains[j]) for j in pk])
    valid = np.arange(P)[None, :] < length[:, None]
    rep.check(bool((nt[:, :P][~valid] == capi.LINEAGE_PAD_HASH).all() and (aa[:, :P][~valid] == capi.LINEAGE_PAD_HASH).all()),
              what + ": a padding slot without the sentinel")
    node = np.where(valid, F.path[pk] - T, 0)
    seqs = anc[np.arange(n)[:, None], node]              # [n][P][L]
    all_seqs = np.concatenate([seqs[valid], naive[pk]])
    _hash_classes(rep, what, all_seqs, np.concatenate([nt[:, :P][valid], nt[:, P]]),
                  np.concatenate([aa[:, :P][valid], aa[:, P]]))
    # the slots of the handle's batch are lh_asr_batch's bases
    rows = _boundary_rows(n, G)
    slots = [i * (P + 1) + s for i in rows for s in range(length[i])]
    rep.bits("lh_lineage_rows_read after " + what, "bases of rows %s" % rows, F.fam.lineage_rows_read(slots),
             np.concatenate([seqs[i, :length[i]] for i in rows]), 1)
    tail = F.lineage(pk[b - 2:], rates, naive, first + b - 2)
    head = F.lineage(pk[:N_SETS], rates, naive, first)
    for k in ("nt_hash", "aa_hash"):
        rep.bits(what + " against rows [%d, n) alone" % (b - 2), k, big[k][b - 2:], tail[k], 1)
        rep.bits(what + " against rows [0, 23) alone", k, big[k][:N_SETS], head[k], 1)
    F.close()


def case_chain(d, rep, n, G, D, first=5, R=4):
    """j: lh_eval_lineage_batch and its device form against the composition of the separately tested entry points."""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    F = Fam(d)
    pk = pick(n, G)
    words = _row_words(F, n, seed=D)
    what = "lh_eval_lineage_batch n=%d D=%d" % (n, D)
    got = F.chain(pk, words, D, first, R)
    P, P1 = F.P, F.P + 1
    length = np.array([len(F.chains[j]) for j in pk])
    # 1. the handle's batch, before another call replaces it: bases, the store
    rows = sorted({0, n - 1} | {b + k for b in range(G, n, G) for k in (-1, 0, 1) if b + k < n})
    rates = F.oracle_rates(R)
    mism = sites = 0
    for i in rows:
        j = int(pk[i])
        for dd in range(D):
            sl = F.fam.lineage_rows_read([(i * D + dd) * P1 + s for s in range(length[i])])
            mism += F.asr_oracle_mismatches(j, got["naive"][i], rates[j], first + i + (dd << 32), slots=sl)
            sites += F.L
    rep.info[what + " oracle mismatches / sites"] = [mism, sites]
    rep.check(mism <= max(1, sites // 200000), "%s: %d of %d sites of rows %s differ from asr_oracle at sample number "
              "first_sample + row + (d << 32)" % (what, mism, sites, rows))
    valid = np.zeros((n, D, P1), dtype=bool)
    valid[:, :, :P] = (np.arange(P)[None, :] < length[:, None])[:, None, :]
    valid[:, :, P] = True
    flat = np.nonzero(valid.reshape(-1))[0].astype(np.int32)
    bases = F.fam.lineage_rows_read(flat)
    by_nt = _hash_classes(rep, what, bases, got["nt_hash"].reshape(-1)[flat], got["aa_hash"].reshape(-1)[flat])
    order = {}
    ids = np.full(n * D * P1, -1, dtype=np.int32)
    ids[flat] = [order.setdefault(s.tobytes(), len(order)) for s in bases]
    bad = F.fam.lineage_resolve(ids)
    rep.check(len(bad) == 0, "%s: lh_lineage_resolve reports %d mismatches, first slot %s" % (what, len(bad), bad[:1]))
    stored = F.fam.lineage_store_read()
    rep.check(stored.shape[0] == len(order) == len(by_nt), "%s: the store holds %d rows, %d distinct sequences, %d "
              "distinct hashes" % (what, stored.shape[0], len(order), len(by_nt)))
    rep.info[what + " slots / distinct sequences"] = [int(len(flat)), len(order)]
    # 2. the composition
    ev = F.eval(pk, R, want=("rates",))
    rel = np.abs(got["loglik"] - ev["loglik"]) / np.abs(ev["loglik"])
    rep.check(bool((rel <= 1e-12).all()), "%s loglik: first bad row %d" % (what, int(np.argmax(rel > 1e-12))))
    rep.bits(what, "rates", got["rates"], ev["rates"], G)
    rep.bits(what, "states", got["states"], F.sample(pk, words, R)["states"], G)
    seqs, hsh = F.hip.naive_sequences(F.fam, got["states"])
    rep.bits(what, "naive", got["naive"], seqs, G)
    rep.bits(what, "naive_hash", got["naive_hash"], hsh, G)
    for dd in range(D):
        lin = F.lineage(pk, got["rates"], got["naive"], first + (dd << 32), per_row=True)
        rep.bits(what, "nt_hash of draw %d" % dd, got["nt_hash"][:, dd], lin["nt_hash"], G)
        rep.bits(what, "aa_hash of draw %d" % dd, got["aa_hash"][:, dd], lin["aa_hash"], G)
    # 3. the device form
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    ops, brl, er, pi, alpha = F.inputs(pk)
    d_in = [t(ops, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64)]
    d_words, d_path = t(words.view(np.int32), np.int32), t(F.path[pk], np.int32)
    res = dict(loglik=torch.full((n,), 0.5, dtype=torch.float64, device=dev),
               rates=torch.zeros((n, R), dtype=torch.float64, device=dev),
               states=torch.zeros((n, F.NS), dtype=torch.int32, device=dev),
               naive=torch.full((n, F.L), 0x55, dtype=torch.uint8, device=dev),
               naive_hash=torch.full((n,), 0x55, dtype=torch.int64, device=dev),
               nt_hash=torch.full((n, D, P1), 0x55, dtype=torch.int64, device=dev),
               aa_hash=torch.full((n, D, P1), 0x55, dtype=torch.int64, device=dev))
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    F.fam.eval_lineage_batch_device(n, F.T, F.depth, *[x.data_ptr() for x in d_in], R, d_words.data_ptr(), PHILOX, first, D,
                                    d_path.data_ptr(), P, {k: v.data_ptr() for k, v in res.items()},
                                    C.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    F.fam.status()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("naive_hash", "nt_hash", "aa_hash"):
        out[k] = out[k].view(np.uint64)
    rep.all_bits("lh_eval_lineage_batch_device n=%d D=%d" % (n, D), out, got, G)
    F.close()


def case_stale(d, rep, n, G):
    """k: a large call, then the 23-row call on one handle; the reverse on a fresh handle."""
    F = Fam(d)
    A = np.load(os.path.join(d, "anchors.npz"))
    naive, rates = A["naive"], F.oracle_rates(4)
    ident, pk = np.arange(N_SETS), pick(n, G)
    w23, wn = mt_words(MT_SEED, N_SETS, F.NW), _row_words(F, n)
    calls = [("lh_eval_batch", lambda q, w: F.eval(q, 4)), ("lh_eval_sample_batch", lambda q, w: F.sample(q, w)),
             ("lh_eval_posterior_batch", lambda q, w: F.posterior(q)),
             ("lh_asr_batch", lambda q, w: F.asr(q, rates, naive, 5)),
             ("lh_lineage_batch", lambda q, w: F.lineage(q, rates, naive, 5)),
             ("lh_eval_lineage_batch", lambda q, w: F.chain(q, w, 3, 5))]
    for name, call in calls:
        big_a, small_a = call(pk, wn), call(ident, w23)
        old = (F.h, F.fam)
        F.open()
        small_b, big_b = call(ident, w23), call(pk, wn)
        rep.all_bits(name + ": 23 rows after %d rows against 23 rows on a fresh handle" % n, small_a, small_b, N_SETS)
        rep.all_bits(name + ": %d rows on a fresh handle against %d rows after 23" % (n, n), big_a, big_b, G)
        old[1].close(), old[0].close()
    for k in EVAL_KEYS:
        rep.bits("lh_eval_batch 23 rows after a large call", k, F.eval(ident, 4)[k], A["eval_R4_x0_" + k], N_SETS)
    F.close()


CASES = {"eval_host": case_eval_host, "eval_device": case_eval_device, "sample": case_sample, "posterior": case_posterior,
         "candidates": case_candidates, "draw": case_draw, "asr": case_asr, "lineage": case_lineage, "chain": case_chain,
         "stale": case_stale}


def main(argv):
    case, d = argv[0], argv[1]
    kw = {}
    for a in argv[2:]:
        k, v = a.split("=")
        kw[k] = v if k == "locus" else [int(x) for x in v.split(",")] if k == "ns" else int(v)
    rep = Report()
    CASES[case](d, rep, **kw)
    rep.done()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv[1:])
