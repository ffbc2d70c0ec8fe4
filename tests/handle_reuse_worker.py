"""Helper of tests/test_gpu_posterior.py::test_one_handle_through_every_entry_point (its own process: the device-pointer
entry points take torch tensors, and torch brings its own HIP runtime, which has to come up first).

One family handle, with profiling on, runs every entry point of the C ABI in turn -- lh_eval_batch (all four outputs),
lh_forward_batch, lh_eval_sample_batch, lh_eval_viterbi_batch, lh_viterbi_forward_batch, lh_eval_draw_batch,
lh_eval_posterior_batch (all outputs), lh_family_set_codons + lh_eval_codons_batch, lh_family_set_candidates +
lh_eval_candidates_batch, lh_asr_batch, lh_lineage_batch, lh_eval_lineage_batch, then the _device forms -- for batch
sizes that grow and then shrink.  Within a size, neighbours share a buffer of the handle: K4, K8 and the draws
out.states, K5, K9 and K6 the forward arrays, the weights and log_offset, the ancestral draws, the lineages and the
chain out.anc.  Every result is compared with the same call on a fresh handle, and every profile counter is read after
each call and once more.  Prints one JSON line: the mismatches and the profile readings that were not what the call
implies (both lists empty when all is well)."""
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [3, 20, 57, 9, 1]  # grow, then shrink
R = 4


def main():
    import numpy as np
    import torch
    from linearham_amd import host
    from linearham_amd.capi import (Family, _CandidateOutputs, _CodonOutputsDevice, _EvalOutputs, _PosteriorOutputs,
                                    load_library)
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_dir = tempfile.mkdtemp(prefix="lh_reuse_")
    sf.generate(sf.Spec.small(locus="igh", n_samples=max(SIZES), seed=23), out_dir)
    yaml_path, pdir, tsv = (os.path.join(out_dir, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    hip = load_library()
    lib = hip.lib
    for fn in (lib.lh_scaler_size, lib.lh_forward_size):
        fn.argtypes, fn.restype = [C.c_void_p], C.c_int64

    def handle():
        h = host.PhyloHMM(yaml_path, 0, pdir, 0)
        return h, h.flatten_tsv(tsv, max(SIZES))

    keep, fl = handle()
    fam = C.c_void_p(fl["family"])
    sizes = keep.sizes()
    T, depth, L, n_xmsa = fl["n_tips"], fl["max_depth"], sizes["n_sites"], sizes["n_xmsa"]
    FS, SS = lib.lh_forward_size(fam), lib.lh_scaler_size(fam)
    NW, NS = lib.lh_sample_words(fam), lib.lh_sample_states(fam)
    rng = np.random.default_rng(5)
    N = max(SIZES)
    words = rng.integers(0, 1 << 32, size=(N, NW), dtype=np.uint64).astype(np.uint32)
    naive = rng.integers(0, 5, size=(N, L)).astype(np.uint8)
    log_offset = rng.normal(-50.0, 5.0, size=N)
    asr_rates = np.ascontiguousarray(np.tile([0.3, 0.7, 1.2, 1.8], (N, 1)))
    # the lineage path of the last tip of every tree (as tests/batch_boundaries_worker.py's Fam builds it)
    labels = list(orc.PhyloHMM(yaml_path, 0, pdir, 0).xmsa_labels)
    chains = []
    for i, s in enumerate(sf.read_trees_tsv(tsv)[:N]):
        children, root, _ = host.newick_arrays(s["tree"], labels)
        assert np.array_equal(hip.schedule_tree(T, children, root)[0], fl["ops"][i])  # flatten_tsv's node numbers
        parent = {}
        for v in range(T, 2 * T - 2):
            parent[int(children[2 * (v - T)])] = parent[int(children[2 * (v - T) + 1])] = v
        chains.append([parent[T - 1]])
        while chains[-1][-1] != root:
            chains[-1].append(parent[chains[-1][-1]])
    PL = max(len(c) for c in chains)
    path = np.full((N, PL), -1, dtype=np.int32)
    for i, c in enumerate(chains):
        path[i, :len(c)] = c
    DRAWS, K = 2, 5
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    d = lambda a: C.c_void_p(a.data_ptr())
    P = lambda a: C.cast(d(a), C.POINTER(C.c_double))

    def inputs(n):
        return [np.ascontiguousarray(fl[k][:n]) for k in ("ops", "brlen", "er", "pi", "alpha")]

    def host_inputs(n):
        ops, brlen, er, pi, alpha = inputs(n)
        return [p(ops, C.c_int32), p(brlen, C.c_double), p(er, C.c_double), p(pi, C.c_double), p(alpha, C.c_double)], \
            (ops, brlen, er, pi, alpha)

    def dev_inputs(n):
        ts = [torch.from_numpy(a).to(dev) for a in inputs(n)]
        return [d(t) for t in ts], ts

    def eval_batch(f, n):
        ptrs, _keep = host_inputs(n)
        ll, rates, em = np.zeros(n), np.zeros((n, R)), np.zeros((n, n_xmsa))
        fwd, sc = np.zeros((n, FS)), np.zeros((n, SS), dtype=np.int32)
        outs = _EvalOutputs(p(rates, C.c_double), p(em, C.c_double), p(fwd, C.c_double), p(sc, C.c_int32))
        hip.check(lib.lh_eval_batch(f, n, T, depth, *ptrs, R, p(ll, C.c_double), C.byref(outs)))
        return [ll, rates, em, fwd, sc]

    def forward_batch(f, n):
        em = emissions[n]
        ll, fwd, sc = np.zeros(n), np.zeros((n, FS)), np.zeros((n, SS), dtype=np.int32)
        outs = _EvalOutputs(None, None, p(fwd, C.c_double), p(sc, C.c_int32))
        hip.check(lib.lh_forward_batch(f, n, p(em, C.c_double), p(ll, C.c_double), C.byref(outs)))
        return [ll, fwd, sc]

    def sample_batch(f, n):
        ptrs, _keep = host_inputs(n)
        ll, rates, st = np.zeros(n), np.zeros((n, R)), np.zeros((n, NS), dtype=np.int32)
        w = np.ascontiguousarray(words[:n])
        hip.check(lib.lh_eval_sample_batch(f, n, T, depth, *ptrs, R, p(w, C.c_uint32), p(ll, C.c_double),
                                           p(rates, C.c_double), p(st, C.c_int32)))
        return [ll, rates, st]

    def posterior_batch(f, n):
        ops, brlen, er, pi, alpha = inputs(n)
        res = hip.eval_posterior_batch(f.value, T, depth, ops, brlen, er, pi, alpha, R, log_offset=log_offset[:n])
        return [res[k] for k in ("loglik", "posterior", "weighted_sum", "weight_stats")]

    def asr_batch(f, n):
        ptrs, _keep = host_inputs(n)
        anc, choice = np.zeros((n, T - 2, L), dtype=np.uint8), np.zeros((n, L), dtype=np.uint8)
        r, nv = np.ascontiguousarray(asr_rates[:n]), np.ascontiguousarray(naive[:n])
        hip.check(lib.lh_asr_batch(f, n, T, depth, *ptrs[:4], p(r, C.c_double), R, p(nv, C.c_uint8), 17, 3,
                                   p(anc, C.c_uint8), p(choice, C.c_uint8)))
        return [anc, choice]

    def viterbi_batch(f, n):
        keys = ("loglik", "states", "log_path", "weight_stats")
        res = hip.eval_viterbi_batch(f.value, T, depth, *inputs(n), R, log_offset=log_offset[:n], want=keys)
        return [res[k] for k in keys]

    def viterbi_forward(f, n):
        return list(hip.viterbi_forward_batch(f.value, emissions[n]))

    def draw_batch(f, n):
        ll, hsh, st = hip.eval_draw_batch(f.value, T, depth, *inputs(n), R, words[:n], want_states=True)
        return [ll, hsh, st, hip.draws_rows_read(f.value, np.arange(n))]

    def codons_batch(f, n):
        hip.set_codons(f.value, 0)
        res = hip.eval_codons_batch(f.value, T, depth, *inputs(n), R, log_offset=log_offset[:n])
        return [res[k] for k in ("loglik", "windows", "genes", "weighted_windows", "weighted_genes", "weight_stats")]

    def candidates_batch(f, n):
        prior = hip.set_candidates(f.value, cands)
        res = hip.eval_candidates_batch(f.value, T, depth, *inputs(n), R, log_offset=log_offset[:n])
        return [prior] + [res[k] for k in ("loglik", "log_cand", "weighted_sum", "weight_stats")]

    def lineage_batch(f, n):
        ops, brlen, er, pi, _ = inputs(n)
        return list(Family.borrow(f.value, hip).lineage_batch(T, depth, ops, brlen, er, pi, asr_rates[:n], naive[:n], 17,
                                                              path[:n], 3))

    def lineage_eval_batch(f, n):
        res = Family.borrow(f.value, hip).eval_lineage_batch(T, depth, *inputs(n), R, words[:n], 17, path[:n], DRAWS, 3)
        return [res[k] for k in sorted(res)]

    def zeros(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def eval_device(f, n):
        ptrs, _keep = dev_inputs(n)
        ll, rates, em, fwd, sc = zeros(n), zeros(n, R), zeros(n, n_xmsa), zeros(n, FS), zeros(n, SS, dtype=torch.int32)
        outs = _EvalOutputs(P(rates), P(em), P(fwd), C.cast(d(sc), C.POINTER(C.c_int32)))
        hip.check(lib.lh_eval_batch_device(f, n, T, depth, *ptrs, R, d(ll), C.byref(outs), stream))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (ll, rates, em, fwd, sc)]

    def sample_device(f, n):
        ptrs, _keep = dev_inputs(n)
        w = torch.from_numpy(np.ascontiguousarray(words[:n]).view(np.int32)).to(dev)
        ll, rates, st = zeros(n), zeros(n, R), zeros(n, NS, dtype=torch.int32)
        hip.check(lib.lh_eval_sample_batch_device(f, n, T, depth, *ptrs, R, d(w), d(ll), d(rates), d(st), stream))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (ll, rates, st)]

    def posterior_device(f, n):
        ptrs, _keep = dev_inputs(n)
        lo = torch.from_numpy(np.ascontiguousarray(log_offset[:n])).to(dev)
        ll, post, wsum, stats = zeros(n), zeros(n, FS), zeros(FS), zeros(3)
        outs = _PosteriorOutputs(P(lo), P(ll), P(post), P(wsum), P(stats))
        hip.check(lib.lh_eval_posterior_batch_device(f, n, T, depth, *ptrs, R, C.byref(outs), stream))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (ll, post, wsum, stats)]

    def asr_device(f, n):
        ptrs, _keep = dev_inputs(n)
        r = torch.from_numpy(np.ascontiguousarray(asr_rates[:n])).to(dev)
        nv = torch.from_numpy(np.ascontiguousarray(naive[:n])).to(dev)
        anc, choice = zeros(n, T - 2, L, dtype=torch.uint8), zeros(n, L, dtype=torch.uint8)
        hip.check(lib.lh_asr_batch_device(f, n, T, depth, *ptrs[:4], d(r), R, d(nv), 17, 3, d(anc), d(choice), stream))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (anc, choice)]

    def log_offset_device(n):
        return torch.from_numpy(np.ascontiguousarray(log_offset[:n])).to(dev)

    def words_device(n):
        return torch.from_numpy(np.ascontiguousarray(words[:n]).view(np.int32)).to(dev)

    def viterbi_device(f, n):
        ptrs, _keep = dev_inputs(n)
        lo = log_offset_device(n)
        out = dict(loglik=zeros(n), states=zeros(n, NS, dtype=torch.int32), log_path=zeros(n), weight_stats=zeros(3))
        hip.eval_viterbi_batch_device(f.value, n, T, depth, *ptrs, R,
                                      dict({k: v.data_ptr() for k, v in out.items()}, log_offset=lo.data_ptr()), stream)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out.values()]

    def draw_device(f, n):
        ptrs, _keep = dev_inputs(n)
        w = words_device(n)
        ll, hsh, st = zeros(n), zeros(n, dtype=torch.int64), zeros(n, NS, dtype=torch.int32)
        hip.check(lib.lh_eval_draw_batch_device(f, n, T, depth, *ptrs, R, d(w), d(ll), d(hsh), d(st), stream))
        torch.cuda.synchronize()
        return [ll.cpu().numpy(), hsh.cpu().numpy().view(np.uint64), st.cpu().numpy(),
                hip.draws_rows_read(f.value, np.arange(n))]

    def codons_device(f, n):
        lay = hip.set_codons(f.value, 0)
        nw, ng = len(lay["window_codon"]), lay["n_genes"]
        ptrs, _keep = dev_inputs(n)
        lo = log_offset_device(n)
        out = [zeros(n), zeros(n, nw, 125), zeros(n, ng), zeros(nw, 125), zeros(ng), zeros(3)]
        outs = _CodonOutputsDevice(lo.data_ptr(), *[t.data_ptr() for t in out])
        hip.check(lib.lh_eval_codons_batch_device(f, n, T, depth, *ptrs, R, C.byref(outs), stream))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    def candidates_device(f, n):
        prior = hip.set_candidates(f.value, cands)
        ptrs, _keep = dev_inputs(n)
        lo = log_offset_device(n)
        out = [zeros(n), zeros(n, K), zeros(K), zeros(3)]
        outs = _CandidateOutputs(P(lo), *[P(t) for t in out])
        hip.check(lib.lh_eval_candidates_batch_device(f, n, T, depth, *ptrs, R, C.byref(outs), stream))
        torch.cuda.synchronize()
        return [prior] + [t.cpu().numpy() for t in out]

    def lineage_eval_device(f, n):
        _ptrs, ts = dev_inputs(n)
        w, pth = words_device(n), torch.from_numpy(np.ascontiguousarray(path[:n])).to(dev)
        u64 = lambda *shape: zeros(*shape, dtype=torch.int64)
        out = dict(aa_hash=u64(n, DRAWS, PL + 1), loglik=zeros(n), naive=zeros(n, L, dtype=torch.uint8), naive_hash=u64(n),
                   nt_hash=u64(n, DRAWS, PL + 1), rates=zeros(n, R), states=zeros(n, NS, dtype=torch.int32))
        Family.borrow(f.value, hip).eval_lineage_batch_device(
            n, T, depth, *[t.data_ptr() for t in ts], R, w.data_ptr(), 17, 3, DRAWS, pth.data_ptr(), PL,
            {k: v.data_ptr() for k, v in out.items()}, stream)
        torch.cuda.synchronize()
        return [v.cpu().numpy().view(np.uint64) if v.dtype == torch.int64 else v.cpu().numpy() for v in out.values()]

    # entry point -> (call, launch groups it records in each of READERS' counters)
    READERS = ("eval", "asr", "posterior", "candidates", "collect", "lineage", "lineage_eval", "viterbi", "codon")
    calls = [("lh_eval_batch", eval_batch, {"eval": 1}), ("lh_forward_batch", forward_batch, {}),
             ("lh_eval_sample_batch", sample_batch, {"eval": 1}),
             ("lh_eval_viterbi_batch", viterbi_batch, {"eval": 1, "viterbi": 1}),
             ("lh_viterbi_forward_batch", viterbi_forward, {}),
             ("lh_eval_draw_batch", draw_batch, {"eval": 1, "collect": 1}),
             ("lh_eval_posterior_batch", posterior_batch, {"eval": 1, "posterior": 1}),
             ("lh_eval_codons_batch", codons_batch, {"eval": 1, "codon": 1}),
             ("lh_eval_candidates_batch", candidates_batch, {"eval": 1, "candidates": 1}),
             ("lh_asr_batch", asr_batch, {"asr": 1}), ("lh_lineage_batch", lineage_batch, {"asr": 1, "lineage": 1}),
             ("lh_eval_lineage_batch", lineage_eval_batch, {"lineage_eval": 1}),
             ("lh_eval_sample_batch after the chain", sample_batch, {"eval": 1}),
             ("lh_eval_batch_device", eval_device, {"eval": 1}), ("lh_eval_sample_batch_device", sample_device, {"eval": 1}),
             ("lh_eval_viterbi_batch_device", viterbi_device, {"eval": 1, "viterbi": 1}),
             ("lh_eval_draw_batch_device", draw_device, {"eval": 1, "collect": 1}),
             ("lh_eval_posterior_batch_device", posterior_device, {"eval": 1, "posterior": 1}),
             ("lh_eval_codons_batch_device", codons_device, {"eval": 1, "codon": 1}),
             ("lh_eval_candidates_batch_device", candidates_device, {"eval": 1, "candidates": 1}),
             ("lh_asr_batch_device", asr_device, {"asr": 1}),
             ("lh_eval_lineage_batch_device", lineage_eval_device, {"lineage_eval": 1})]
    calls = [(name, call, tuple(groups.get(r, 0) for r in READERS)) for name, call, groups in calls]

    def profile():
        ms, k = [C.c_double() for _ in range(3)], C.c_int64()
        hip.check(lib.lh_profile_read(fam, *[C.byref(x) for x in ms], C.byref(k)))
        a_ms, a_k, p_ms, p_k = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        hip.check(lib.lh_asr_profile_read(fam, C.byref(a_ms), C.byref(a_k)))
        hip.check(lib.lh_posterior_profile_read(fam, C.byref(p_ms), C.byref(p_k)))
        chain_ms, chain_k = Family.borrow(fam.value, hip).lineage_eval_profile_read()
        rest = [hip.candidates_profile_read(fam.value), hip.collect_profile_read(fam.value),
                Family.borrow(fam.value, hip).lineage_profile_read(), tuple(chain_ms.values()) + (chain_k,),
                hip.viterbi_profile_read(fam.value), hip.codon_profile_read(fam.value)]
        return [(k.value, [x.value for x in ms]), (a_k.value, [a_ms.value]), (p_k.value, [p_ms.value])] + \
            [(r[-1], list(r[:-1])) for r in rest]

    # K6's candidates: five distinct naive sequences the family itself draws (on a handle of their own)
    cand_h, cand_fl = handle()
    cand_f = C.c_void_p(cand_fl["family"])
    cands = np.unique(hip.naive_sequences(cand_f.value, sample_batch(cand_f, N)[2])[0], axis=0)[:K]
    cand_h.close()
    assert cands.shape == (K, L)

    hip.check(lib.lh_profile_enable(fam, 1))
    emissions = {}
    mismatches, bad_profile = [], []
    for n in SIZES:
        emissions[n] = np.ascontiguousarray(eval_batch(fam, n)[2])  # lh_forward_batch's input, from this handle
        profile()
        for name, call, groups in calls:
            got = call(fam, n)
            for (k, ms), want_k, reader in zip(profile(), groups, READERS):
                if k != want_k or (k > 0 and not (sum(ms) > 0 and min(ms) >= 0)) or (k == 0 and any(ms)):
                    bad_profile.append([name, n, reader, k, ms])
            for (k, ms), reader in zip(profile(), READERS):
                if k != 0 or any(ms):
                    bad_profile.append([name, n, reader + " (second read)", k, ms])
            fresh_h, fresh_fl = handle()
            want = call(C.c_void_p(fresh_fl["family"]), n)
            fresh_h.close()
            for i, (a, b) in enumerate(zip(got, want)):
                if a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
                    mismatches.append([name, n, i])
    keep.close()
    print(json.dumps({"calls": len(SIZES) * len(calls), "mismatches": mismatches, "bad_profile": bad_profile}))
    shutil.rmtree(out_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
