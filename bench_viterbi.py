#!/usr/bin/env python3
"""Throughput of the most probable annotation per tree sample (K0-K2 + K8, lh_eval_viterbi_batch_device) on the
configs[2] family, inputs resident in HBM.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_viterbi.py [--batch 49152] [--steps 5] [--warmup 1] [--preset config2|small] [--check 1]

Each step evaluates `batch` tree samples and leaves every sample's most probable state path, its log joint probability and
the log-likelihood on the device.  The HIP-event split (model, prune, forward, K8) comes from the library's profiling
calls.  Beside it, from the same process: one lh_eval_sample_batch_device step on the same inputs (K0-K2 + K4, the draw the
annotation counting script relies on), and the exact scoring of the batch's distinct most probable paths on every row
(lh_family_set_candidate_paths once, then K0-K2 + K6b per step).  A few rows are checked against tests/viterbi_oracle.py
outside the timed loops."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=49152)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    ap.add_argument("--check", type=int, default=1, help="rows checked against the oracle")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import _CandidateOutputs, _ViterbiOutputsDevice
    from oracle import linearham_oracle as orc
    from tests import posterior_oracle as po
    from tests import viterbi_oracle as vo
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    n = args.batch
    spec = {"config2": sf.Spec(n_samples=n), "small": sf.Spec.small(n_samples=min(n, 512))}[args.preset]
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_marginals_%s_%d" % (args.preset, spec.n_samples))
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    tsv = os.path.join(fam_dir, "trees.tsv")
    yaml_path, pdir = os.path.join(fam_dir, "cluster.yaml"), os.path.join(fam_dir, "hmm_params")
    rows = sf.read_trees_tsv(tsv)
    R = 4
    hmm = host.PhyloHMM(yaml_path, 0, pdir, 0)
    flat = hmm.flatten_tsv(tsv, n)
    T, depth = flat["n_tips"], flat["max_depth"]
    lib = linearham_amd.load_library()
    fam = C.c_void_p(flat["family"])
    S, n_words = lib.sample_states(fam), int(lib.lib.lh_sample_words(fam))
    d = {k: torch.from_numpy(np.ascontiguousarray(flat[k])).to(dev) for k in ("ops", "brlen", "er", "pi", "alpha")}
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    lp = torch.empty(n, dtype=torch.float64, device=dev)
    st = torch.empty((n, S), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    outs = _ViterbiOutputsDevice(loglik=ll.data_ptr(), states=st.data_ptr(), log_path=lp.data_ptr())
    inputs = (d["ops"].data_ptr(), d["brlen"].data_ptr(), d["er"].data_ptr(), d["pi"].data_ptr(), d["alpha"].data_ptr())

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        lib.check(lib.lib.lh_family_status(fam))
        lib.check(lib.lib.lh_profile_enable(fam, 1))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ms = [C.c_double() for _ in range(3)]
        k = C.c_int64()
        lib.check(lib.lib.lh_profile_read(fam, *[C.byref(x) for x in ms], C.byref(k)))
        lib.check(lib.lib.lh_profile_enable(fam, 0))
        lib.check(lib.lib.lh_family_status(fam))
        return dt / args.steps * 1e3, {"model": ms[0].value / args.steps, "prune": ms[1].value / args.steps,
                                       "forward": ms[2].value / args.steps}

    # K0-K2 + K8
    def viterbi_step():
        lib.check(lib.lib.lh_eval_viterbi_batch_device(fam, n, T, depth, *inputs, R, C.byref(outs), C.c_void_p(stream)))
    step_ms, split = timed(viterbi_step)
    k8_ms, k8_n = lib.viterbi_profile_read(fam)
    split["K8"] = k8_ms / args.steps
    states, log_path, loglik = st.cpu().numpy(), lp.cpu().numpy(), ll.cpu().numpy()

    # beside it: K0-K2 + K4 (lh_eval_sample_batch_device) on the same inputs
    words = torch.from_numpy(np.random.default_rng(0).integers(0, 2 ** 32, (n, n_words), dtype=np.uint64)
                             .astype(np.uint32).view(np.int32)).to(dev)

    def sample_step():
        lib.check(lib.lib.lh_eval_sample_batch_device(fam, n, T, depth, *inputs, R, words.data_ptr(), ll.data_ptr(), None,
                                                      st.data_ptr(), C.c_void_p(stream)))
    sample_ms, sample_split = timed(sample_step)

    # path scoring: the batch's distinct most probable paths, scored exactly on every row (K6b)
    ok = states[:, 0] >= 0
    distinct = np.unique(states[ok], axis=0)
    t0 = time.perf_counter()
    prior = lib.set_candidate_paths(fam, distinct)
    register_ms = (time.perf_counter() - t0) * 1e3
    K = len(distinct)
    wsum = torch.empty(K, dtype=torch.float64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    d_rb = torch.from_numpy(np.array([rows[i % len(rows)]["likelihood"] for i in range(n)])).to(dev)

    def P(t):
        return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    couts = _CandidateOutputs(P(d_rb), P(ll), None, P(wsum), P(stats))

    def score_step():
        lib.check(lib.lib.lh_eval_candidates_batch_device(fam, n, T, depth, *inputs, R, C.byref(couts), C.c_void_p(stream)))
    score_ms, score_split = timed(score_step)
    _, k6b_ms, k6b_n = lib.candidates_profile_read(fam)
    split["path_scoring_K6b"] = k6b_ms / max(k6b_n, 1)
    sw = stats.cpu().numpy()
    covered = float((wsum.cpu().numpy() / sw[1]).sum())

    # parity outside the timed loops
    worst = 0.0
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    for i in range(args.check):
        r = rows[i % len(rows)]
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        ref = vo.viterbi(o, po.emission_count(o))
        if not np.array_equal(vo.to_states(o, ref["path"]), states[i]):
            raise SystemExit("parity failure: row %d's path differs from the oracle's (margin %.3g)" % (i, ref["margin"]))
        worst = max(worst, abs(log_path[i] - ref["log_path"]) / (1.0 + abs(ref["log_path"])))
    if not worst < 1e-10:
        raise SystemExit("parity failure: log_path differs from the oracle by %.3g" % worst)
    out = {"metric": "most probable annotation rows/sec (K0-K2 + K8 sweep and trace-back)",
           "value": n / step_ms * 1e3, "unit": "tree samples/s", "ms_per_step": step_ms,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "states_per_path": S},
           "kernel_ms_per_step": split, "k8_share": split["K8"] / step_ms,
           "k8_over_prune": split["K8"] / split["prune"] if split["prune"] > 0 else None,
           "k8_over_forward": split["K8"] / split["forward"] if split["forward"] > 0 else None,
           "sample_batch": {"ms_per_step": sample_ms, "kernel_ms_per_step": sample_split},
           "path_scoring": {"distinct_map_paths": K, "register_ms": register_ms, "ms_per_step": score_ms,
                            "kernel_ms_per_step": score_split, "covered_mass": covered,
                            "impossible_paths": int(np.sum(~np.isfinite(prior)))},
           "rows_without_path": int((~ok).sum()),
           "mean_log_path_posterior": float(np.mean((log_path - loglik)[ok])),
           "parity": {"rows": args.check, "max_scaled_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
