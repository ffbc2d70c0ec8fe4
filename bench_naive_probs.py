#!/usr/bin/env python3
"""Throughput of exact posterior probabilities of candidate naive sequences (K0-K2 + K6b,
lh_eval_candidates_batch_device) on the configs[2] family, inputs resident in HBM.  Not the headline metric (bench.py
is); prints one JSON line.

  python bench_naive_probs.py [--batch 49152] [--steps 5] [--warmup 1] [--candidates 1024] [--preset config2|small]

Candidates are the naive sequences K4 draws in RunPipeline, one per row of the family's tree table, distinct, in
first-appearance order, at most --candidates of them.  Each step evaluates `batch` tree samples and
reduces P(s_k | data, t) over them to one importance-weighted sum per candidate on the device.  K6a (the candidates'
priors) runs once, in lh_family_set_candidates, and is reported on its own.  A few (row, candidate) pairs are checked
against tests/naive_probs_oracle.py outside the timed loop."""
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
    ap.add_argument("--candidates", type=int, default=1024)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    ap.add_argument("--check", type=int, default=2, help="rows checked against the oracle (4 candidates each)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import _CandidateOutputs
    from oracle import linearham_oracle as orc
    from tests import naive_probs_oracle as npo
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
    # candidates: K4's draws (RunPipeline, one per table row), distinct, first-appearance order
    t0 = time.perf_counter()
    draws_path = os.path.join(tempfile.mkdtemp(prefix="lh_bench_k6_"), "draws.tsv")
    host.PhyloHMM(yaml_path, 0, pdir, 0).run_pipeline(tsv, draws_path, R)
    draw_s = time.perf_counter() - t0
    seen, draws = {}, 0
    with open(draws_path) as f:
        c = f.readline().rstrip("\n").split("\t").index("NaiveSequence")
        for line in f:
            draws += 1
            seen.setdefault(line.rstrip("\n").split("\t")[c], None)
            if len(seen) >= args.candidates:
                break
    os.remove(draws_path)
    cands = np.array([["ACGTN".index(ch) for ch in s] for s in seen], dtype=np.uint8)
    K = len(cands)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    hmm = host.PhyloHMM(yaml_path, 0, pdir, 0)
    flat = hmm.flatten_tsv(tsv, n)
    T, depth = flat["n_tips"], flat["max_depth"]
    lib = linearham_amd.load_library()
    fam = C.c_void_p(flat["family"])
    lib.check(lib.lib.lh_profile_enable(fam, 1))
    prior = lib.set_candidates(fam, cands)
    k6a_ms, _, _ = lib.candidates_profile_read(fam)
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    rb = np.array([rows[i % len(rows)]["likelihood"] for i in range(n)])
    d = {k: torch.from_numpy(np.ascontiguousarray(flat[k])).to(dev) for k in ("ops", "brlen", "er", "pi", "alpha")}
    d_rb = torch.from_numpy(rb).to(dev)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    wsum = torch.empty(K, dtype=torch.float64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def P(t):
        return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    outs = _CandidateOutputs(P(d_rb), P(ll), None, P(wsum), P(stats))

    def step():
        lib.check(lib.lib.lh_eval_candidates_batch_device(fam, n, T, depth, d["ops"].data_ptr(), d["brlen"].data_ptr(),
                                                          d["er"].data_ptr(), d["pi"].data_ptr(), d["alpha"].data_ptr(),
                                                          R, C.byref(outs), C.c_void_p(stream)))
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
    _, k6b_ms, k6b_n = lib.candidates_profile_read(fam)
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_family_status(fam))
    split = {"model": ms[0].value / args.steps, "prune": ms[1].value / args.steps, "forward": ms[2].value / args.steps,
             "K6b": k6b_ms / max(k6b_n, 1)}
    # parity outside the timed loop: a few (row, candidate) pairs against the oracle's factorised form
    check = lib.eval_candidates_batch(fam, T, depth, flat["ops"][:args.check], flat["brlen"][:args.check],
                                      flat["er"][:args.check], flat["pi"][:args.check], flat["alpha"][:args.check], R, K,
                                      want=("log_cand", "loglik"))
    worst = 0.0
    picks = [0, K // 3, (2 * K) // 3, K - 1]
    for i in range(args.check):
        r = rows[i % len(rows)]
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        oll = o.log_likelihood()
        for kk in picks:
            want = npo.log_cand(o, cands[kk], oll)
            worst = max(worst, abs(check["log_cand"][i, kk] - want) / (1.0 + 1e-3 * abs(oll)))
    if not worst < 1e-9:
        raise SystemExit("parity failure: log P(s | data, t) differs from the oracle by %.3g" % worst)
    st = stats.cpu().numpy()
    p = wsum.cpu().numpy() / st[1]
    out = {"metric": "candidate naive-sequence posterior rows/sec (K0-K2 + K6b scoring + weighted reduction)",
           "value": n * args.steps / dt, "unit": "tree samples/s", "pairs_per_s": n * K * args.steps / dt,
           "ms_per_step": dt / args.steps * 1e3,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "candidates": K, "draws": draws,
                      "draw_s": draw_s},
           "k6a_ms": k6a_ms, "kernel_ms_per_step": split, "k6b_share": split["K6b"] / (dt / args.steps * 1e3),
           "impossible_candidates": int(np.sum(prior == -np.inf)), "coverage": float(p.sum()),
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"rows": args.check, "candidates": len(picks), "max_scaled_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
