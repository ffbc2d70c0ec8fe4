#!/usr/bin/env python3
"""Throughput of the lineage step's device work (K3 + K7: lh_asr_batch_device, then lh_lineage_collect_device) on the
configs[2] family, inputs resident in HBM, and K7's share of it.  Not the headline metric (bench.py is); prints one
JSON line.

  python bench_lineage.py [--batch 2048] [--steps 5] [--warmup 1] [--preset config2|config4|small]

The seed is the family's last tip; each sample's path (seed's parent .. root) comes from the product's own tree
arrays.  K7 reads (path length + 1) * L bytes per sample and writes 16 * (P + 1); K3 moves 64 B per (inner node, site)
of the same sample, so K7 should be a small share of the step: `k7_share` is the measured one (HIP events of both
kernels in the same run, lh_lineage_profile_read and lh_asr_profile_read)."""
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
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "config4", "small"])
    args = ap.parse_args()
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import host
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    spec = {"config2": sf.Spec(n_samples=256), "small": sf.Spec.small(n_samples=16),
            "config4": sf.Spec(n_leaves=500, n_sites=600, n_samples=64)}[args.preset]
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_%s_r0" % args.preset)
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    hmm = host.PhyloHMM(os.path.join(fam_dir, "cluster.yaml"), 0, os.path.join(fam_dir, "hmm_params"), 0)
    sizes = hmm.sizes()
    n = args.batch
    flat = hmm.flatten_tsv(os.path.join(fam_dir, "trees.tsv"), n)
    T, depth, R, L = flat["n_tips"], flat["max_depth"], 4, sizes["n_sites"]
    rng = np.random.default_rng(1)
    lib = linearham_amd.load_library()
    fam = C.c_void_p(flat["family"])
    rates = np.zeros((n, R))
    _ll = np.zeros(n)
    from linearham_amd.capi import _EvalOutputs, c_f64p, c_i32p
    outs = _EvalOutputs()
    outs.rates = rates.ctypes.data_as(c_f64p)
    lib.check(lib.lib.lh_eval_batch(fam, n, T, depth, np.ascontiguousarray(flat["ops"]).ctypes.data_as(c_i32p),
                                    np.ascontiguousarray(flat["brlen"]).ctypes.data_as(c_f64p),
                                    flat["er"].ctypes.data_as(c_f64p), flat["pi"].ctypes.data_as(c_f64p),
                                    flat["alpha"].ctypes.data_as(c_f64p), R, _ll.ctypes.data_as(c_f64p),
                                    C.byref(outs)))
    naive = rng.integers(0, 4, size=(n, L)).astype(np.uint8)
    # the paths of the last tip: the table's rows repeat over the batch as flatten_tsv repeats them
    rows = sf.read_trees_tsv(os.path.join(fam_dir, "trees.tsv"))
    from oracle import linearham_oracle as orc
    labels = list(orc.PhyloHMM(os.path.join(fam_dir, "cluster.yaml"), 0, os.path.join(fam_dir, "hmm_params"), 0).xmsa_labels)
    chains = []
    for r in rows:
        children, root, _ = host.newick_arrays(r["tree"], labels)
        children = np.asarray(children).ravel()
        parent = {}
        for v in range(T, 2 * T - 2):
            parent[int(children[2 * (v - T)])] = parent[int(children[2 * (v - T) + 1])] = v
        c = [parent[T - 1]]
        while c[-1] != root:
            c.append(parent[c[-1]])
        chains.append(c)
    P = max(len(c) for c in chains)
    path = np.full((n, P), -1, dtype=np.int32)
    for i in range(n):
        c = chains[i % len(chains)]
        path[i, :len(c)] = c
    d = {k: torch.from_numpy(np.ascontiguousarray(flat[k])).to(dev) for k in ("ops", "brlen", "er", "pi")}
    d_rates, d_naive, d_path = (torch.from_numpy(a).to(dev) for a in (rates, naive, path))
    anc = torch.zeros((n, T - 2, L), dtype=torch.uint8, device=dev)
    nt = torch.zeros((n, P + 1), dtype=torch.int64, device=dev)
    aa = torch.zeros((n, P + 1), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step(seed):
        lib.check(lib.lib.lh_asr_batch_device(fam, n, T, depth, d["ops"].data_ptr(), d["brlen"].data_ptr(),
                                              d["er"].data_ptr(), d["pi"].data_ptr(), d_rates.data_ptr(), R,
                                              d_naive.data_ptr(), seed, 0, anc.data_ptr(), None, C.c_void_p(stream)))
        lib.check(lib.lib.lh_lineage_collect_device(fam, n, T, anc.data_ptr(), d_naive.data_ptr(), d_path.data_ptr(), P,
                                                    nt.data_ptr(), aa.data_ptr(), C.c_void_p(stream)))
    for w in range(args.warmup):
        step(w)
    torch.cuda.synchronize()
    lib.check(lib.lib.lh_profile_enable(fam, 1))
    t0 = time.perf_counter()
    for s in range(args.steps):
        step(100 + s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms3, k3, ms7, k7 = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
    lib.check(lib.lib.lh_asr_profile_read(fam, C.byref(ms3), C.byref(k3)))
    lib.check(lib.lib.lh_lineage_profile_read(fam, C.byref(ms7), C.byref(k7)))
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    # the hashes must separate exactly the distinct sequences of the last step (checked on the first 64 samples)
    a, h_nt = anc.cpu().numpy(), nt.cpu().numpy()
    seen = {}
    for i in range(min(n, 64)):
        c = chains[i % len(chains)]
        for s, v in enumerate(c):
            key = a[i, v - T].tobytes()
            if seen.setdefault(key, int(h_nt[i, s])) != int(h_nt[i, s]):
                raise SystemExit("parity failure: one sequence, two hashes")
    if len(set(seen.values())) != len(seen):
        raise SystemExit("parity failure: two sequences, one hash")
    k3_ms, k7_ms = ms3.value / args.steps, ms7.value / args.steps
    mean_len = float(np.mean([len(chains[i % len(chains)]) for i in range(n)]))
    out = {"metric": "lineage samples/sec (K3 + K7, inputs resident)", "value": n * args.steps / dt,
           "unit": "tree samples/s", "ms_per_step": dt / args.steps * 1e3,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "n_sites": L, "R": R, "path_len_max": P,
                      "path_len_mean": mean_len},
           "kernel_ms_per_step": {"asr_K3": k3_ms, "lineage_K7": k7_ms, "k3_launches": k3.value, "k7_launches": k7.value},
           "k7_share": k7_ms / (k3_ms + k7_ms),
           "k7_bytes_per_sample": {"read": (mean_len + 1) * L, "written": 16 * (P + 1)},
           "distinct_sequences_in_first_64_samples": len(seen)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
