#!/usr/bin/env python3
"""Throughput of the exact ancestral-state marginals along a seed's lineage (K0-K2 + K5 + K11,
lh_eval_ancestral_batch_device) on the configs[2] family, inputs resident in HBM, and K11b's time beside K3's for one
draw per row on the same family in the same run.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_ancestral.py [--batch 4096] [--steps 3] [--warmup 1] [--preset config2|small] [--seed-tip 1]

Each step evaluates `batch` distinct tree samples and reduces the tables of the seed's parent and of the MRCA, and the
rate posteriors, to importance-weighted sums on the device (the per-row tables stay in the handle's scratch).  One row is
checked against tests/ancestral_marginal_oracle.py outside the timed loop."""
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
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    ap.add_argument("--seed-tip", type=int, default=1)
    ap.add_argument("--check", type=int, default=1, help="rows checked against the oracle")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import capi, host
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    n = args.batch
    spec = {"config2": sf.Spec(n_samples=n), "small": sf.Spec.small(n_samples=min(n, 512))}[args.preset]
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_marginals_%s_%d" % (args.preset, spec.n_samples))
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    tsv = os.path.join(fam_dir, "trees.tsv")
    yaml_path, pdir = os.path.join(fam_dir, "cluster.yaml"), os.path.join(fam_dir, "hmm_params")
    hmm = host.PhyloHMM(yaml_path, 0, pdir, 0)
    lib = linearham_amd.load_library()
    fam = C.c_void_p(hmm.flatten_tsv(tsv, 1)["family"])
    from oracle import linearham_oracle as orc
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    labels = list(o.xmsa_labels)
    T, R, L = len(labels), 4, o.msa.shape[1]
    rows = sf.read_trees_tsv(tsv)
    # the trees as the host numbers them, their schedules, and the seed's path in each
    ops, brl, paths, trees, depth = [], [], [], [], 0
    for i in range(n):
        r = rows[i % len(rows)]
        children, root, brlen = host.newick_arrays(r["tree"], labels)
        op, dp = lib.schedule_tree(T, children, root)
        ops.append(op), brl.append(brlen), paths.append(capi.seed_path(T, children, root, args.seed_tip))
        trees.append((children, root, brlen))
        depth = max(depth, dp)
    path = capi.pad_paths(paths)
    P = path.shape[1]
    pick = lambda k: np.array([rows[i % len(rows)][k] for i in range(n)], dtype=np.float64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(np.stack(ops), np.int32), "brlen": t(np.stack(brl), np.float64), "er": t(pick("er"), np.float64),
         "pi": t(pick("pi"), np.float64), "alpha": t(pick("alpha"), np.float64), "path": t(path, np.int32)}
    outs = {"log_offset": t(pick("likelihood"), np.float64),
            "loglik": torch.empty(n, dtype=torch.float64, device=dev),
            "weighted_sum": torch.empty((2, L, 4), dtype=torch.float64, device=dev),
            "weighted_rate": torch.empty((L, R), dtype=torch.float64, device=dev),
            "weight_stats": torch.empty(3, dtype=torch.float64, device=dev)}
    stream = torch.cuda.current_stream().cuda_stream
    tree_ptrs = [d[k].data_ptr() for k in ("ops", "brlen", "er", "pi", "alpha")]

    def step():
        lib.eval_ancestral_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P,
                                        {k: v.data_ptr() for k, v in outs.items()}, stream)
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
    k11a, k11b, red, groups = lib.ancestral_profile_read(fam)
    ms_step = dt / args.steps * 1e3
    split = {"K11a": k11a / args.steps, "K11b": k11b / args.steps, "reduction": red / args.steps}
    split["K0-K2 + K5 (the rest of the step)"] = ms_step - sum(split.values())
    # K3 for one draw per row on the same trees, rates and a naive sequence per row: the sampling kernel's own time
    rates = torch.empty((n, R), dtype=torch.float64, device=dev)
    eo = capi._EvalOutputs()
    eo.rates = C.cast(rates.data_ptr(), C.POINTER(C.c_double))
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_eval_batch_device(fam, n, T, depth, *tree_ptrs, R, outs["loglik"].data_ptr(), C.byref(eo),
                                           C.c_void_p(stream)))
    naive = t(np.random.default_rng(1).integers(0, 4, size=(n, L)), np.uint8)
    anc = torch.empty((n, T - 2, L), dtype=torch.uint8, device=dev)

    def k3():
        lib.check(lib.lib.lh_asr_batch_device(fam, n, T, depth, d["ops"].data_ptr(), d["brlen"].data_ptr(), d["er"].data_ptr(),
                                              d["pi"].data_ptr(), rates.data_ptr(), R, naive.data_ptr(), C.c_uint64(7),
                                              C.c_uint64(0), anc.data_ptr(), None, C.c_void_p(stream)))
    k3()
    torch.cuda.synchronize()
    lib.check(lib.lib.lh_profile_enable(fam, 1))
    for _ in range(args.steps):
        k3()
    torch.cuda.synchronize()
    k3_ms, _ = lib._profile_read("lh_asr_profile_read", fam)
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_family_status(fam))
    # parity outside the timed loop
    from tests import ancestral_marginal_oracle as amo
    from tests import posterior_oracle as po
    worst = 0.0
    for i in range(args.check):
        r = rows[i % len(rows)]
        res = lib.eval_ancestral_batch(fam, T, depth, np.stack(ops[i:i + 1]), np.stack(brl[i:i + 1]), [r["er"]], [r["pi"]],
                                       [r["alpha"]], R, [paths[i]], want=("site_base", "marg", "rate_post"))
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        q = po.site_base(o, po.smoothing(o))
        children, root, brlen = trees[i]
        marg, rp = amo.marginals(children, root, brlen, T, o.msa, q, r["er"], np.asarray(r["pi"]),
                                 orc.gamma_rates_mean(r["alpha"], R), paths[i])
        worst = max(worst, float(np.abs(res["site_base"][0] - q).max()), float(np.abs(res["marg"][0] - marg).max()),
                    float(np.abs(res["rate_post"][0] - rp).max()))
    if not worst < 1e-9:
        raise SystemExit("parity failure: ancestral marginals differ from the oracle by %.3g" % worst)
    st = outs["weight_stats"].cpu().numpy()
    out = {"metric": "exact ancestral-marginal rows/sec (K0-K2 + K5 + K11 + weighted reduction)",
           "value": n * args.steps / dt, "unit": "tree samples/s", "ms_per_step": ms_step,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "n_sites": L, "path_len": P,
                      "mean_chain": float(np.mean([len(p) for p in paths])), "seed_tip": args.seed_tip,
                      "launch_groups_per_step": groups / args.steps},
           "kernel_ms_per_step": split, "k11b_share": split["K11b"] / ms_step,
           "k11b_vs_k3": {"K11b_ms": split["K11b"], "K3_one_draw_ms": k3_ms / args.steps,
                          "ratio": split["K11b"] / (k3_ms / args.steps) if k3_ms > 0 else None},
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"rows": args.check, "max_abs_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
