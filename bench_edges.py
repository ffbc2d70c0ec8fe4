#!/usr/bin/env python3
"""Throughput of the exact substitution posteriors along a seed's lineage (K0-K2 + K5 + K12, lh_eval_edges_batch_device)
on the configs[2] family, inputs resident in HBM, in both forms of K12b -- the lean one (chain_counts, the seed edge, the
naive edge and edge_load, reduced to importance-weighted sums on the device) and the one that also writes every edge's
table -- and K11b's time from lh_eval_ancestral_batch_device on the same rows in the same run.  Not the headline metric
(bench.py is); prints one JSON line.

  python bench_edges.py [--batch 4096] [--steps 3] [--warmup 1] [--preset config2|small] [--seed-tip 1]

The three calls alternate inside every step, each warmed up with its own shapes first; the kernel times are HIP events on
the launch stream (lh_edges_profile_read, lh_ancestral_profile_read), the rows/s a host clock around a synchronise.  One row
is checked against tests/edge_oracle.py outside the timed loop."""
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
    tip = args.seed_tip
    rows = sf.read_trees_tsv(tsv)
    ops, brl, paths, trees, depth = [], [], [], [], 0
    for i in range(n):
        r = rows[i % len(rows)]
        children, root, brlen = host.newick_arrays(r["tree"], labels)
        op, dp = lib.schedule_tree(T, children, root)
        ops.append(op), brl.append(brlen), paths.append(capi.seed_path(T, children, root, tip))
        trees.append((children, root, brlen))
        depth = max(depth, dp)
    path = capi.pad_paths(paths)
    P = path.shape[1]
    pick = lambda k: np.array([rows[i % len(rows)][k] for i in range(n)], dtype=np.float64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(np.stack(ops), np.int32), "brlen": t(np.stack(brl), np.float64), "er": t(pick("er"), np.float64),
         "pi": t(pick("pi"), np.float64), "alpha": t(pick("alpha"), np.float64), "path": t(path, np.int32)}
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    offset = t(pick("likelihood"), np.float64)
    lean = {"log_offset": offset, "loglik": new(n), "weighted_counts": new(L, 4, 4), "weighted_seed_edge": new(L, 4, 4),
            "weighted_naive_edge": new(L, 5, 4), "edge_load": new(n, P + 1), "weight_stats": new(3)}
    full = dict(lean, edge=new(n, P, L, 4, 4))
    k11 = {"log_offset": offset, "loglik": new(n), "weighted_sum": new(2, L, 4), "weighted_rate": new(L, R),
           "weight_stats": new(3)}
    stream = torch.cuda.current_stream().cuda_stream
    tree_ptrs = [d[k].data_ptr() for k in ("ops", "brlen", "er", "pi", "alpha")]
    ptrs = lambda outs: {k: v.data_ptr() for k, v in outs.items()}

    def edges(outs):
        lib.eval_edges_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, tip, ptrs(outs), stream)

    def ancestral():
        lib.eval_ancestral_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, ptrs(k11), stream)
    calls = {"lean": lambda: edges(lean), "edge": lambda: edges(full), "k11": ancestral}
    for _ in range(max(1, args.warmup)):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    lib.check(lib.lib.lh_family_status(fam))
    lib.check(lib.lib.lh_profile_enable(fam, 1))
    wall = {k: 0.0 for k in calls}
    ms = {k: [0.0, 0.0, 0.0] for k in calls}
    groups = 0
    for _ in range(args.steps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[k] += time.perf_counter() - t0
            r = lib.ancestral_profile_read(fam) if k == "k11" else lib.edges_profile_read(fam)
            ms[k] = [a + b for a, b in zip(ms[k], r[:3])]
            groups = r[3]
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_family_status(fam))
    per = lambda k: [x / args.steps for x in ms[k]]
    # parity outside the timed loop
    from tests import edge_oracle as eo
    from tests import posterior_oracle as po
    worst = 0.0
    for i in range(args.check):
        r = rows[i % len(rows)]
        res = lib.eval_edges_batch(fam, T, depth, np.stack(ops[i:i + 1]), np.stack(brl[i:i + 1]), [r["er"]], [r["pi"]],
                                   [r["alpha"]], R, [paths[i]], tip,
                                   want=("site_base", "edge", "naive_edge", "chain_counts", "edge_load"))
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        q = po.site_base(o, po.smoothing(o))
        children, root, brlen = trees[i]
        want = eo.edges(children, root, brlen, T, o.msa, q, r["er"], np.asarray(r["pi"]), orc.gamma_rates_mean(r["alpha"], R),
                        paths[i], tip)
        k = len(paths[i])
        load = np.concatenate([res["edge_load"][0, :k], res["edge_load"][0, -1:]])
        worst = max(worst, float(np.abs(res["site_base"][0] - q).max()), float(np.abs(res["edge"][0, :k] - want["edge"]).max()),
                    float(np.abs(res["naive_edge"][0] - want["naive_edge"]).max()),
                    float(np.abs(res["chain_counts"][0] - want["chain_counts"]).max()),
                    float(np.abs(load - want["edge_load"]).max()))
    if not worst < 1e-9:
        raise SystemExit("parity failure: edge tables differ from the oracle by %.3g" % worst)
    st = lean["weight_stats"].cpu().numpy()
    mean_load = float(lean["edge_load"].sum(dim=1).mean().cpu())
    form = lambda k, name: {"rows_per_s": n * args.steps / wall[k], "ms_per_step": wall[k] / args.steps * 1e3,
                            "kernel_ms_per_step": {"K11a": per(k)[0], name: per(k)[1], "reduction": per(k)[2]}}
    out = {"metric": "exact lineage-substitution rows/sec (K0-K2 + K5 + K12 lean + weighted reduction)",
           "value": n * args.steps / wall["lean"], "unit": "tree samples/s",
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "n_sites": L, "path_len": P,
                      "mean_chain": float(np.mean([len(p) for p in paths])), "seed_tip": tip, "steps": args.steps,
                      "launch_groups_last_call": groups},
           "lean": form("lean", "K12b"), "edge_writing": form("edge", "K12b"), "ancestral": form("k11", "K11b"),
           "k12b_vs_k11b": {"K12b_lean_ms": per("lean")[1], "K12b_edge_ms": per("edge")[1], "K11b_ms": per("k11")[1],
                            "lean_over_k11b": per("lean")[1] / per("k11")[1] if per("k11")[1] > 0 else None,
                            "edge_over_k11b": per("edge")[1] / per("k11")[1] if per("k11")[1] > 0 else None},
           "mean_expected_substitutions_per_row": mean_load,
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"rows": args.check, "max_abs_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
