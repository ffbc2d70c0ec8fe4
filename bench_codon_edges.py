#!/usr/bin/env python3
"""Throughput of the exact amino-acid replacement posteriors along a seed's lineage (K0-K2 + K9 + K15b's tables + K15,
lh_eval_codon_edges_batch_device) on the configs[2] family, inputs resident in HBM: the HIP-event times of the step's
stages -- K9 with the tables (K15b, the rate sum, the naive codons of every codon), the contraction, the weighted reduction
-- beside K14's step at the MRCA (lh_eval_node_codons_batch_device), K12b's edge-writing form on a slice of the rows
(lh_eval_edges_batch_device with `edge`) and the forward sweep's time (lh_profile_read) in the same run.  Not the headline
metric (bench.py is); prints one JSON line.

  python bench_codon_edges.py [--batch 4096] [--steps 3] [--warmup 1] [--preset config2|small] [--seed-tip 1] [--frame 0]
                              [--edge-rows 512] [--out <file>]

One row is checked against tests/codon_edge_oracle.py outside the timed loop."""
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
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--edge-rows", type=int, default=512, help="rows of K12b's edge-writing form (its output is 128 P L bytes a row)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import capi, host
    from oracle import linearham_oracle as orc
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
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    labels = list(o.xmsa_labels)
    T, R, L = len(labels), 4, o.msa.shape[1]
    rows = sf.read_trees_tsv(tsv)
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
    ops_a, brl_a, er_a, pi_a, alpha_a = np.stack(ops), np.stack(brl), pick("er"), pick("pi"), pick("alpha")
    lay = lib.set_codons(fam, args.frame)
    nc, nw = lay["n_codons"], len(lay["window_codon"])
    msa = np.asarray(o.msa)
    n_prune = len({tuple(msa[:, j]) for j in range(L) if (msa[:, j] != 4).any()})

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(ops_a, np.int32), "brlen": t(brl_a, np.float64), "er": t(er_a, np.float64), "pi": t(pi_a, np.float64),
         "alpha": t(alpha_a, np.float64), "path": t(path, np.int32)}
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    outs = {"log_offset": t(pick("likelihood"), np.float64), "loglik": empty(n), "weighted_codon_counts": empty(nc, 4),
            "weighted_aa_counts": empty(nc, 21, 21), "weighted_seed_change": empty(nc, 3), "weight_stats": empty(3)}
    stream = torch.cuda.current_stream().cuda_stream
    tree_ptrs = [d[k].data_ptr() for k in ("ops", "brlen", "er", "pi", "alpha")]
    out_ptrs = {k: v.data_ptr() for k, v in outs.items()}

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
        lib.check(lib.lib.lh_profile_enable(fam, 0))
        return dt

    dt = timed(lambda: lib.eval_codon_edges_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, args.seed_tip,
                                                         out_ptrs, stream))
    tables, contraction, red, groups = lib.codon_edges_profile_read(fam)
    sw = outs["weight_stats"][1].item()
    k15 = {"rows_per_s": n * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
           "kernel_ms_per_step": {"K9 + tables": tables / args.steps, "contraction": contraction / args.steps,
                                  "reduction": red / args.steps},
           "launch_groups_per_step": groups / args.steps,
           "expected_synonymous": float(outs["weighted_codon_counts"][:, 1].sum().item() / sw),
           "expected_replacement": float(outs["weighted_codon_counts"][:, 2].sum().item() / sw)}
    mean_chain = float(np.mean([len(p) for p in paths]))
    # K15b writes, K15m reads R partial tables of P (n_prune + 1) 80 doubles a row and writes one; K15 reads the live slots
    part_bytes = 8.0 * R * P * (n_prune + 1) * 80
    k15["hbm_bytes_per_row"] = {"K15b partials written": part_bytes, "K15m read": part_bytes, "K15m table written": part_bytes / R,
                                "K15 table read (live slots, at most)": 8.0 * mean_chain * (n_prune + 1) * 80}
    # K14's step at the MRCA on the same rows
    o14 = {"log_offset": outs["log_offset"], "loglik": outs["loglik"], "weighted_codons": empty(nc, 64),
           "weighted_change": empty(nc, 4), "weight_stats": empty(3)}
    p14 = {k: v.data_ptr() for k, v in o14.items()}
    dt14 = timed(lambda: lib.eval_node_codons_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, capi.NODE_MRCA,
                                                           p14, stream))
    t14 = lib.node_codons_profile_read(fam)
    k14 = {"ms_per_step": dt14 / args.steps * 1e3,
           "kernel_ms_per_step": {"K9 + tables": t14[0] / args.steps, "contraction": t14[1] / args.steps, "reduction": t14[2] / args.steps}}
    # K12b's edge-writing form on the first rows
    m = max(1, min(n, args.edge_rows))
    o12 = {"loglik": empty(m), "edge": empty(m, P, L, 16)}
    p12 = {k: v.data_ptr() for k, v in o12.items()}
    dt12 = timed(lambda: lib.eval_edges_batch_device(fam, m, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, args.seed_tip, p12,
                                                     stream))
    t12 = capi.Family.borrow(fam, lib).edges_profile_read()[0]
    k12 = {"rows": m, "ms_per_step": dt12 / args.steps * 1e3, "K12b_ms_per_step": t12["k12b_ms"] / args.steps,
           "K12b_us_per_row": t12["k12b_ms"] / args.steps / m * 1e3}
    k15["tables_us_per_row"] = tables / args.steps / n * 1e3
    # the forward sweep of a plain evaluation of the same rows
    eo = capi._EvalOutputs()
    timed(lambda: lib.check(lib.lib.lh_eval_batch_device(fam, n, T, depth, *tree_ptrs, R, outs["loglik"].data_ptr(),
                                                         C.byref(eo), C.c_void_p(stream))))
    ms = [C.c_double() for _ in range(3)]
    launches = C.c_int64()
    lib.check(lib.lib.lh_profile_read(fam, C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2]), C.byref(launches)))
    lib.check(lib.lib.lh_family_status(fam))

    # parity outside the timed loop: row 0
    from tests import ancestral_marginal_oracle as amo
    from tests import codon_edge_oracle as ceo
    from tests import codon_oracle as co
    r = rows[0]
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
    o.initialize_phylo_emission()
    o.log_likelihood()
    Q = co.dense(o, args.frame)[0]
    children, root, brlen = trees[0]
    tables_ = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")
    res = lib.eval_codon_edges_batch(fam, T, depth, ops_a[:1], brl_a[:1], er_a[:1], pi_a[:1], alpha_a[:1], R, [paths[0]],
                                     args.seed_tip, want=tables_)
    pi0, rates0 = np.asarray(r["pi"], dtype=float), orc.gamma_rates_mean(r["alpha"], R)
    pre = amo.prepare(children, root, brlen, T, o.msa, r["er"], pi0, rates0)
    H = ceo.cond_edges(children, root, brlen, T, o.msa, r["er"], pi0, rates0, paths[0], args.seed_tip, pre=pre)
    want = ceo.tables(Q, H, args.frame)
    worst = max(float(np.abs(res[k][0] - want[k]).max()) for k in tables_)
    if not worst < 1e-8:
        raise SystemExit("parity failure: the lineage's replacement tables differ from the oracle by %.3g" % worst)
    st = outs["weight_stats"].cpu().numpy()
    out = {"metric": "exact lineage amino-acid replacement rows/sec (K0-K2 + K9 + K15b tables + K15 + weighted reduction)",
           "value": k15["rows_per_s"], "unit": "rows/s",
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "n_sites": L, "n_prune": n_prune, "n_codons": nc,
                      "n_window": nw, "frame": args.frame, "path_len": P, "mean_chain": mean_chain, "seed_tip": args.seed_tip,
                      "steps": args.steps},
           "k15": k15, "k14_mrca": k14, "k12_edge_form": k12, "forward_K2_ms_per_step": ms[2].value / args.steps,
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"max_abs_err": worst}}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
