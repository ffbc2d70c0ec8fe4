#!/usr/bin/env python3
"""Throughput of the exact codon marginals of a lineage node (K0-K2 + K9 + K13's tables + K14,
lh_eval_node_codons_batch_device) on the configs[2] family, inputs resident in HBM, at both nodes (the seed's parent, the
MRCA): the HIP-event times of the step's stages -- K9 with the tables (K13b, the naive codons of every codon), the
contraction, the weighted reduction -- beside K9's own time on the same rows (lh_eval_codons_batch_device) and the forward
sweep's (lh_profile_read) in the same run.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_node_codons.py [--batch 4096] [--steps 3] [--warmup 1] [--preset config2|small] [--seed-tip 1] [--frame 0]
                              [--with-tip <tip>] [--out <file>]

--with-tip names a second tip: the run then also times the slot form (lh_eval_node_codons_at_batch_device) at the most
recent common ancestor of the two tips, a slot of its own per row, and reports it beside the two fixed nodes.

One row is checked against tests/node_codon_oracle.py outside the timed loop."""
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
    ap.add_argument("--with-tip", type=int, default=0, help="a second tip: also time K14 at its common ancestor with the seed")
    ap.add_argument("--frame", type=int, default=0)
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
    ops, brl, paths, trees, depth, slots = [], [], [], [], 0, []
    for i in range(n):
        r = rows[i % len(rows)]
        children, root, brlen = host.newick_arrays(r["tree"], labels)
        op, dp = lib.schedule_tree(T, children, root)
        ops.append(op), brl.append(brlen), paths.append(capi.seed_path(T, children, root, args.seed_tip))
        trees.append((children, root, brlen))
        if args.with_tip:
            slots.append(capi.clade_slot(T, children, root, args.seed_tip, [args.with_tip])[1])
        depth = max(depth, dp)
    path = capi.pad_paths(paths)
    P = path.shape[1]
    pick = lambda k: np.array([rows[i % len(rows)][k] for i in range(n)], dtype=np.float64)
    ops_a, brl_a, er_a, pi_a, alpha_a = np.stack(ops), np.stack(brl), pick("er"), pick("pi"), pick("alpha")
    lay = lib.set_codons(fam, args.frame)
    nc, nw, ng = lay["n_codons"], len(lay["window_codon"]), lay["n_genes"]

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(ops_a, np.int32), "brlen": t(brl_a, np.float64), "er": t(er_a, np.float64), "pi": t(pi_a, np.float64),
         "alpha": t(alpha_a, np.float64), "path": t(path, np.int32)}
    outs = {"log_offset": t(pick("likelihood"), np.float64),
            "loglik": torch.empty(n, dtype=torch.float64, device=dev),
            "weighted_codons": torch.empty((nc, 64), dtype=torch.float64, device=dev),
            "weighted_change": torch.empty((nc, 4), dtype=torch.float64, device=dev),
            "weight_stats": torch.empty(3, dtype=torch.float64, device=dev)}
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

    per_node = {}
    if args.with_tip:
        d["slot"] = t(slots, np.int32)
    for name, node in (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA)) + ((("slot", None),) if args.with_tip else ()):
        if node is None:
            dt = timed(lambda: lib.eval_node_codons_at_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P,
                                                                    d["slot"].data_ptr(), out_ptrs, stream))
        else:
            dt = timed(lambda: lib.eval_node_codons_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, node,
                                                                 out_ptrs, stream))
        tables, contraction, red, groups = lib.node_codons_profile_read(fam)
        per_node[name] = {"rows_per_s": n * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                          "kernel_ms_per_step": {"K9 + tables": tables / args.steps, "contraction": contraction / args.steps,
                                                 "reduction": red / args.steps},
                          "launch_groups_per_step": groups / args.steps,
                          "expected_synonymous": float(outs["weighted_change"][:, 1].sum().item() / outs["weight_stats"][1].item()),
                          "expected_replacement": float(outs["weighted_change"][:, 2].sum().item() / outs["weight_stats"][1].item())}
    # K9 alone on the same rows
    k9_outs = capi._CodonOutputsDevice(loglik=outs["loglik"].data_ptr(),
                                       weighted_windows=torch.empty((max(nw, 1), 125), dtype=torch.float64, device=dev).data_ptr(),
                                       weighted_genes=torch.empty(max(ng, 1), dtype=torch.float64, device=dev).data_ptr())
    timed(lambda: lib.check(lib.lib.lh_eval_codons_batch_device(fam, n, T, depth, *tree_ptrs, R, C.byref(k9_outs),
                                                                C.c_void_p(stream))))
    k9_ms = lib.codon_profile_read(fam)[0] / args.steps
    # the forward sweep of a plain evaluation of the same rows
    eo = capi._EvalOutputs()
    timed(lambda: lib.check(lib.lib.lh_eval_batch_device(fam, n, T, depth, *tree_ptrs, R, outs["loglik"].data_ptr(),
                                                         C.byref(eo), C.c_void_p(stream))))
    ms = [C.c_double() for _ in range(3)]
    launches = C.c_int64()
    lib.check(lib.lib.lh_profile_read(fam, C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2]), C.byref(launches)))
    lib.check(lib.lib.lh_family_status(fam))

    # parity outside the timed loop: row 0, both nodes
    from tests import ancestral_probs_oracle as apo
    from tests import codon_oracle as co
    from tests import node_codon_oracle as nco
    worst = 0.0
    r = rows[0]
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
    o.initialize_phylo_emission()
    o.log_likelihood()
    Q = co.dense(o, args.frame)[0]
    children, root, brlen = trees[0]
    for node in (capi.NODE_PARENT, capi.NODE_MRCA):
        res = lib.eval_node_codons_batch(fam, T, depth, ops_a[:1], brl_a[:1], er_a[:1], pi_a[:1], alpha_a[:1], R, [paths[0]],
                                         node, want=("codons", "change"))
        G = apo.cond_tables(children, root, brlen, T, o.msa, r["er"], np.asarray(r["pi"]), orc.gamma_rates_mean(r["alpha"], R),
                            paths[0], node)
        worst = max(worst, float(np.abs(res["codons"][0] - nco.contraction(Q, G, args.frame)).max()),
                    float(np.abs(res["change"][0] - nco.change(Q, G, args.frame)).max()))
    if not worst < 1e-8:
        raise SystemExit("parity failure: the node's codon tables differ from the oracle by %.3g" % worst)
    st = outs["weight_stats"].cpu().numpy()
    out = {"metric": "exact node-codon table rows/sec at the MRCA (K0-K2 + K9 + K13 tables + K14 + weighted reduction)",
           "value": per_node["mrca"]["rows_per_s"], "unit": "rows/s",
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "n_sites": L, "n_codons": nc, "n_window": nw,
                      "frame": args.frame, "path_len": P, "mean_chain": float(np.mean([len(p) for p in paths])),
                      "seed_tip": args.seed_tip, "steps": args.steps},
           "parent": per_node["parent"], "mrca": per_node["mrca"],
           "k9_alone_ms_per_step": k9_ms, "forward_K2_ms_per_step": ms[2].value / args.steps,
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"max_abs_err": worst}}
    if args.with_tip:
        out["slot"] = dict(per_node["slot"], with_tip=args.with_tip,
                           slots={"mean": float(np.mean(slots)), "min": int(min(slots)), "max": int(max(slots))})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
