#!/usr/bin/env python3
"""Throughput of the exact probabilities of candidate ancestral sequences (K0-K2 + K5 + K13,
lh_eval_ancestral_candidates_batch_device) on the configs[2] family, inputs resident in HBM, at both nodes (the seed's parent,
the MRCA), beside the forward sweep's time per evaluation (lh_profile_read) and K11b's time on the same rows
(lh_eval_ancestral_batch_device) in the same run.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_ancestral_probs.py [--batch 4096] [--candidates 64] [--steps 3] [--warmup 1] [--preset config2|small]
                                  [--seed-tip 1] [--with-tip <tip>] [--alternations 5] [--out <file>]

--with-tip names a second tip: the run then also times the slot form (lh_eval_ancestral_candidates_at_batch_device) at the
most recent common ancestor of the two tips, a slot of its own per row, and reports the table time of the three forms over
--alternations rounds of parent, MRCA, slot in turn after the warm-up, with the mean and range of the slots.

The candidates are distinct MRCA sequences of the family's own ancestral draws (lh_eval_draw_batch, lh_naive_sequences,
lh_asr_batch).  Each step scores every candidate on `batch` distinct tree samples -- batch x candidates forward sweeps --
and reduces them to the importance-weighted sum on the device.  One row is checked against
tests/ancestral_probs_oracle.py outside the timed loop."""
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
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    ap.add_argument("--seed-tip", type=int, default=1)
    ap.add_argument("--with-tip", type=int, default=0, help="a second tip: also time K13 at its common ancestor with the seed")
    ap.add_argument("--alternations", type=int, default=5, help="rounds of parent, MRCA, slot in turn (with --with-tip)")
    ap.add_argument("--check", type=int, default=2, help="candidates of row 0 checked against the oracle")
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
    n, K = args.batch, args.candidates
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

    # the candidates: distinct MRCA sequences among one ancestral draw of each of the first rows
    borrowed = capi.Family.borrow(fam, lib)
    m = min(n, 2 * K)
    head = (ops_a[:m], brl_a[:m], er_a[:m], pi_a[:m], alpha_a[:m])
    nw = lib.lib.lh_sample_words(fam)
    words = np.random.default_rng(3).integers(0, 2 ** 32, size=(m, nw), dtype=np.uint64).astype(np.uint32)
    _, _, states = lib.eval_draw_batch(fam, T, depth, *head, R, words, want_states=True)
    naive, _ = lib.naive_sequences(fam, states)
    _, ev = borrowed.eval_batch(T, depth, *head, R, want=("rates",))
    anc, _ = borrowed.asr_batch(T, depth, head[0], head[1], head[2], head[3], ev["rates"], naive, 11, 0)
    seen, cands = set(), []
    for i in range(m):
        q = anc[i, paths[i][-1] - T]
        if bytes(q) not in seen and len(cands) < K:
            seen.add(bytes(q))
            cands.append(q)
    if len(cands) < K:
        raise SystemExit("only %d distinct MRCA sequences among %d draws" % (len(cands), m))
    cands = np.stack(cands)
    lib.set_ancestral_candidates(fam, cands)

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(ops_a, np.int32), "brlen": t(brl_a, np.float64), "er": t(er_a, np.float64), "pi": t(pi_a, np.float64),
         "alpha": t(alpha_a, np.float64), "path": t(path, np.int32)}
    outs = {"log_offset": t(pick("likelihood"), np.float64),
            "loglik": torch.empty(n, dtype=torch.float64, device=dev),
            "weighted_sum": torch.empty(K, dtype=torch.float64, device=dev),
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
    for name, node in (("parent", capi.NODE_PARENT), ("mrca", capi.NODE_MRCA)):
        dt = timed(lambda: lib.eval_ancestral_candidates_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P,
                                                                      node, out_ptrs, stream))
        tables, pairs, red, groups = lib.ancestral_candidates_profile_read(fam)
        ms_step = dt / args.steps * 1e3
        per_node[name] = {"pairs_per_s": n * K * args.steps / dt, "ms_per_step": ms_step,
                          "kernel_ms_per_step": {"tables": tables / args.steps, "pair emissions + sweeps": pairs / args.steps,
                                                 "reduction": red / args.steps},
                          "ms_per_49152_pairs": pairs / args.steps / (n * K) * 49152,
                          "launch_groups_per_step": groups / args.steps,
                          "weighted_sum_total": float(outs["weighted_sum"].sum().item())}
    # the three forms of the tables in turn: ms[0] of the profile reader, one step per reading
    forms = None
    if args.with_tip:
        d["slot"] = t(slots, np.int32)
        calls = {"parent": lambda: lib.eval_ancestral_candidates_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(),
                                                                             P, capi.NODE_PARENT, out_ptrs, stream),
                 "mrca": lambda: lib.eval_ancestral_candidates_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(),
                                                                           P, capi.NODE_MRCA, out_ptrs, stream),
                 "slot": lambda: lib.eval_ancestral_candidates_at_batch_device(fam, n, T, depth, *tree_ptrs, R,
                                                                              d["path"].data_ptr(), P, d["slot"].data_ptr(),
                                                                              out_ptrs, stream)}
        for step in calls.values():
            for _ in range(max(args.warmup, 1)):
                step()
        torch.cuda.synchronize()
        lib.check(lib.lib.lh_family_status(fam))
        forms = {k: [] for k in calls}
        for _ in range(args.alternations):
            for name, step in calls.items():
                lib.check(lib.lib.lh_profile_enable(fam, 1))
                step()
                torch.cuda.synchronize()
                lib.check(lib.lib.lh_profile_enable(fam, 0))
                forms[name].append(lib.ancestral_candidates_profile_read(fam)[0])
        lens = np.array([len(p) for p in paths])
        forms = {"tables_ms": forms, "with_tip": args.with_tip,
                 "slots": {"mean": float(np.mean(slots)), "min": int(min(slots)), "max": int(max(slots))},
                 "down_steps_mean": {"parent": float(np.mean(lens - 1)), "mrca": 0.0, "slot": float(np.mean(lens - 1 - np.array(slots)))}}
    # the forward sweep of a plain evaluation of the same rows
    eo = capi._EvalOutputs()
    dt = timed(lambda: lib.check(lib.lib.lh_eval_batch_device(fam, n, T, depth, *tree_ptrs, R, outs["loglik"].data_ptr(),
                                                              C.byref(eo), C.c_void_p(stream))))
    ms = [C.c_double() for _ in range(3)]
    launches = C.c_int64()
    lib.check(lib.lib.lh_profile_read(fam, C.byref(ms[0]), C.byref(ms[1]), C.byref(ms[2]), C.byref(launches)))
    forward_ms = ms[2].value / args.steps
    # K11b on the same rows
    k11_outs = {"loglik": outs["loglik"].data_ptr(),
                "weighted_sum": torch.empty((2, L, 4), dtype=torch.float64, device=dev).data_ptr()}
    timed(lambda: lib.eval_ancestral_batch_device(fam, n, T, depth, *tree_ptrs, R, d["path"].data_ptr(), P, k11_outs, stream))
    _, k11b, _, _ = lib.ancestral_profile_read(fam)
    lib.check(lib.lib.lh_family_status(fam))

    # parity outside the timed loop: row 0, the first candidates, both nodes
    from tests import ancestral_probs_oracle as apo
    worst = 0.0
    r = rows[0]
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
    o.initialize_phylo_emission()
    children, root, brlen = trees[0]
    for node in (capi.NODE_PARENT, capi.NODE_MRCA):
        res = lib.eval_ancestral_candidates_batch(fam, T, depth, ops_a[:1], brl_a[:1], er_a[:1], pi_a[:1], alpha_a[:1], R,
                                                  [paths[0]], node, want=("cond", "log_cand"))
        G = apo.cond_tables(children, root, brlen, T, o.msa, r["er"], np.asarray(r["pi"]), orc.gamma_rates_mean(r["alpha"], R),
                            paths[0], node)
        want = apo.log_candidates(o, G, cands[:args.check])
        worst = max(worst, float(np.abs(res["cond"][0] - G).max()),
                    float(np.abs(res["log_cand"][0, :args.check] - want).max()) if args.check else 0.0)
    if not worst < 1e-8:
        raise SystemExit("parity failure: candidate probabilities differ from the oracle by %.3g" % worst)
    st = outs["weight_stats"].cpu().numpy()
    out = {"metric": "exact ancestral-candidate (row, candidate) pairs/sec at the MRCA (K0-K2 + K5 + K13 + weighted reduction)",
           "value": per_node["mrca"]["pairs_per_s"], "unit": "pairs/s",
           "config": {"workload": args.preset, "batch": n, "candidates": K, "n_tips": T, "R": R, "n_sites": L, "path_len": P,
                      "mean_chain": float(np.mean([len(p) for p in paths])), "seed_tip": args.seed_tip, "steps": args.steps},
           "parent": per_node["parent"], "mrca": per_node["mrca"],
           "forward": {"K2_ms_per_step": forward_ms, "K2_ms_per_49152_evaluations": forward_ms / n * 49152},
           "k11b_ms_per_step": k11b / args.steps,
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"candidates": args.check, "max_abs_err": worst}}
    if forms:
        out["forms"] = forms
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
