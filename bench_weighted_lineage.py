#!/usr/bin/env python3
"""Rows/s of the weighted lineage pipeline's device work on the configs[2] family: the chain lh_eval_lineage_batch (K0-K2, K4,
K6c, K3 with D ancestral draws per row, K7 behind one pruning launch) against the same work composed from the existing
entry points with their host round trips -- lh_eval_batch for the rates, lh_eval_draw_batch, lh_draws_rows_read, then
lh_lineage_batch once per draw.  Host pointers on both sides, one process, the two alternating after warm-up, at D = 1 and
D = 8.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_weighted_lineage.py [--batch 2048] [--steps 4] [--warmup 1] [--preset config2|small] [--draws 1,8]

Both sides must return the same hashes (checked on the last step); the chain's stage times are HIP events
(lh_lineage_eval_profile_read)."""
import argparse
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
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    ap.add_argument("--draws", default="1,8")
    args = ap.parse_args()
    import numpy as np
    import linearham_amd
    from linearham_amd import capi, host
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    spec = {"config2": sf.Spec(n_samples=256), "small": sf.Spec.small(n_samples=16)}[args.preset]
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_%s_r0" % args.preset)
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    yaml_path, pdir, tsv = (os.path.join(fam_dir, x) for x in ("cluster.yaml", "hmm_params", "trees.tsv"))
    hmm = host.PhyloHMM(yaml_path, 0, pdir, 0)
    n = args.batch
    flat = hmm.flatten_tsv(tsv, n)
    T, depth, R, L = flat["n_tips"], flat["max_depth"], 4, hmm.sizes()["n_sites"]
    lib = linearham_amd.load_library()
    fam = capi.Family.borrow(flat["family"], lib)
    # the paths of the last tip: the table's rows repeat over the batch as flatten_tsv repeats them
    rows = sf.read_trees_tsv(tsv)
    labels = list(orc.PhyloHMM(yaml_path, 0, pdir, 0).xmsa_labels)
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
    NW = lib.lib.lh_sample_words(fam.handle)
    words = np.random.default_rng(1).integers(0, 2 ** 32, size=(n, NW), dtype=np.uint64).astype(np.uint32)
    ev = (T, depth, flat["ops"], flat["brlen"], flat["er"], flat["pi"], flat["alpha"], R)
    all_rows = np.arange(n, dtype=np.int32)

    def chain(seed, D):
        return fam.eval_lineage_batch(*ev, words, seed, path, D)

    def composed(seed, D):
        _, res = fam.eval_batch(*ev, want=("rates",))
        ll, _, _ = lib.eval_draw_batch(fam, *ev, words)
        naive = lib.draws_rows_read(fam, all_rows)
        nt, aa = [], []
        for d in range(D):
            a, b = fam.lineage_batch(T, depth, flat["ops"], flat["brlen"], flat["er"], flat["pi"], res["rates"], naive,
                                     seed, path, d << 32)
            nt.append(a)
            aa.append(b)
        return ll, np.stack(nt, axis=1), np.stack(aa, axis=1)

    results = {}
    for D in [int(x) for x in args.draws.split(",")]:
        for w in range(args.warmup):
            chain(w, D)
            composed(w, D)
        t_chain = t_comp = 0.0
        for s in range(args.steps):
            t0 = time.perf_counter()
            got = chain(100 + s, D)
            t1 = time.perf_counter()
            ll, nt, aa = composed(100 + s, D)
            t2 = time.perf_counter()
            t_chain += t1 - t0
            t_comp += t2 - t1
        # the chain's stage times from one more step, with the event timers on (the timed steps above ran without them)
        fam.profile_enable(True)
        fam.lineage_eval_profile_read()
        chain(100, D)
        ms, groups = fam.lineage_eval_profile_read()
        fam.profile_enable(False)
        if not (np.array_equal(got["nt_hash"], nt) and np.array_equal(got["aa_hash"], aa)):
            raise SystemExit("parity failure: the chain and the composition disagree at D = %d" % D)
        finite = np.isfinite(ll)
        if not np.allclose(got["loglik"][finite], ll[finite], rtol=1e-12, atol=0):
            raise SystemExit("parity failure: log-likelihoods differ at D = %d" % D)
        dev_ms = sum(ms.values())
        results["D%d" % D] = {
            "chain_rows_per_s": n * args.steps / t_chain, "composed_rows_per_s": n * args.steps / t_comp,
            "chain_over_composed": t_comp / t_chain, "chain_ms_per_step": t_chain / args.steps * 1e3,
            "composed_ms_per_step": t_comp / args.steps * 1e3,
            "chain_device_ms_per_step": ms,
            "chain_device_share": {"K1": ms["k1_ms"] / dev_ms, "K3": ms["k3_ms"] / dev_ms, "K7": ms["k7_ms"] / dev_ms},
            "launch_groups_per_step": groups}
    out = {"metric": "weighted lineage rows/sec (chain vs composition, host pointers)",
           "value": results[sorted(results)[0]]["chain_rows_per_s"], "unit": "rows/s",
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "n_sites": L, "R": R, "path_len_max": P,
                      "steps": args.steps, "warmup": args.warmup},
           "draws": results}
    print(json.dumps(out), flush=True)
    fam.close()


if __name__ == "__main__":
    main()
