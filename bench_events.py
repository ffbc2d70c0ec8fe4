#!/usr/bin/env python3
"""Throughput of the exact posteriors of deletion and insertion lengths (K0-K2 + K5 + K10, lh_eval_events_batch_device)
on the configs[2] family, inputs resident in HBM.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_events.py [--batch 49152] [--steps 5] [--warmup 1] [--preset config2|small]

Each step evaluates `batch` distinct tree samples, smooths a copy of their forward arrays (K5), forms the exit, enter and
span tables of every junction (K10) and reduces them and the gene posteriors to importance-weighted sums on the device.
The step's kernels are timed by the handle's profiling events in the same run: K0, K1, K2, K5 (with the copy it smooths)
and K10 (with the reduction).  A few rows are checked against tests/events_oracle.py's dense form outside the timed
loop."""
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
    ap.add_argument("--check", type=int, default=2, help="rows checked against the oracle")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import _EventsOutputsDevice
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    n = args.batch
    spec = {"config2": sf.Spec(n_samples=n), "small": sf.Spec.small(n_samples=min(n, 512))}[args.preset]
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_marginals_%s_%d" % (args.preset, spec.n_samples))
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    tsv = os.path.join(fam_dir, "trees.tsv")
    hmm = host.PhyloHMM(os.path.join(fam_dir, "cluster.yaml"), 0, os.path.join(fam_dir, "hmm_params"), 0)
    flat = hmm.flatten_tsv(tsv, n)
    T, depth, R = flat["n_tips"], flat["max_depth"], 4
    lib = linearham_amd.load_library()
    fam = C.c_void_p(flat["family"])
    FS = lib.lib.lh_forward_size(fam)
    rows = sf.read_trees_tsv(tsv)
    rb = np.array([rows[i % len(rows)]["likelihood"] for i in range(n)])
    d = {k: torch.from_numpy(np.ascontiguousarray(flat[k])).to(dev) for k in ("ops", "brlen", "er", "pi", "alpha")}
    d_rb = torch.from_numpy(rb).to(dev)
    lay = lib.events_layout(fam)
    NE, NG = lay["size"], lay["n_genes"]
    win = torch.empty((n, NE), dtype=torch.float64, device=dev)
    gen = torch.empty((n, NG), dtype=torch.float64, device=dev)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    wwin = torch.empty(NE, dtype=torch.float64, device=dev)
    wgen = torch.empty(NG, dtype=torch.float64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    outs = _EventsOutputsDevice(*[t.data_ptr() for t in (d_rb, ll, win, gen, wwin, wgen, stats)])

    def step():
        lib.check(lib.lib.lh_eval_events_batch_device(fam, n, T, depth, d["ops"].data_ptr(), d["brlen"].data_ptr(),
                                                      d["er"].data_ptr(), d["pi"].data_ptr(), d["alpha"].data_ptr(), R,
                                                      C.byref(outs), C.c_void_p(stream)))
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
    k5_ms, k10_ms, k10_n = lib.events_profile_read(fam)
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_family_status(fam))
    split = {"model": ms[0].value / args.steps, "prune": ms[1].value / args.steps, "forward": ms[2].value / args.steps,
             "K5_on_a_copy": k5_ms / max(k10_n, 1), "K10": k10_ms / max(k10_n, 1)}
    # parity outside the timed loop: rows against the events oracle's dense form
    from oracle import linearham_oracle as orc
    from tests import events_oracle as eo
    from tests import posterior_oracle as po
    w, g = win[:args.check].cpu().numpy(), gen[:args.check].cpu().numpy()
    worst = 0.0
    o = orc.PhyloHMM(os.path.join(fam_dir, "cluster.yaml"), 0, os.path.join(fam_dir, "hmm_params"), 0)
    for i in range(args.check):
        r = rows[i % len(rows)]
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        post = po.smoothing(o)
        ow = eo.flat(eo.dense(o, post))
        og = np.concatenate([post[k] for k in ("vgerm", "dgerm", "jgerm") if k in post])
        if ow.shape != w[i].shape:
            raise SystemExit("parity failure: the events layout differs from the oracle's")
        worst = max(worst, float(np.max(np.abs(w[i] - ow))), float(np.max(np.abs(g[i] - og))))
    if not worst < 1e-9:
        raise SystemExit("parity failure: event tables differ from the oracle by %.3g" % worst)
    st = stats.cpu().numpy()
    out = {"metric": "exact deletion / insertion posterior rows/sec (K0-K2 + K5 + K10 + weighted reduction)",
           "value": n * args.steps / dt, "unit": "tree samples/s", "ms_per_step": dt / args.steps * 1e3,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "forward_size": FS, "events_size": NE,
                      "n_genes": NG, "junctions": lay["junctions"]},
           "kernel_ms_per_step": split, "k10_share": split["K10"] / (dt / args.steps * 1e3),
           "k10_over_k5": split["K10"] / split["K5_on_a_copy"] if split["K5_on_a_copy"] > 0 else None,
           "bytes_per_sample": {"read_forward_and_posterior": 16 * FS, "written": 8 * (NE + NG)},
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"rows": args.check, "max_abs_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
