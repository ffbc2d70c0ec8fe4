#!/usr/bin/env python3
"""Throughput of exact codon marginals of the naive sequence (K0-K2 + K9, lh_eval_codons_batch_device) on the
configs[2] family, inputs resident in HBM.  Not the headline metric (bench.py is); prints one JSON line.

  python bench_codons.py [--batch 49152] [--steps 5] [--warmup 1] [--preset config2|small] [--frame 0]

Each step evaluates `batch` distinct tree samples and reduces their window codons and gene posteriors to importance-
weighted sums on the device.  A few rows are checked against tests/codon_oracle.py (the three-position smoothing formula on
the numpy oracle's forward arrays), outside the timed loop."""
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
    ap.add_argument("--frame", type=int, default=0, choices=[0, 1, 2])
    ap.add_argument("--check", type=int, default=2, help="rows checked against the oracle")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    import torch
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import _CodonOutputsDevice
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
    lay = lib.set_codons(fam, args.frame)
    NW, NG = len(lay["window_codon"]), lay["n_genes"]
    win = torch.empty((n, NW, 125), dtype=torch.float64, device=dev)
    gen = torch.empty((n, NG), dtype=torch.float64, device=dev)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    wwin = torch.empty((NW, 125), dtype=torch.float64, device=dev)
    wgen = torch.empty(NG, dtype=torch.float64, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    outs = _CodonOutputsDevice(*[t.data_ptr() for t in (d_rb, ll, win, gen, wwin, wgen, stats)])

    def step():
        lib.check(lib.lib.lh_eval_codons_batch_device(fam, n, T, depth, d["ops"].data_ptr(), d["brlen"].data_ptr(),
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
    k9_ms, k9_n = lib.codon_profile_read(fam)
    lib.check(lib.lib.lh_profile_enable(fam, 0))
    lib.check(lib.lib.lh_family_status(fam))
    split = {"model": ms[0].value / args.steps, "prune": ms[1].value / args.steps, "forward": ms[2].value / args.steps,
             "K9": k9_ms / max(k9_n, 1)}
    # parity outside the timed loop: rows against the codon oracle's dense form
    from oracle import linearham_oracle as orc
    from tests import codon_oracle as co
    w, g = win[:args.check].cpu().numpy(), gen[:args.check].cpu().numpy()
    worst = 0.0
    o = orc.PhyloHMM(os.path.join(fam_dir, "cluster.yaml"), 0, os.path.join(fam_dir, "hmm_params"), 0)
    for i in range(args.check):
        r = rows[i % len(rows)]
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], R, is_path=False)
        o.initialize_phylo_emission()
        o.log_likelihood()
        table, post = co.dense(o, args.frame)
        ow, og, olay = co.window_inputs(o, table, post, args.frame)
        if olay["window_codon"] != lay["window_codon"]:
            raise SystemExit("parity failure: the window codons differ from the oracle's")
        worst = max(worst, float(np.max(np.abs(w[i] - ow))), float(np.max(np.abs(g[i] - og))))
    if not worst < 1e-9:
        raise SystemExit("parity failure: codon windows differ from the oracle by %.3g" % worst)
    st = stats.cpu().numpy()
    out = {"metric": "exact codon-marginal rows/sec (K0-K2 + K9 smoothing + weighted reduction)",
           "value": n * args.steps / dt, "unit": "tree samples/s", "ms_per_step": dt / args.steps * 1e3,
           "config": {"workload": args.preset, "batch": n, "n_tips": T, "R": R, "forward_size": FS, "frame": args.frame,
                      "n_window": NW, "n_codons": lay["n_codons"], "n_genes": NG},
           "kernel_ms_per_step": split, "k9_share": split["K9"] / (dt / args.steps * 1e3),
           "bytes_per_sample": {"read_forward": 8 * FS, "written": 8 * (NW * 125 + NG)},
           "kish_ess": float(st[1] * st[1] / st[2]) if st[2] > 0 else 0.0,
           "parity": {"rows": args.check, "max_abs_err": worst}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
