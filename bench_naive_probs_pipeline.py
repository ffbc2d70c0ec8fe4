#!/usr/bin/env python3
"""The two passes of RunNaiveProbsPipeline on the configs[2] family (synthetic 100 leaves x 400 sites, full V/D/J
germline set), and K6c against the host way of collecting draws; not the headline metric (bench.py is).  Prints one JSON
line.

  python bench_naive_probs_pipeline.py [--batch 49152] [--steps 3] [--warmup 1] [--preset config2|small]

pipeline: `linearham --naive-probs-pipeline` on the family's table (one batch of `batch` rows), timed by the pipeline
          itself (LH_PIPELINE_TIMING: table parsing, device calls, host collection, per pass); rows/s of each pass
          with and without the table parsing;
K6c:      its own time per batch from HIP events (lh_collect_profile_read), over lh_eval_draw_batch calls;
host way: lh_eval_sample_batch (states to the host) + HMM::ApplySampledStates + a map of the strings (C++)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=49152)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--preset", default="config2", choices=["config2", "small"])
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    import numpy as np
    from linearham_amd import host
    from linearham_amd.capi import load_library
    from tools import synth_family as sf
    n = args.batch
    spec = {"config2": sf.Spec(n_samples=n), "small": sf.Spec.small(n_samples=min(n, 512))}[args.preset]
    n = spec.n_samples
    fam_dir = os.path.join(tempfile.gettempdir(), "lh_bench_naive_pipeline_%s_%d" % (args.preset, n))
    if not os.path.exists(os.path.join(fam_dir, "meta.json")):
        sf.generate(spec, fam_dir)
    tsv = os.path.join(fam_dir, "trees.tsv")
    yaml_path, pdir = os.path.join(fam_dir, "cluster.yaml"), os.path.join(fam_dir, "hmm_params")
    rb = np.array([r["likelihood"] for r in sf.read_trees_tsv(tsv)])[:n]
    R = 4
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = h.flatten_tsv(tsv, n)
    hip = load_library()
    fam = C.c_void_p(fl["family"])
    W = hip.lib.lh_sample_words(fam)
    S = hip.lib.lh_sample_states(fam)
    words = np.random.default_rng(0).integers(0, 2 ** 32, (n, W), dtype=np.uint64).astype(np.uint32)
    a = (fam, fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"], fl["er"], fl["pi"], fl["alpha"], R)

    def pass1():
        hip.draws_reset(fam)
        ll, hsh, _ = hip.eval_draw_batch(*a, words)
        ids, cand = {}, np.empty(n, dtype=np.int32)
        for i, x in enumerate(hsh.tolist()):
            cand[i] = ids.setdefault(x, len(ids)) if np.isfinite(ll[i] - rb[i]) else -1
        mism = hip.draws_resolve(fam, cand)
        assert len(mism) == 0
        return len(ids)

    states = np.zeros((n, S), dtype=np.int32)
    ll = np.zeros(n)
    c_i32p, c_f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    hip.lib.lh_eval_sample_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_f64p, c_f64p, c_f64p,
                                             c_f64p, C.c_int32, C.POINTER(C.c_uint32), c_f64p, c_f64p, c_i32p]
    lib_h = host.load_host()
    lib_h.lhh_phylo_apply_states_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_double)]

    def host_way():
        t0 = time.perf_counter()
        p = lambda x, t: np.ascontiguousarray(x).ctypes.data_as(t)  # noqa: E731
        hip.check(hip.lib.lh_eval_sample_batch(fam, n, fl["n_tips"], fl["max_depth"], p(fl["ops"], c_i32p),
                                               p(fl["brlen"], c_f64p), p(fl["er"], c_f64p), p(fl["pi"], c_f64p),
                                               p(fl["alpha"], c_f64p), R, words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               ll.ctypes.data_as(c_f64p), None, states.ctypes.data_as(c_i32p)))
        t1 = time.perf_counter()
        nd, sec = C.c_int(), C.c_double()
        host._check(lib_h.lhh_phylo_apply_states_map(h.h, n, states.ctypes.data, C.byref(nd), C.byref(sec)))
        return t1 - t0, sec.value, nd.value

    for _ in range(args.warmup):
        pass1()
        host_way()
    hip.lib.lh_profile_enable(fam, 1)
    hip.collect_profile_read(fam)
    for _ in range(args.steps):
        distinct = pass1()
    k6c_ms, k6c_launches = hip.collect_profile_read(fam)
    hip.lib.lh_profile_enable(fam, 0)
    hw = [host_way() for _ in range(args.steps)]
    t_states = sum(x[0] for x in hw) / args.steps
    t_apply = sum(x[1] for x in hw) / args.steps
    assert hw[0][2] == distinct, (hw[0][2], distinct)
    # the pipeline itself, in a process of its own (its stage times are read once per process)
    exe = os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    out_dir = tempfile.mkdtemp(prefix="lh_bench_np_")
    env = dict(os.environ, LH_PIPELINE_TIMING="1")
    pat = re.compile(r"\[RunNaiveProbsPipeline\] (\d+) rows; pass 1 \(([^)]*)\): parse ([\d.]+) s, device ([\d.]+) s, "
                     r"collect ([\d.]+) s, total ([\d.]+) s; pass 2 \((\d+) candidates\): priors ([\d.]+) s, "
                     r"parse ([\d.]+) s, device ([\d.]+) s, total ([\d.]+) s")
    runs = []
    for k in range(args.warmup + args.steps):
        r = subprocess.run([exe, "--naive-probs-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0",
                            "--hmm-param-dir", pdir, "--input-path", tsv, "--output-path", os.path.join(out_dir, "np"),
                            "--num-rates", str(R)], capture_output=True, text=True, env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stderr)
        m = pat.search(r.stderr)
        if m is None:
            raise SystemExit("no stage times in the pipeline's output:\n" + r.stderr)
        if k >= args.warmup:
            runs.append([float(x) for x in m.groups()[2:6]] + [int(m.group(7))] + [float(x) for x in m.groups()[7:]])
    avg = [sum(r[i] for r in runs) / len(runs) for i in range(len(runs[0]))]
    p1_parse, p1_dev, p1_collect, p1_total, n_cand, p2_prior, p2_parse, p2_dev, p2_total = avg
    print(json.dumps({
        "metric": "naive_probs_pipeline_rows_per_s", "preset": args.preset, "rows": n, "steps": args.steps,
        "candidates": int(n_cand),
        "pass1_rows_per_s": n / p1_total, "pass1_rows_per_s_without_parsing": n / (p1_total - p1_parse),
        "pass1_s": {"parse": p1_parse, "device": p1_dev, "collect": p1_collect, "total": p1_total},
        "pass2_rows_per_s": n / p2_total, "pass2_rows_per_s_without_parsing": n / (p2_total - p2_parse),
        "pass2_s": {"priors": p2_prior, "parse": p2_parse, "device": p2_dev, "total": p2_total},
        "k6c_ms_per_batch": k6c_ms / max(k6c_launches, 1), "k6c_launches": k6c_launches,
        "host_way_rows_per_s": n / (t_states + t_apply), "host_way_states_s": t_states, "host_way_apply_map_s": t_apply}))

if __name__ == "__main__":
    main()
