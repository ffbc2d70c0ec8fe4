"""Helper of tests/test_gpu_eval_overlap.py: one child process per value of LH_EVAL_SPLIT (and of LH_CHUNK), which the
library reads once per process; the device-pointer entry points take torch tensors, whose HIP runtime has to come up first.

    python -m tests.eval_overlap_worker OUT.npz DIR

DIR holds the synthetic family (written by the first child that needs it).  The child runs every scenario of the test
module's docstring with whatever hooks its environment sets and writes every output into OUT.npz; the last line it prints
is JSON: {"failures": [...], "info": {...}} -- what the child can judge by itself (profile counters, the handle loop,
hipGetLastError)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 5, 8, 9)
N_ROWS = 23
GROUP = 256                  # LH_CHUNK's smallest value
N_GROUPS = 2 * GROUP + 5     # two full launch groups and a remainder
R = 4
KEYS = ("loglik", "rates", "xmsa_emission", "forward", "scaler_counts")
VICTIM = 3                   # n = 5, S = 3: sub-batches of rows {0, 1}, {2, 3}, {4}


def hip_runtime():
    """The HIP runtime this process has loaded already (its hipGetLastError is per thread)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, "expected one HIP runtime in the process: %s" % paths
    rt = C.CDLL(paths[0])
    rt.hipGetLastError.restype = C.c_int
    return rt


def main(out_path, d):
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import Family, _EvalOutputs
    from tests import batch_boundaries_worker as bw
    from tests import desc_builder as db
    from tools import synth_family as sf
    hip = linearham_amd.load_library()
    lib = hip.lib
    rt = hip_runtime()
    out_dir = os.path.join(d, "igh")
    if not os.path.exists(os.path.join(out_dir, "trees.tsv")):
        sf.generate(sf.Spec.small(locus="igh", n_samples=N_ROWS, seed=12), out_dir)
    yaml_path, pdir, tsv = (os.path.join(out_dir, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    keep = host.PhyloHMM(yaml_path, 0, pdir, 0)
    fl = keep.flatten_tsv(tsv, N_ROWS)
    fam = Family.borrow(fl["family"], hip)
    fam.n_xmsa = keep.sizes()["n_xmsa"]
    T, depth, L = fl["n_tips"], fl["max_depth"], keep.sizes()["n_sites"]
    NW, NS = lib.lh_sample_words(fam.handle), lib.lh_sample_states(fam.handle)
    chunked = "LH_CHUNK" in os.environ
    res, failures, info = {}, [], {}
    dp = lambda t: C.c_void_p(t.data_ptr())
    f64 = lambda t: C.cast(dp(t), C.POINTER(C.c_double))

    def rows_of(arrays, rows):
        return [np.ascontiguousarray(arrays[k][rows]) for k in ("ops", "brlen", "er", "pi", "alpha")]

    def prepare(f, xs, n_xmsa):
        """Inputs and all four optional outputs of lh_eval_batch_device as torch tensors (on torch's stream: the caller
        waits for the device before it launches)."""
        ts = [torch.from_numpy(a).to(dev) for a in xs]
        n = len(xs[4])
        out = dict(loglik=torch.full((n,), 0.5, dtype=torch.float64, device=dev),
                   rates=torch.zeros((n, R), dtype=torch.float64, device=dev),
                   xmsa_emission=torch.zeros((n, n_xmsa), dtype=torch.float64, device=dev),
                   forward=torch.zeros((n, f.forward_size), dtype=torch.float64, device=dev),
                   scaler_counts=torch.full((n, f.scaler_size), -7, dtype=torch.int32, device=dev))
        return ts, out

    def launch(f, prepared, n_tips, max_depth, stream):
        """Enqueues the call; nothing is waited for."""
        ts, out = prepared
        outs = _EvalOutputs(f64(out["rates"]), f64(out["xmsa_emission"]), f64(out["forward"]),
                            C.cast(dp(out["scaler_counts"]), C.POINTER(C.c_int32)))
        hip.check(lib.lh_eval_batch_device(f.handle, len(out["loglik"]), n_tips, max_depth, *[dp(t) for t in ts], R,
                                           dp(out["loglik"]), C.byref(outs), C.c_void_p(stream)))
        return out

    def enqueue(f, xs, n_tips, max_depth, n_xmsa, stream):
        prepared = prepare(f, xs, n_xmsa)
        torch.cuda.synchronize()
        return launch(f, prepared, n_tips, max_depth, stream), prepared

    def put(prefix, out):
        for k in KEYS:
            res[prefix + k] = out[k].cpu().numpy() if hasattr(out[k], "cpu") else out[k]

    def eval_device(rows, stream):
        out, _ts = enqueue(fam, rows_of(fl, rows), T, depth, fam.n_xmsa, stream)
        torch.cuda.synchronize()
        return out

    current = torch.cuda.current_stream().cuda_stream
    if chunked:
        # launch-group edge: two full groups and a remainder, every group in sub-batches of its own
        rows = (np.arange(N_GROUPS) * 7 + np.arange(N_GROUPS) // GROUP) % N_ROWS
        fam.profile_enable(True)
        put("groups_", eval_device(rows, current))
        ms = fam.profile_read()
        info["groups profile"] = ms
        if ms["launch_groups"] != 3:
            failures.append("%d rows in launch groups of %d: lh_profile_read counts %d launch groups"
                            % (N_GROUPS, GROUP, ms["launch_groups"]))
        fam.profile_enable(False)
    else:
        # 1. sizes and outputs, device and host pointers, with profiling on: one launch group per call, times > 0
        fam.profile_enable(True)
        groups = 1
        for n in SIZES:
            rows = np.arange(n)
            put("dev_n%d_" % n, eval_device(rows, current))
            ms = fam.profile_read()
            if ms["launch_groups"] != groups or not all(ms[k] > 0 for k in ("model_ms", "prune_ms", "forward_ms")):
                failures.append("lh_eval_batch_device n=%d: profile %s" % (n, ms))
            ll, out = fam.eval_batch(T, depth, *rows_of(fl, rows), R, want=KEYS[1:])
            put("host_n%d_" % n, dict(out, loglik=ll))
            ms = fam.profile_read()
            if ms["launch_groups"] != groups or not all(ms[k] > 0 for k in ("model_ms", "prune_ms", "forward_ms")):
                failures.append("lh_eval_batch n=%d: profile %s" % (n, ms))
        fam.profile_enable(False)
        # 2. the toy family of tests/golden
        o, toy, _sets, inp, _cands = bw.toy_family()
        for n in (3, 5):
            xs = [np.ascontiguousarray(inp[k][:n]) for k in ("ops", "brl", "er", "pi", "alpha")]
            out, _ts = enqueue(toy, xs, inp["T"], inp["depth"], toy.n_xmsa, current)
            torch.cuda.synchronize()
            put("toy_n%d_" % n, out)
        toy.close()
        # 3. the legacy default stream and a stream of torch's that is not its default
        side = torch.cuda.Stream(device=dev)
        put("null_", eval_device(np.arange(9), 0))
        put("side_", eval_device(np.arange(9), side.cuda_stream))
        # 4. three calls back to back with different inputs and nothing waited for in between, then one by one
        calls = [np.arange(0, 9), np.arange(9, 14), np.arange(14, 23)]
        for name, stream in (("null", 0), ("side", side.cuda_stream)):
            prepared = [prepare(fam, rows_of(fl, rows), fam.n_xmsa) for rows in calls]
            torch.cuda.synchronize()
            for pr in prepared:
                launch(fam, pr, T, depth, stream)
            torch.cuda.synchronize()
            for i, (_ts, out) in enumerate(prepared):
                put("b2b_%s_%d_" % (name, i), out)
        for i, rows in enumerate(calls):
            put("one_%d_" % i, eval_device(rows, side.cuda_stream))
        # 5. K4 and K3 behind an evaluation
        n = 5
        rng = np.random.default_rng(3)
        ts = [torch.from_numpy(a).to(dev) for a in rows_of(fl, np.arange(n))]
        words = torch.from_numpy(rng.integers(0, 2 ** 32, size=(n, NW), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
        ll = torch.zeros(n, dtype=torch.float64, device=dev)
        rates = torch.zeros((n, R), dtype=torch.float64, device=dev)
        st = torch.full((n, NS), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        hip.check(lib.lh_eval_sample_batch_device(fam.handle, n, T, depth, *[dp(t) for t in ts], R, dp(words), dp(ll),
                                                  dp(rates), dp(st), C.c_void_p(side.cuda_stream)))
        torch.cuda.synchronize()
        res["sample_loglik"], res["sample_rates"], res["sample_states"] = ll.cpu().numpy(), rates.cpu().numpy(), st.cpu().numpy()
        naive = torch.from_numpy(rng.integers(0, 4, size=(n, L)).astype(np.uint8)).to(dev)
        asr_rates = torch.from_numpy(np.ascontiguousarray(np.tile([0.3, 0.7, 1.2, 1.8], (n, 1)))).to(dev)
        anc = torch.full((n, T - 2, L), 9, dtype=torch.uint8, device=dev)
        choice = torch.full((n, L), 9, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        hip.check(lib.lh_asr_batch_device(fam.handle, n, T, depth, *[dp(t) for t in ts[:4]], dp(asr_rates), R, dp(naive), 17,
                                          3, dp(anc), dp(choice), C.c_void_p(side.cuda_stream)))
        torch.cuda.synchronize()
        fam.status()
        res["asr_anc"], res["asr_rate_choice"] = anc.cpu().numpy(), choice.cpu().numpy()
        # 6. a malformed device schedule in the second sub-batch (tests/device_schedule_worker.py's "tip")
        xs = rows_of(fl, np.arange(n))
        ops = xs[0].reshape(n, -1, 4)
        k_tip = next(k for k in range(ops.shape[1]) if (ops[VICTIM, k, 0] & 15) == 1)
        ops[VICTIM, k_tip, 1] = 1 << 20
        out, _ts = enqueue(fam, xs, T, depth, fam.n_xmsa, current)
        status = []
        for _ in range(2):           # the error state is reported once
            try:
                fam.status()
                status.append("")
            except RuntimeError as e:
                status.append(str(e))
        put("bad_", out)
        res["bad_status"] = np.array(status)
        put("after_bad_", eval_device(np.arange(n), current))
        # 7. twenty handles, one evaluation each
        desc = db.build_family_desc(o)
        xs = [np.ascontiguousarray(inp[k][:5]) for k in ("ops", "brl", "er", "pi", "alpha")]
        lls = []
        for _ in range(20):
            f = linearham_amd.Family(desc, hip)
            out, _ts = enqueue(f, xs, inp["T"], inp["depth"], f.n_xmsa, current)
            torch.cuda.synchronize()
            f.status()
            lls.append(out["loglik"].cpu().numpy())
            f.close()
        res["handles_loglik"] = np.stack(lls)
        rc = rt.hipGetLastError()
        if rc != 0:
            failures.append("hipGetLastError after twenty handles: %d" % rc)
    info["k1_form"], info["k2_form"] = fam.k1_form(), fam.k2_form()
    fam.close()
    keep.close()
    np.savez(out_path, **res)
    print(json.dumps({"failures": failures, "info": info}))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv[1], sys.argv[2])
