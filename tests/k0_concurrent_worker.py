"""Helper of tests/test_gpu_k0_concurrent.py: one child process per setting of LH_K0_SERIAL and LH_EVAL_SPLIT, which the
library reads once per process (LH_CHUNK=256 in all of them); the device-pointer entry points take torch tensors, whose HIP
runtime has to come up first.

    python -m tests.k0_concurrent_worker OUT.npz DIR

DIR holds the two synthetic families (written by the first child).  The child runs every scenario of the test module's
docstring with whatever hooks its environment sets and writes every output into OUT.npz; the last line it prints is JSON:
{"failures": [...], "info": {...}}."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 23
GROUP = 256                       # LH_CHUNK's smallest value
SIZES = (1, 3, 130, 2 * GROUP + 5)  # the last one: two full launch groups and a remainder
R = 4
KEYS = ("loglik", "rates", "xmsa_emission", "forward", "scaler_counts")
FAMILIES = {"igh": dict(locus="igh", n_leaves=8, seed=12), "igk": dict(locus="igk", n_leaves=11, seed=5)}  # 9 and 12 tips
VICTIM = 3
N_BAD = 5
CALLS = (np.arange(0, 9), np.arange(9, 14))   # the two calls back to back


def rows_for(n):
    """n rows of the table, neighbours from different trees, a launch group's rows not those of the next"""
    i = np.arange(n)
    return (i * 7 + i // GROUP) % N_ROWS


def main(out_path, d):
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import host
    from linearham_amd.capi import Family, _EvalOutputs
    from tools import synth_family as sf
    hip = linearham_amd.load_library()
    lib = hip.lib
    res, failures, info = {}, [], {}
    dp = lambda t: C.c_void_p(t.data_ptr())
    f64 = lambda t: C.cast(dp(t), C.POINTER(C.c_double))
    stream = torch.cuda.Stream(device=dev).cuda_stream   # not torch's default: the fork and the joins are the only order

    for name, kw in FAMILIES.items():
        out_dir = os.path.join(d, name)
        if not os.path.exists(os.path.join(out_dir, "trees.tsv")):
            sf.generate(sf.Spec.small(n_samples=N_ROWS, **kw), out_dir)
        yaml_path, pdir, tsv = (os.path.join(out_dir, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
        keep = host.PhyloHMM(yaml_path, 0, pdir, 0)
        fl = keep.flatten_tsv(tsv, N_ROWS)
        fam = Family.borrow(fl["family"], hip)
        fam.n_xmsa = keep.sizes()["n_xmsa"]
        T, depth = fl["n_tips"], fl["max_depth"]
        NW, NS = lib.lh_sample_words(fam.handle), lib.lh_sample_states(fam.handle)
        info[name] = {"tips": int(T)}
        ops_rows = np.asarray(fl["ops"]).reshape(N_ROWS, -1)
        info[name]["distinct_schedules"] = len({r.tobytes() for r in ops_rows})

        def xs_of(rows):
            return [np.ascontiguousarray(fl[k][rows]) for k in ("ops", "brlen", "er", "pi", "alpha")]

        def prepare(xs):
            ts = [torch.from_numpy(a).to(dev) for a in xs]
            n = len(xs[4])
            out = dict(loglik=torch.full((n,), 0.5, dtype=torch.float64, device=dev),
                       rates=torch.zeros((n, R), dtype=torch.float64, device=dev),
                       xmsa_emission=torch.zeros((n, fam.n_xmsa), dtype=torch.float64, device=dev),
                       forward=torch.zeros((n, fam.forward_size), dtype=torch.float64, device=dev),
                       scaler_counts=torch.full((n, fam.scaler_size), -7, dtype=torch.int32, device=dev))
            return ts, out

        def launch(prepared):
            """Enqueues the call; nothing is waited for."""
            ts, out = prepared
            outs = _EvalOutputs(f64(out["rates"]), f64(out["xmsa_emission"]), f64(out["forward"]),
                                C.cast(dp(out["scaler_counts"]), C.POINTER(C.c_int32)))
            hip.check(lib.lh_eval_batch_device(fam.handle, len(out["loglik"]), T, depth, *[dp(t) for t in ts], R,
                                               dp(out["loglik"]), C.byref(outs), C.c_void_p(stream)))
            return out

        def eval_device(xs):
            prepared = prepare(xs)
            torch.cuda.synchronize()
            out = launch(prepared)
            torch.cuda.synchronize()
            return out

        def put(prefix, out):
            for k in KEYS:
                res["%s_%s_%s" % (name, prefix, k)] = out[k].cpu().numpy() if hasattr(out[k], "cpu") else out[k]

        # 1. sizes, device and host pointers; profiling on for the device calls: every stage's time above zero
        fam.profile_enable(True)
        for n in SIZES:
            rows = rows_for(n)
            put("dev_n%d" % n, eval_device(xs_of(rows)))
            ms = fam.profile_read()
            groups = (n + GROUP - 1) // GROUP
            if ms["launch_groups"] != groups or not all(ms[k] > 0 for k in ("model_ms", "prune_ms", "forward_ms")):
                failures.append("%s: lh_eval_batch_device n=%d: profile %s" % (name, n, ms))
        fam.profile_enable(False)
        for n in SIZES:
            ll, out = fam.eval_batch(T, depth, *xs_of(rows_for(n)), R, want=KEYS[1:])
            put("host_n%d" % n, dict(out, loglik=ll))
        # 2. K4 behind an evaluation
        n = 130
        rng = np.random.default_rng(3)
        ts = [torch.from_numpy(a).to(dev) for a in xs_of(rows_for(n))]
        words = torch.from_numpy(rng.integers(0, 2 ** 32, size=(n, NW), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
        ll = torch.zeros(n, dtype=torch.float64, device=dev)
        rates = torch.zeros((n, R), dtype=torch.float64, device=dev)
        st = torch.full((n, NS), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        hip.check(lib.lh_eval_sample_batch_device(fam.handle, n, T, depth, *[dp(t) for t in ts], R, dp(words), dp(ll),
                                                  dp(rates), dp(st), C.c_void_p(stream)))
        torch.cuda.synchronize()
        fam.status()
        for k, v in (("loglik", ll), ("rates", rates), ("states", st)):
            res["%s_sample_%s" % (name, k)] = v.cpu().numpy()
        # 3. two calls back to back, nothing waited for in between; then one by one
        prepared = [prepare(xs_of(rows)) for rows in CALLS]
        torch.cuda.synchronize()
        for pr in prepared:
            launch(pr)
        torch.cuda.synchronize()
        for i, (_ts, out) in enumerate(prepared):
            put("b2b_%d" % i, out)
        for i, rows in enumerate(CALLS):
            put("one_%d" % i, eval_device(xs_of(rows)))
        # 4. one corrupted schedule (a tip index far out of range: K0c refuses the sample, K1 leaves it alone)
        xs = xs_of(np.arange(N_BAD))
        put("clean", eval_device(xs))
        ops = xs[0].reshape(N_BAD, -1, 4)
        k_tip = next(k for k in range(ops.shape[1]) if (ops[VICTIM, k, 0] & 15) == 1)
        ops[VICTIM, k_tip, 1] = 1 << 20
        out = eval_device(xs)
        status = []
        for _ in range(2):           # the error state is reported once
            try:
                fam.status()
                status.append("")
            except RuntimeError as e:
                status.append(str(e))
        put("bad", out)
        res[name + "_bad_status"] = np.array(status)
        put("after_bad", eval_device(xs_of(np.arange(N_BAD))))
        info[name]["k1_form"], info[name]["k2_form"] = fam.k1_form(), fam.k2_form()
        fam.close()
        keep.close()
    np.savez(out_path, **res)
    print(json.dumps({"failures": failures, "info": info}))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv[1], sys.argv[2])
