"""Helper of tests/test_gpu_ancestral_probs.py: one case per process.

pairs   LH_ANC_PAIRS is read once per process: n = 5 rows and K = 3 candidates under LH_ANC_PAIRS=7, so that a group of
        pairs cuts rows and candidates; printed for the parent to compare with its own run without the hook.
chunk   LH_CHUNK=256: one call over n = 259 rows against the same rows alone.
device  the _device form on a stream of torch's (torch first: it brings its own HIP runtime).
bound   LH_ANC_OUT_MB=1: the refusal that names the largest n."""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS_FAMILY = dict(n_samples=5, seed=45)


def pairs_candidates(L):
    import numpy as np
    from tests import ancestral_probs_oracle as apo
    rng = np.random.default_rng(14)
    cands = rng.integers(0, 4, size=(3, L)).astype(np.uint8)
    cands[1, rng.random(L) < 0.5] = apo.OPEN
    cands[2] = apo.OPEN
    return cands


def _case(hip, tmp, **kw):
    import pathlib
    from tests.ancestral_probs_cases import synth
    return synth(hip, pathlib.Path(tmp), **kw)


def pairs(tmp):
    import linearham_amd
    from tests.ancestral_probs_cases import MRCA
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, **PAIRS_FAMILY)
    res, _ = c.probs([(i, 1 + i) for i in range(5)], MRCA, pairs_candidates(c.L), want=("log_cand", "weighted_sum"))
    return {"log_cand": [[x.hex() for x in row] for row in res["log_cand"].tolist()],
            "weighted_sum": [x.hex() for x in res["weighted_sum"].tolist()]}


def chunk(tmp):
    import numpy as np
    import linearham_amd
    from linearham_amd import capi
    from tests.ancestral_probs_cases import PARENT
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=4, seed=33)
    n = 259
    pairs_ = [(i % 4, 1 + (i * 5) % (c.T - 1)) for i in range(n)]
    capi.Family.borrow(c.family, hip).profile_enable(True)
    full, _ = c.probs(pairs_, PARENT, pairs_candidates(c.L))
    groups = hip.ancestral_candidates_profile_read(c.family)[3]
    checked, bad = [0, 255, 256, 258], []
    for i in checked:
        alone, _ = c.probs([pairs_[i]], PARENT)
        for key in ("loglik", "cond", "log_cand"):
            if not np.array_equal(alone[key][0], full[key][i]):
                bad.append((i, key))
    return {"n": n, "groups": groups, "rows_checked": checked, "mismatches": bad}


def device(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi
    from tests.ancestral_probs_cases import PARENT
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_leaves=12, n_samples=4, seed=31)
    fam = capi.Family.borrow(c.family, hip)
    n = 4
    pairs_ = [(i, 1 + 2 * i) for i in range(n)]
    rows = [p[0] for p in pairs_]
    cands = pairs_candidates(c.L)
    K = len(cands)
    host, paths = c.probs(pairs_, PARENT, cands, want=("loglik", "cond", "log_cand", "weighted_sum", "weight_stats"))
    P = max(len(p) for p in paths)
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    L = c.L

    def status():
        try:
            fam.status()
        except RuntimeError as e:
            return str(e)
        return ""

    def run(ops_arr, path_arr):
        d = [t(ops_arr, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64),
             t(path_arr, np.int32)]
        outs = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev),
                "cond": torch.full((n, L, 5, 4), 7.0, dtype=torch.float64, device=dev),   # stale values that must not survive
                "log_cand": torch.full((n, K), 7.0, dtype=torch.float64, device=dev),
                "weighted_sum": torch.zeros(K, dtype=torch.float64, device=dev),
                "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_ancestral_candidates_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                       d[3].data_ptr(), d[4].data_ptr(), R, d[5].data_ptr(), P, PARENT,
                                                       {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
        st = status()
        return {k: v.cpu().numpy() for k, v in outs.items()}, st, status()

    path_arr = capi.pad_paths(paths)
    clean, st0, _ = run(ops, path_arr)
    res = {"clean_status": st0, "clean_equals_host": bool(all(np.array_equal(clean[k], host[k]) for k in host))}
    victim = 1
    assert len(paths[victim]) >= 2, "the victim's chain has two nodes to swap"
    keep = [i for i in range(n) if i != victim]

    def verdict(ops_arr, path_arr):
        o, st, st2 = run(ops_arr, path_arr)
        lw = o["loglik"][keep]
        w = np.exp(lw - lw.max())
        ref = np.tensordot(w, np.exp(o["log_cand"][keep]), axes=1)
        return {"status": st, "second_status": st2,
                "victim_all_nan": bool(np.isnan(o["cond"][victim]).all() and np.isnan(o["log_cand"][victim]).all()),
                "others_unchanged": bool(all(np.array_equal(o[k][i], clean[k][i]) for i in keep for k in ("cond", "log_cand"))),
                "weights_leave_the_victim_out": bool(np.allclose(o["weighted_sum"], ref, rtol=1e-13, atol=1e-300) and
                                                     abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum())}
    bad_ops = ops.copy()
    pops = [k for k in range(bad_ops.shape[1]) if (bad_ops[victim, k, 0] & 15) == 2]
    assert pops, "the victim's tree has a pending sibling"
    bad_ops[victim, pops[0], 3] = 1 if bad_ops[victim, pops[0], 3] == 0 else 0
    res["schedule"] = verdict(bad_ops, path_arr)
    swapped = path_arr.copy()
    swapped[victim, 0], swapped[victim, 1] = path_arr[victim, 1], path_arr[victim, 0]
    res["not_a_chain"] = verdict(ops, swapped)
    short = path_arr.copy()
    short[victim, len(paths[victim]) - 1] = -1                                      # the last entry is no longer the root
    res["not_the_root"] = verdict(ops, short)
    return res


def bound(tmp):
    import numpy as np
    import linearham_amd
    from tests.ancestral_probs_cases import MRCA
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=2, seed=35)
    cands = pairs_candidates(c.L)
    most = (1 << 20) // (8 * (c.L * 20 + len(cands)))
    message = ""
    try:
        c.probs([(i % 2, 1) for i in range(most + 1)], MRCA, cands, want=("cond", "log_cand"))
    except RuntimeError as e:
        message = str(e)
    ok, _ = c.probs([(i % 2, 1) for i in range(most)], MRCA, want=("cond", "log_cand"))
    return {"most": most, "message": message, "largest_passes": bool(np.isfinite(ok["log_cand"]).all())}


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_ancp_")
    try:
        print(json.dumps({"pairs": pairs, "chunk": chunk, "device": device, "bound": bound}[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
