"""Helper of tests/test_gpu_node_codons.py: one case per process.

chunk   LH_CHUNK=256: one call over n = 259 rows against the same rows alone.
device  the _device form on a stream of torch's (torch first: it brings its own HIP runtime).
bound   LH_ANC_OUT_MB=1: the refusal that names the largest n."""
import json
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _case(hip, tmp, **kw):
    import pathlib
    from tests.node_codons_cases import synth
    return synth(hip, pathlib.Path(tmp), **kw)


def chunk(tmp):
    import numpy as np
    import linearham_amd
    from linearham_amd import capi
    from tests.node_codons_cases import PARENT
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=4, seed=33)
    c.set_frame(1)
    n = 259
    pairs_ = [(i % 4, 1 + (i * 5) % (c.T - 1)) for i in range(n)]
    capi.Family.borrow(c.family, hip).profile_enable(True)
    full, _ = c.node_codons(pairs_, PARENT)
    groups = hip.node_codons_profile_read(c.family)[3]
    checked, bad = [0, 255, 256, 258], []
    for i in checked:
        alone, _ = c.node_codons([pairs_[i]], PARENT)
        for key in ("loglik", "codons", "change"):
            if not np.array_equal(alone[key][0], full[key][i]):
                bad.append((i, key))
    return {"n": n, "groups": groups, "rows_checked": checked, "mismatches": bad,
            "finite": bool(np.isfinite(full["codons"]).all() and np.isfinite(full["change"]).all())}


def device(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi
    from tests.node_codons_cases import PARENT
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_leaves=12, n_samples=4, seed=31)
    nc = c.set_frame(0)["n_codons"]
    fam = capi.Family.borrow(c.family, hip)
    n = 4
    pairs_ = [(i, 1 + 2 * i) for i in range(n)]
    rows = [p[0] for p in pairs_]
    members = ("loglik", "codons", "change", "weighted_codons", "weighted_change", "weight_stats")
    host, paths = c.node_codons(pairs_, PARENT, want=members)
    P = max(len(p) for p in paths)
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)

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
                "codons": torch.full((n, nc, 64), 7.0, dtype=torch.float64, device=dev),   # stale values that must not survive
                "change": torch.full((n, nc, 4), 7.0, dtype=torch.float64, device=dev),
                "weighted_codons": torch.zeros((nc, 64), dtype=torch.float64, device=dev),
                "weighted_change": torch.zeros((nc, 4), dtype=torch.float64, device=dev),
                "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_node_codons_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
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
        ok = True
        for k in ("codons", "change"):
            ref = np.tensordot(w, o[k][keep], axes=1)
            ok = ok and bool(np.allclose(o["weighted_" + k], ref, rtol=1e-13, atol=1e-300))
        return {"status": st, "second_status": st2,
                "victim_all_nan": bool(np.isnan(o["codons"][victim]).all() and np.isnan(o["change"][victim]).all()),
                "others_unchanged": bool(all(np.array_equal(o[k][i], clean[k][i]) for i in keep for k in ("codons", "change"))),
                "weights_leave_the_victim_out": ok and bool(abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum())}
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
    from tests.node_codons_cases import MRCA
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=2, seed=35)
    nc = c.set_frame(0)["n_codons"]
    most = (1 << 20) // (8 * nc * 68)
    message = ""
    try:
        c.node_codons([(i % 2, 1) for i in range(most + 1)], MRCA, want=("codons", "change"))
    except RuntimeError as e:
        message = str(e)
    ok, _ = c.node_codons([(i % 2, 1) for i in range(most)], MRCA, want=("codons", "change"))
    return {"most": most, "message": message, "largest_passes": bool(np.isfinite(ok["codons"]).all())}


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_nodec_")
    try:
        print(json.dumps({"chunk": chunk, "device": device, "bound": bound}[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
