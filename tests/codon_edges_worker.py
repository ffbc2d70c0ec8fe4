"""Helper of tests/test_gpu_codon_edges.py: one case per process.

groups  LH_CODON_EDGES_MB=<n>: one call cut into several launch groups by the memory hook against the same rows alone.
device  the _device form on a stream of torch's (torch first: it brings its own HIP runtime).
bound   LH_EDGE_OUT_MB=1: the refusal that names the largest n."""
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
    from tests.codon_edges_cases import synth
    return synth(hip, pathlib.Path(tmp), **kw)


def groups(tmp):
    import numpy as np
    import linearham_amd
    from linearham_amd import capi
    from tests.codon_edges_cases import TABLES
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=4, seed=33)
    c.set_frame(1)
    n, tip = 11, 3
    pairs_ = [(i % 4, tip) for i in range(n)]
    capi.Family.borrow(c.family, hip).profile_enable(True)
    want = ("loglik",) + TABLES + ("weighted_codon_counts", "weighted_aa_counts", "weighted_seed_change", "weight_stats")
    full, _ = c.codon_edges(pairs_, tip, want=want)
    n_groups = hip.codon_edges_profile_read(c.family)[3]
    bad = []
    for i in range(4):
        alone, paths = c.codon_edges([pairs_[i]], tip)
        k = len(paths[0])  # (the batch's path_len is its longest chain: a row's live slots and its naive edge keep their bits)
        for j in range(i, n, 4):
            for key in ("loglik",) + TABLES:
                a, b = alone[key][0], full[key][j]
                same = np.array_equal(a[:k], b[:k]) and np.array_equal(a[-1], b[-1]) and not b[k:-1].any() \
                    if key in ("edge_change", "edge_load") else np.array_equal(a, b)
                if not same:
                    bad.append((j, key))
    lw = full["loglik"] + 1000.0
    w = np.exp(lw - lw.max())
    sums = all(np.allclose(full["weighted_" + k], np.tensordot(w, full[k], axes=1), rtol=1e-13, atol=1e-300)
               for k in ("codon_counts", "aa_counts", "seed_change"))
    return {"n": n, "groups": n_groups, "mismatches": bad, "weighted_sums": bool(sums),
            "finite": bool(all(np.isfinite(full[k]).all() for k in TABLES))}


def device(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi
    from tests.codon_edges_cases import TABLES
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_leaves=12, n_samples=4, seed=31)
    nc = c.set_frame(0)["n_codons"]
    fam = capi.Family.borrow(c.family, hip)
    n = 4
    rows = list(range(n))
    victim = 1
    tip = [u for u in range(1, c.T) if len(c.path(victim, u)) >= 2][0]
    pairs_ = [(i, tip) for i in rows]
    sums = ("weighted_codon_counts", "weighted_aa_counts", "weighted_seed_change", "weight_stats")
    host, paths = c.codon_edges(pairs_, tip, want=("loglik",) + TABLES + sums)
    P = max(len(p) for p in paths)
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    shapes = {"loglik": (n,), "codon_counts": (n, nc, 4), "aa_counts": (n, nc, 21, 21), "seed_change": (n, nc, 3),
              "edge_change": (n, P + 1, nc, 3), "edge_load": (n, P + 1, 2), "weighted_codon_counts": (nc, 4),
              "weighted_aa_counts": (nc, 21, 21), "weighted_seed_change": (nc, 3), "weight_stats": (3,)}

    def status():
        try:
            fam.status()
        except RuntimeError as e:
            return str(e)
        return ""

    def run(ops_arr, path_arr):
        d = [t(ops_arr, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64),
             t(path_arr, np.int32)]
        outs = {k: torch.full(s, 7.0, dtype=torch.float64, device=dev) for k, s in shapes.items()}  # stale values
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_codon_edges_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                              d[3].data_ptr(), d[4].data_ptr(), R, d[5].data_ptr(), P, tip,
                                              {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
        st = status()
        return {k: v.cpu().numpy() for k, v in outs.items()}, st, status()

    path_arr = capi.pad_paths(paths)
    clean, st0, _ = run(ops, path_arr)
    res = {"clean_status": st0, "clean_equals_host": bool(all(np.array_equal(clean[k], host[k]) for k in host))}
    keep = [i for i in range(n) if i != victim]

    def verdict(ops_arr, path_arr):
        o, st, st2 = run(ops_arr, path_arr)
        lw = o["loglik"][keep]
        w = np.exp(lw - lw.max())
        ok = True
        for k in ("codon_counts", "aa_counts", "seed_change"):
            ref = np.tensordot(w, o[k][keep], axes=1)
            ok = ok and bool(np.allclose(o["weighted_" + k], ref, rtol=1e-13, atol=1e-300))
        return {"status": st, "second_status": st2,
                "victim_all_nan": bool(all(np.isnan(o[k][victim]).all() for k in TABLES)),
                "others_unchanged": bool(all(np.array_equal(o[k][i], clean[k][i]) for i in keep for k in TABLES)),
                "weights_leave_the_victim_out": ok and bool(abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum())}
    swapped = path_arr.copy()
    swapped[victim, 0], swapped[victim, 1] = path_arr[victim, 1], path_arr[victim, 0]
    res["not_a_chain"] = verdict(ops, swapped)
    # the victim's row carries another tip's (valid) path: the seed is not a child of its first node
    stranger = [u for u in range(1, c.T) if c.path(victim, u)[0] != paths[victim][0] and len(c.path(victim, u)) <= P][0]
    foreign = path_arr.copy()
    foreign[victim] = capi.pad_paths([c.path(victim, stranger), [0] * P])[0]
    res["not_a_child"] = verdict(ops, foreign)
    # the host-pointer form refuses both
    for name, arr in (("host_not_a_chain", swapped), ("host_not_a_child", foreign)):
        try:
            hip.eval_codon_edges_batch(c.family, *c.args(rows), arr, tip)
            res[name] = ""
        except RuntimeError as e:
            res[name] = str(e)
    return res


def bound(tmp):
    import numpy as np
    import linearham_amd
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=2, seed=35)
    nc = c.set_frame(0)["n_codons"]
    tip = 1
    P = max(len(c.path(i, tip)) for i in range(2))
    most = (1 << 20) // (8 * (nc * 4 + (P + 1) * 2))
    want = ("codon_counts", "edge_load")
    message = ""
    try:
        c.codon_edges([(i % 2, tip) for i in range(most + 1)], tip, want=want)
    except RuntimeError as e:
        message = str(e)
    ok, _ = c.codon_edges([(i % 2, tip) for i in range(most)], tip, want=want)
    return {"most": most, "message": message, "largest_passes": bool(np.isfinite(ok["codon_counts"]).all())}


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_cedge_")
    try:
        print(json.dumps({"groups": groups, "device": device, "bound": bound}[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
