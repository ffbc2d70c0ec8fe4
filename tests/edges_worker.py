"""Helper of tests/test_gpu_edges.py: one case per process.

chunk   LH_CHUNK is read once per process: one call of lh_eval_edges_batch and one of lh_asr_edges_batch over n = 259 rows
        under LH_CHUNK=256, against the same rows alone.
device  the _device forms on a stream of torch's (torch first: it brings its own HIP runtime).
bound   LH_EDGE_OUT_MB (read once per process): the refusal that names the largest n."""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _case(hip, tmp, **kw):
    import pathlib
    from tests.edges_cases import EdgeEvalCase
    from tools import synth_family as sf
    out = os.path.join(tmp, "fam")
    sf.generate(sf.Spec.small(**kw), out)
    rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    return EdgeEvalCase(hip, os.path.join(out, "cluster.yaml"), os.path.join(out, "hmm_params"), rows, 4, pathlib.Path(tmp))


def _live(res, key, i, k):
    """Row i of an output without its padding slots (k: the row's path length)."""
    import numpy as np
    x = res[key][i]
    if key == "edge":
        return x[:k]
    if key == "edge_load":
        return np.concatenate([x[:k], x[-1:]])
    return x


def chunk(tmp):
    import numpy as np
    import linearham_amd
    from linearham_amd import capi
    from tests.edges_cases import TABLES
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=4, seed=33)
    n, tip = 259, 4
    rows = [i % 4 for i in range(n)]
    fam = capi.Family.borrow(c.family, hip)
    fam.profile_enable(True)
    keys = ("loglik", "site_base", "seed_edge") + TABLES
    full, paths = c.run_edges(rows, tip, want=keys)
    groups_eval = hip.edges_profile_read(c.family)[3]
    a = c.args(rows)
    _, ev = fam.eval_batch(*a, want=("rates",))
    hip.edges_profile_read(c.family)
    e_full = fam.asr_edges_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], full["site_base"], capi.pad_paths(paths), tip)
    groups_edges = hip.edges_profile_read(c.family)[3]
    fam.profile_enable(False)
    checked, bad = [0, 255, 256, 258], []
    for i in checked:
        alone, path = c.run_edges([rows[i]], tip, want=keys)
        k = len(path[0])
        for key in keys:
            if not np.array_equal(_live(alone, key, 0, k), _live(full, key, i, k)):
                bad.append(("eval", i, key))
        b = c.args([rows[i]])
        e1 = fam.asr_edges_batch(b[0], b[1], b[2], b[3], b[4], b[5], ev["rates"][i:i + 1], full["site_base"][i:i + 1],
                                 capi.pad_paths(path), tip)
        for key in TABLES:
            if not np.array_equal(_live(e1, key, 0, k), _live(e_full, key, i, k)):
                bad.append(("edges", i, key))
            if not np.array_equal(_live(e_full, key, i, k), _live(full, key, i, k)):
                bad.append(("composition", i, key))
    return {"n": n, "groups_eval": groups_eval, "groups_edges": groups_edges, "rows_checked": checked, "mismatches": bad}


def device(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi
    from tests.edges_cases import TABLES
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_leaves=12, n_samples=4, seed=31)
    fam = capi.Family.borrow(c.family, hip)
    n = 4
    rows = list(range(n))
    # a seed whose chain has two nodes or more in the victim's tree
    victim = 1
    tip = [t for t in range(1, c.T) if len(c.path(victim, t)) >= 2][0]
    host, paths = c.run_edges(rows, tip)
    P = max(len(p) for p in paths)
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    _, ev = fam.eval_batch(T, depth, ops, brl, er, pi, alpha, R, want=("rates",))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    L = c.L
    shapes = {"edge": (n, P, L, 4, 4), "naive_edge": (n, L, 5, 4), "chain_counts": (n, L, 4, 4), "edge_load": (n, P + 1),
              "rate_post": (n, L, R)}

    def status():
        try:
            fam.status()
        except RuntimeError as e:
            return str(e)
        return ""

    def edges(ops_arr, path_arr, seed):
        d = [t(ops_arr, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(ev["rates"], np.float64),
             t(host["site_base"], np.float64), t(path_arr, np.int32)]
        outs = {k: torch.full(s, 7.0, dtype=torch.float64, device=dev) for k, s in shapes.items()}   # stale values
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            fam.asr_edges_batch_device(n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                       d[4].data_ptr(), R, d[5].data_ptr(), d[6].data_ptr(), P, seed,
                                       {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
        st = status()
        return {k: v.cpu().numpy() for k, v in outs.items()}, st, status()

    path_arr = capi.pad_paths(paths)
    clean, st0, _ = edges(ops, path_arr, tip)
    res = {"clean_status": st0,
           "clean_equals_host": bool(all(np.array_equal(_live(clean, k, i, len(paths[i])), _live(host, k, i, len(paths[i])))
                                         for i in range(n) for k in TABLES))}

    def verdict(ops_arr, path_arr, seed, others_of):
        got, st, st2 = edges(ops_arr, path_arr, seed)
        others = all(np.array_equal(got[k][i], clean[k][i]) for k in TABLES for i in others_of)
        return {"status": st, "second_status": st2,
                "victim_all_nan": bool(all(np.isnan(got[k][victim]).all() for k in TABLES if k != "rate_post")),
                "others_unchanged": bool(others)}
    keep = [i for i in range(n) if i != victim]
    bad_ops = ops.copy()
    pops = [k for k in range(bad_ops.shape[1]) if (bad_ops[victim, k, 0] & 15) == 2]
    assert pops, "the victim's tree has a pending sibling"
    bad_ops[victim, pops[0], 3] = 1 if bad_ops[victim, pops[0], 3] == 0 else 0
    res["schedule"] = verdict(bad_ops, path_arr, tip, keep)
    swapped = path_arr.copy()
    swapped[victim, 0], swapped[victim, 1] = path_arr[victim, 1], path_arr[victim, 0]
    res["not_a_chain"] = verdict(ops, swapped, tip, keep)
    # the victim's row carries another tip's (valid) path: the seed is not a child of its first node
    stranger = [u for u in range(1, c.T) if c.path(victim, u)[0] != paths[victim][0] and len(c.path(victim, u)) <= P][0]
    foreign = path_arr.copy()
    foreign[victim] = capi.pad_paths([c.path(victim, stranger), [0] * P])[0]
    res["not_a_child"] = verdict(ops, foreign, tip, keep)
    # the evaluation form on the same stream: the victim's row NaN, and left out of the weighted sums
    d = [t(ops, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64), t(foreign, np.int32)]
    outs = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev),
            "chain_counts": torch.full((n, L, 4, 4), 7.0, dtype=torch.float64, device=dev),
            "weighted_counts": torch.zeros((L, 4, 4), dtype=torch.float64, device=dev),
            "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        hip.eval_edges_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                    d[4].data_ptr(), R, d[5].data_ptr(), P, tip, {k: v.data_ptr() for k, v in outs.items()},
                                    stream.cuda_stream)
    res["eval_status"], res["eval_second_status"] = status(), status()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    res["eval_victim_all_nan"] = bool(np.isnan(o["chain_counts"][victim]).all())
    lw = o["loglik"][keep]
    w = np.exp(lw - lw.max())
    ref = np.tensordot(w, o["chain_counts"][keep], axes=1)
    res["eval_weights_leave_the_victim_out"] = bool(
        np.allclose(o["weighted_counts"], ref, rtol=1e-13, atol=1e-300) and o["weight_stats"][0] == lw.max() and
        abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum())
    return res


def bound(tmp):
    """LH_EDGE_OUT_MB=1: the host-pointer forms refuse a batch whose device copies of the per-row outputs would exceed
    1 MiB, naming the largest n; that n passes."""
    import numpy as np
    import linearham_amd
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=2, seed=35)
    tip = 1
    P = max(len(c.path(0, tip)), len(c.path(1, tip)))
    want = ("edge", "chain_counts", "edge_load")
    most = (1 << 20) // (8 * (16 * P * c.L + 16 * c.L + P + 1))
    message = ""
    try:
        c.run_edges([i % 2 for i in range(most + 1)], tip, want=want)
    except RuntimeError as e:
        message = str(e)
    ok, _ = c.run_edges([i % 2 for i in range(most)], tip, want=want)
    return {"most": most, "message": message, "largest_passes": bool(np.isfinite(ok["edge"][:, 0]).all())}


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_edges_")
    try:
        print(json.dumps({"chunk": chunk, "device": device, "bound": bound}[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
