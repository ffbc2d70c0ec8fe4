"""Helper of tests/test_gpu_ancestral.py: one case per process.

chunk   LH_CHUNK is read once per process: one call of lh_eval_ancestral_batch and one of lh_asr_marginals_batch over
        n = 259 rows under LH_CHUNK=256, against the same rows alone.
device  the _device forms on a stream of torch's (torch first: it brings its own HIP runtime).
bound   LH_ANC_OUT_MB (read once per process): the refusal that names the largest n."""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _case(hip, tmp, **kw):
    import pathlib
    from tests.ancestral_cases import EvalCase
    from tools import synth_family as sf
    out = os.path.join(tmp, "fam")
    sf.generate(sf.Spec.small(**kw), out)
    rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    return EvalCase(hip, os.path.join(out, "cluster.yaml"), os.path.join(out, "hmm_params"), rows, 4, pathlib.Path(tmp))


def chunk(tmp):
    import numpy as np
    import linearham_amd
    from linearham_amd import capi
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=4, seed=33)
    n = 259
    pairs = [(i % 4, 1 + (i * 5) % (c.T - 1)) for i in range(n)]
    fam = capi.Family.borrow(c.family, hip)
    fam.profile_enable(True)
    full, paths = c.run(pairs)
    groups_eval = hip.ancestral_profile_read(c.family)[3]
    rows = [p[0] for p in pairs]
    a = c.args(rows)
    _, ev = fam.eval_batch(*a, want=("rates",))
    hip.ancestral_profile_read(c.family)
    m_full, rp_full = fam.asr_marginals_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], full["site_base"],
                                              capi.pad_paths(paths))
    groups_marginals = hip.ancestral_profile_read(c.family)[3]
    fam.profile_enable(False)
    checked, bad = [0, 255, 256, 258], []
    for i in checked:
        alone, path = c.run([pairs[i]])
        k = len(path[0])
        for key in ("loglik", "site_base", "rate_post"):
            if not np.array_equal(alone[key][0], full[key][i]):
                bad.append(("eval", i, key))
        if not np.array_equal(alone["marg"][0, :k], full["marg"][i, :k]):
            bad.append(("eval", i, "marg"))
        b = c.args([rows[i]])
        m1, rp1 = fam.asr_marginals_batch(b[0], b[1], b[2], b[3], b[4], b[5], ev["rates"][i:i + 1], full["site_base"][i:i + 1],
                                          capi.pad_paths(path))
        if not (np.array_equal(m1[0, :k], m_full[i, :k]) and np.array_equal(rp1[0], rp_full[i])):
            bad.append(("marginals", i))
        if not (np.array_equal(m_full[i, :k], full["marg"][i, :k]) and np.array_equal(rp_full[i], full["rate_post"][i])):
            bad.append(("composition", i))
    return {"n": n, "groups_eval": groups_eval, "groups_marginals": groups_marginals, "rows_checked": checked,
            "mismatches": bad}


def device(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_leaves=12, n_samples=4, seed=31)
    fam = capi.Family.borrow(c.family, hip)
    n = 4
    pairs = [(i, 1 + 2 * i) for i in range(n)]
    rows = [p[0] for p in pairs]
    host, paths = c.run(pairs)
    P = max(len(p) for p in paths)
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    _, ev = fam.eval_batch(T, depth, ops, brl, er, pi, alpha, R, want=("rates",))
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    L = c.L

    def status():
        try:
            fam.status()
        except RuntimeError as e:
            return str(e)
        return ""

    def marginals(ops_arr, path_arr):
        d = [t(ops_arr, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(ev["rates"], np.float64),
             t(host["site_base"], np.float64), t(path_arr, np.int32)]
        marg = torch.full((n, P, L, 4), 7.0, dtype=torch.float64, device=dev)      # stale values that must not survive
        rp = torch.full((n, L, R), 7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            fam.asr_marginals_batch_device(n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                           d[4].data_ptr(), R, d[5].data_ptr(), d[6].data_ptr(), P, marg.data_ptr(),
                                           rp.data_ptr(), stream.cuda_stream)
        st = status()
        return marg.cpu().numpy(), rp.cpu().numpy(), st, status()

    path_arr = capi.pad_paths(paths)
    marg0, rp0, st0, _ = marginals(ops, path_arr)
    res = {"clean_status": st0,
           "clean_equals_host": bool(all(np.array_equal(marg0[i, :len(paths[i])], host["marg"][i, :len(paths[i])])
                                         for i in range(n)) and np.array_equal(rp0, host["rate_post"]))}
    victim = 1
    assert len(paths[victim]) >= 2, "the victim's chain has two nodes to swap"

    def verdict(ops_arr, path_arr):
        marg, rp, st, st2 = marginals(ops_arr, path_arr)
        others = all(np.array_equal(marg[i], marg0[i]) and np.array_equal(rp[i], rp0[i]) for i in range(n) if i != victim)
        return {"status": st, "second_status": st2, "victim_all_nan": bool(np.isnan(marg[victim]).all()),
                "others_unchanged": bool(others)}
    bad_ops = ops.copy()
    pops = [k for k in range(bad_ops.shape[1]) if (bad_ops[victim, k, 0] & 15) == 2]
    assert pops, "the victim's tree has a pending sibling"
    bad_ops[victim, pops[0], 3] = 1 if bad_ops[victim, pops[0], 3] == 0 else 0
    res["schedule"] = verdict(bad_ops, path_arr)
    swapped = path_arr.copy()
    swapped[victim, 0], swapped[victim, 1] = path_arr[victim, 1], path_arr[victim, 0]
    res["not_a_chain"] = verdict(ops, swapped)
    short = path_arr.copy()
    k = len(paths[victim])
    short[victim, k - 1] = -1                                                       # the last entry is no longer the root
    res["not_the_root"] = verdict(ops, short)
    # the evaluation form on the same stream: the victim's row NaN, and left out of the weighted sums
    d = [t(ops, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64), t(swapped, np.int32)]
    outs = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev),
            "marg": torch.full((n, P, L, 4), 7.0, dtype=torch.float64, device=dev),
            "weighted_sum": torch.zeros((2, L, 4), dtype=torch.float64, device=dev),
            "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        hip.eval_ancestral_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                        d[3].data_ptr(), d[4].data_ptr(), R, d[5].data_ptr(), P,
                                        {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
    res["eval_status"], res["eval_second_status"] = status(), status()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    res["eval_victim_all_nan"] = bool(np.isnan(o["marg"][victim]).all())
    keep = [i for i in range(n) if i != victim]
    lw = o["loglik"][keep]
    w = np.exp(lw - lw.max())
    ends = np.stack([np.stack([o["marg"][i, 0], o["marg"][i, len(paths[i]) - 1]]) for i in keep])
    ref = np.tensordot(w, ends, axes=1)
    res["eval_weights_leave_the_victim_out"] = bool(
        np.allclose(o["weighted_sum"], ref, rtol=1e-13, atol=1e-300) and o["weight_stats"][0] == lw.max() and
        abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum())
    return res


def bound(tmp):
    """LH_ANC_OUT_MB=1: the host-pointer evaluation form refuses a batch whose device copies of site_base, marg and
    rate_post would exceed 1 MiB, naming the largest n; that n passes."""
    import numpy as np
    import linearham_amd
    hip = linearham_amd.load_library()
    c = _case(hip, tmp, n_samples=2, seed=35)
    tip = 1
    P = max(len(c.path(0, tip)), len(c.path(1, tip)))
    most = (1 << 20) // (8 * c.L * (4 * P + c.R + 5))
    message = ""
    try:
        c.run([(i % 2, tip) for i in range(most + 1)])
    except RuntimeError as e:
        message = str(e)
    ok, _ = c.run([(i % 2, tip) for i in range(most)])
    return {"most": most, "message": message, "largest_passes": bool(np.isfinite(ok["marg"][:, 0]).all())}


if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_anc_")
    try:
        print(json.dumps({"chunk": chunk, "device": device, "bound": bound}[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
