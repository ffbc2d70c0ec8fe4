"""Helper of tests/test_gpu_weighted_lineage.py::test_device_entry_point_and_a_rejected_schedule (its own process: torch
first).  lh_eval_lineage_batch_device on torch tensors and a stream against the host-pointer form, then the same call on a
schedule K0c rejects -- the validated-input path tests/test_device_schedules.py exercises: no fault is provoked."""
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    import linearham_amd
    from linearham_amd import capi, host
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tools import synth_family as sf
    hip = linearham_amd.load_library()
    out = tempfile.mkdtemp(prefix="lh_wlindev_")
    try:
        sf.generate(sf.Spec.small(n_leaves=12, n_samples=5, seed=31), out)
        yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
        o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
        rows = sf.read_trees_tsv(tsv)
        h = host.PhyloHMM(yaml_path, 0, pdir, 0)
        fam = capi.Family.borrow(h.flatten_tsv(tsv, 1)["family"], hip)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    T, L, R, D = o.msa.shape[0] + 1, o.msa.shape[1], 4, 3
    ops, brl, chains, depth = [], [], [], 0
    for r in rows:
        children, root, brlen = db.tree_arrays(orc.parse_newick(r["tree"]), o.xmsa_labels)
        op, d = hip.schedule_tree(T, children, root)
        ops.append(np.asarray(op, dtype=np.int32).reshape(-1, 4)), brl.append(brlen)
        depth = max(depth, d)
        children = np.asarray(children).ravel()
        parent = {}
        for v in range(T, 2 * T - 2):
            parent[int(children[2 * (v - T)])] = parent[int(children[2 * (v - T) + 1])] = v
        c = [parent[T - 1]]
        while c[-1] != root:
            c.append(parent[c[-1]])
        chains.append(c)
    ops, brl = np.stack(ops), np.stack(brl)
    n = len(rows)
    P = max(len(c) for c in chains)
    path = np.full((n, P), -1, dtype=np.int32)
    for i, c in enumerate(chains):
        path[i, :len(c)] = c
    er, pi = np.array([r["er"] for r in rows]), np.array([r["pi"] for r in rows])
    alpha = np.array([r["alpha"] for r in rows])
    NW, NS = hip.lib.lh_sample_words(fam.handle), hip.lib.lh_sample_states(fam.handle)
    words = np.random.default_rng(4).integers(0, 2 ** 32, size=(n, NW), dtype=np.uint64).astype(np.uint32)
    seed, first = 9, 2
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    def run(ops_arr):
        d_in = [t(ops_arr, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64)]
        d_words, d_path = t(words.view(np.int32), np.int32), t(path, np.int32)
        # stale values that must not survive
        res = dict(loglik=torch.full((n,), 0.5, dtype=torch.float64, device=dev),
                   rates=torch.zeros((n, R), dtype=torch.float64, device=dev),
                   states=torch.zeros((n, NS), dtype=torch.int32, device=dev),
                   naive=torch.full((n, L), 0x55, dtype=torch.uint8, device=dev),
                   naive_hash=torch.full((n,), 0x55, dtype=torch.int64, device=dev),
                   nt_hash=torch.full((n, D, P + 1), 0x55, dtype=torch.int64, device=dev),
                   aa_hash=torch.full((n, D, P + 1), 0x55, dtype=torch.int64, device=dev))
        stream = torch.cuda.current_stream().cuda_stream
        fam.eval_lineage_batch_device(n, T, depth, *[x.data_ptr() for x in d_in], R, d_words.data_ptr(), seed, first, D,
                                      d_path.data_ptr(), P, {k: v.data_ptr() for k, v in res.items()}, C.c_void_p(stream))
        status = ""
        try:
            fam.status()
        except RuntimeError as e:
            status = str(e)
        out = {k: v.cpu().numpy() for k, v in res.items()}
        for k in ("naive_hash", "nt_hash", "aa_hash"):
            out[k] = out[k].view(np.uint64)
        return out, status
    dev0, status0 = run(ops)
    hst = fam.eval_lineage_batch(T, depth, ops, brl, er, pi, alpha, R, words, seed, path, D, first)
    equal = all(np.array_equal(dev0[k], hst[k]) for k in hst)
    bad = ops.copy()
    victim = 1
    pops = [k for k in range(bad.shape[1]) if (bad[victim, k, 0] & 15) == 2]
    assert pops, "the victim's tree has a pending sibling"
    bad[victim, pops[0], 3] = 1 if bad[victim, pops[0], 3] == 0 else 0
    dev1, status1 = run(bad)
    ones = np.uint64(0xffffffffffffffff)
    keep = [i for i in range(n) if i != victim]
    others = all(np.array_equal(dev1[k][keep], dev0[k][keep]) for k in dev0)
    print(json.dumps({"clean_status": status0, "stream_equals_host": bool(equal), "bad_status": status1,
                      "victim_loglik_nan": bool(np.isnan(dev1["loglik"][victim])),
                      "victim_all_ones_in_every_draw": bool((dev1["nt_hash"][victim] == ones).all() and
                                                            (dev1["aa_hash"][victim] == ones).all()),
                      "others_unchanged": bool(others)}))
    fam.close()
    h.close()


if __name__ == "__main__":
    main()
