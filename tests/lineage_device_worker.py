"""Helper of tests/test_gpu_lineage.py::test_collect_device_and_a_rejected_schedule (its own process: torch first)."""
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
    from oracle import linearham_oracle as orc
    from tests import desc_builder as db
    from tools import synth_family as sf
    hip = linearham_amd.load_library()
    out = tempfile.mkdtemp(prefix="lh_lindev_")
    try:
        sf.generate(sf.Spec.small(n_leaves=12, n_samples=4, seed=31), out)
        h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
        rows = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    T, L, R = h.msa.shape[0] + 1, h.msa.shape[1], 4
    ops, brl, chains, depth = [], [], [], 0
    for r in rows:
        children, root, brlen = db.tree_arrays(orc.parse_newick(r["tree"]), h.xmsa_labels)
        o, d = hip.schedule_tree(T, children, root)
        ops.append(np.asarray(o, dtype=np.int32).reshape(-1, 4)), brl.append(brlen)
        depth = max(depth, d)
        children = np.asarray(children).ravel()
        parent = {}
        for v in range(T, 2 * T - 2):
            parent[int(children[2 * (v - T)])] = parent[int(children[2 * (v - T) + 1])] = v
        c = [parent[T - 1]]
        while c[-1] != root:
            c.append(parent[c[-1]])
        chains.append(c)
    ops = np.stack(ops)
    n = len(rows)
    P = max(len(c) for c in chains)
    path = np.full((n, P), -1, dtype=np.int32)
    for i, c in enumerate(chains):
        path[i, :len(c)] = c
    rates = np.stack([orc.gamma_rates_mean(r["alpha"], R) for r in rows])
    naive = np.random.default_rng(2).integers(0, 5, size=(n, L)).astype(np.uint8)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    def run(ops_arr, path_arr):
        d_ops, d_brl = t(ops_arr, np.int32), t(np.stack(brl), np.float64)
        d_er, d_pi = t([r["er"] for r in rows], np.float64), t([r["pi"] for r in rows], np.float64)
        d_rates, d_naive, d_path = t(rates, np.float64), t(naive, np.uint8), t(path_arr, np.int32)
        anc = torch.full((n, T - 2, L), 0x55, dtype=torch.uint8, device=dev)
        nt = torch.full((n, P + 1), 0x55, dtype=torch.int64, device=dev)      # stale values that must not survive
        aa = torch.full((n, P + 1), 0x55, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        hip.check(hip.lib.lh_asr_batch_device(fam.handle, n, T, depth, d_ops.data_ptr(), d_brl.data_ptr(), d_er.data_ptr(),
                                              d_pi.data_ptr(), d_rates.data_ptr(), R, d_naive.data_ptr(), C.c_uint64(9),
                                              C.c_uint64(0), anc.data_ptr(), None, C.c_void_p(stream)))
        fam.lineage_collect_device(n, T, anc.data_ptr(), d_naive.data_ptr(), d_path.data_ptr(), P, nt.data_ptr(),
                                   aa.data_ptr(), C.c_void_p(stream))
        status = ""
        try:
            fam.status()
        except RuntimeError as e:
            status = str(e)
        return anc.cpu().numpy(), nt.cpu().numpy().view(np.uint64), aa.cpu().numpy().view(np.uint64), status
    anc0, nt0, aa0, status0 = run(ops, path)
    # the host-pointer call on the same inputs and draws gives the same hashes
    nt_h, aa_h = fam.lineage_batch(T, depth, ops, np.stack(brl), [r["er"] for r in rows], [r["pi"] for r in rows], rates,
                                   naive, 9, path)
    # equal sequences, equal hashes; padding = the sentinel
    seen, ok = {}, True
    for i, c in enumerate(chains):
        for s, v in enumerate(c):
            ok = ok and seen.setdefault(anc0[i, v - T].tobytes(), int(nt0[i, s])) == int(nt0[i, s])
        ok = ok and all(int(nt0[i, s]) == 0 and int(aa0[i, s]) == 0 for s in range(len(c), P))
    ok = ok and len(set(seen.values())) == len(seen)
    # a path entry outside the inner nodes counts as padding (device-resident paths are not trusted)
    wild = path.copy()
    wild[0, 0] = 2 * T - 2
    wild[1, 0] = 0
    _, nt2, aa2, _ = run(ops, wild)
    wild_ok = int(nt2[0, 0]) == 0 and int(nt2[1, 0]) == 0 and np.array_equal(nt2[2:], nt0[2:]) and \
        np.array_equal(nt2[:2, 1:], nt0[:2, 1:])
    bad = ops.copy()
    victim = 1
    pops = [k for k in range(bad.shape[1]) if (bad[victim, k, 0] & 15) == 2]
    assert pops, "the victim's tree has a pending sibling"
    bad[victim, pops[0], 3] = 1 if bad[victim, pops[0], 3] == 0 else 0
    anc1, nt1, aa1, status1 = run(bad, path)
    ones = np.uint64(0xffffffffffffffff)
    others = all(np.array_equal(nt1[i], nt0[i]) and np.array_equal(aa1[i], aa0[i]) for i in range(n) if i != victim)
    print(json.dumps({"clean_status": status0, "clean_hashes_ok": bool(ok), "bad_status": status1,
                      "host_call_equal": bool(np.array_equal(nt_h, nt0) and np.array_equal(aa_h, aa0)),
                      "wild_path_is_padding": bool(wild_ok),
                      "victim_all_ones": bool((nt1[victim] == ones).all() and (aa1[victim] == ones).all()),
                      "others_unchanged": bool(others)}))
    fam.close()


if __name__ == "__main__":
    main()
