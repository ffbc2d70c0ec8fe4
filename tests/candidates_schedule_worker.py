"""Helper of tests/test_gpu_naive_probs.py::test_rejected_device_schedule (its own process, as
tests/posterior_schedule_worker.py).  Runs lh_eval_candidates_batch_device on a small synthetic family with one row's
DEVICE-RESIDENT schedule corrupted; prints a JSON line with what came back."""
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
    from linearham_amd import host
    from linearham_amd.capi import _CandidateOutputs, load_library
    from oracle import linearham_oracle as orc
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    out = tempfile.mkdtemp(prefix="lh_candsched_")
    sf.generate(sf.Spec.small(locus="igh", n_samples=6, seed=31), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    r = rows[0]
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
    o.initialize_phylo_emission()
    o.log_likelihood()
    seen = {}
    for _ in range(30):
        seen.setdefault(o.sample_naive_sequence(), None)
    cands = np.array([["ACGTN".index(c) for c in s] for s in seen], dtype=np.uint8)
    K = len(cands)
    hip = load_library()
    fl = h.flatten_tsv(tsv, 6)
    hip.set_candidates(fl["family"], cands)
    rb = np.array([r["likelihood"] for r in rows])
    clean = hip.eval_candidates_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"], fl["er"],
                                      fl["pi"], fl["alpha"], 4, log_offset=rb)
    ops = fl["ops"].copy()
    victim = 2
    k_tip = next(k for k in range(ops.shape[1]) if (ops[victim, k, 0] & 15) == 1)  # a tip-into-accumulator op
    ops[victim, k_tip, 1] = 1 << 20  # a tip number far outside the alignment
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d = {"ops": t(ops, np.int32), "brlen": t(fl["brlen"], np.float64), "er": t(fl["er"], np.float64),
         "pi": t(fl["pi"], np.float64), "alpha": t(fl["alpha"], np.float64)}
    d_rb = t(rb, np.float64)
    fam = C.c_void_p(fl["family"])
    lc = torch.zeros((6, K), dtype=torch.float64, device=dev)
    ll = torch.zeros(6, dtype=torch.float64, device=dev)
    wsum = torch.zeros(K, dtype=torch.float64, device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    P = lambda x: C.cast(C.c_void_p(x.data_ptr()), C.POINTER(C.c_double))
    outs = _CandidateOutputs(P(d_rb), P(ll), P(lc), P(wsum), P(stats))
    stream = torch.cuda.current_stream().cuda_stream
    hip.check(hip.lib.lh_eval_candidates_batch_device(fam, 6, fl["n_tips"], fl["max_depth"], d["ops"].data_ptr(),
                                                      d["brlen"].data_ptr(), d["er"].data_ptr(), d["pi"].data_ptr(),
                                                      d["alpha"].data_ptr(), 4, C.byref(outs), C.c_void_p(stream)))
    torch.cuda.synchronize()
    status = hip.lib.lh_family_status(fam)
    message = hip.error() if status else ""
    second = hip.lib.lh_family_status(fam)
    p, l = lc.cpu().numpy(), ll.cpu().numpy()
    keep = [i for i in range(6) if i != victim]
    lw = clean["loglik"][keep] - rb[keep]
    m = lw.max()
    w = np.exp(lw - m)
    st = stats.cpu().numpy()
    ref = w @ np.exp(clean["log_cand"][keep])
    got = wsum.cpu().numpy()
    nz = ref != 0
    print(json.dumps({"status": int(status), "message": message, "second_status": int(second),
                      "victim_all_nan": bool(np.all(np.isnan(p[victim]))), "victim_loglik_nan": bool(np.isnan(l[victim])),
                      "others_equal_clean": bool(np.array_equal(p[keep], clean["log_cand"][keep])),
                      "max_lw_equal": bool(st[0] == m), "sum_w_rel": float(abs(st[1] - w.sum()) / w.sum()),
                      "sum_w2_rel": float(abs(st[2] - (w * w).sum()) / (w * w).sum()),
                      "weighted_sum_rel": float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0}))
    shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    main()
