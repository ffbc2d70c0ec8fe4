"""Helper of tests/test_gpu_events.py::test_device_entry_point (its own process, importing torch first, as
tests/posterior_schedule_worker.py).  Runs lh_eval_events_batch_device on a small synthetic family with device-resident
inputs on a stream: once clean, once with one sample's DEVICE-RESIDENT schedule corrupted; prints a JSON line."""
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
    from linearham_amd.capi import _EventsOutputsDevice, load_library
    from tools import synth_family as sf
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    out = tempfile.mkdtemp(prefix="lh_eventsdev_")
    sf.generate(sf.Spec.small(locus="igh", n_samples=6, seed=31), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    hip = load_library()
    fl = h.flatten_tsv(tsv, 6)
    rb = np.array([r["likelihood"] for r in sf.read_trees_tsv(tsv)])
    lay = hip.events_layout(fl["family"])
    clean = hip.eval_events_batch(fl["family"], fl["n_tips"], fl["max_depth"], fl["ops"], fl["brlen"], fl["er"],
                                  fl["pi"], fl["alpha"], 4, log_offset=rb)
    fam = C.c_void_p(fl["family"])
    ne, ng = lay["size"], lay["n_genes"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream()

    def run(ops):
        d = {"ops": t(ops, np.int32), "brlen": t(fl["brlen"], np.float64), "er": t(fl["er"], np.float64),
             "pi": t(fl["pi"], np.float64), "alpha": t(fl["alpha"], np.float64), "rb": t(rb, np.float64)}
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        o = dict(loglik=z(6), events=z(6, ne), genes=z(6, ng), weighted_events=z(ne), weighted_genes=z(ng),
                 weight_stats=z(3))
        torch.cuda.synchronize()
        outs = _EventsOutputsDevice(d["rb"].data_ptr(), *[o[k].data_ptr() for k in (
            "loglik", "events", "genes", "weighted_events", "weighted_genes", "weight_stats")])
        with torch.cuda.stream(stream):
            hip.check(hip.lib.lh_eval_events_batch_device(fam, 6, fl["n_tips"], fl["max_depth"], d["ops"].data_ptr(),
                                                          d["brlen"].data_ptr(), d["er"].data_ptr(), d["pi"].data_ptr(),
                                                          d["alpha"].data_ptr(), 4, C.byref(outs),
                                                          C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    same = run(fl["ops"])
    status_clean = hip.lib.lh_family_status(fam)
    bits = {k: bool(np.array_equal(same[k], clean[k])) for k in clean}
    ops = fl["ops"].copy()
    victim = 2
    k_tip = next(k for k in range(ops.shape[1]) if (ops[victim, k, 0] & 15) == 1)  # a tip-into-accumulator op
    ops[victim, k_tip, 1] = 1 << 20  # a tip number far outside the alignment
    bad = run(ops)
    status = hip.lib.lh_family_status(fam)
    message = hip.error() if status else ""
    second = hip.lib.lh_family_status(fam)
    keep = [i for i in range(6) if i != victim]
    lw = clean["loglik"][keep] - rb[keep]
    m = lw.max()
    w = np.exp(lw - m)
    st = bad["weight_stats"]

    def rel(got, ref):
        nz = ref != 0
        return float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0
    print(json.dumps({"same_bits": bits, "status_clean": int(status_clean), "status": int(status), "message": message,
                      "second_status": int(second),
                      "victim_all_nan": bool(np.all(np.isnan(bad["events"][victim])) and np.all(np.isnan(bad["genes"][victim]))
                                             and np.isnan(bad["loglik"][victim])),
                      "others_equal_clean": bool(np.array_equal(bad["events"][keep], clean["events"][keep]) and
                                                 np.array_equal(bad["genes"][keep], clean["genes"][keep])),
                      "max_lw_equal": bool(st[0] == m), "sum_w_rel": float(abs(st[1] - w.sum()) / w.sum()),
                      "sum_w2_rel": float(abs(st[2] - (w * w).sum()) / (w * w).sum()),
                      "weighted_events_rel": rel(bad["weighted_events"], w @ clean["events"][keep]),
                      "weighted_genes_rel": rel(bad["weighted_genes"], w @ clean["genes"][keep]),
                      "finite_sums": bool(np.all(np.isfinite(bad["weighted_events"])) and
                                          np.all(np.isfinite(bad["weighted_genes"])))}))
    shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    main()
