"""Helper of tests/test_gpu_viterbi.py::test_device_entry_point_and_rejected_schedule (its own process, as
tests/posterior_schedule_worker.py).  Runs lh_eval_viterbi_batch_device on a stream of torch's for a small synthetic
family, first as it is and then with one sample's DEVICE-RESIDENT schedule corrupted; prints a JSON line with what came
back."""
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
    from linearham_amd.capi import load_library
    from tests import viterbi_cases as vc
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    out = tempfile.mkdtemp(prefix="lh_vitdev_")
    n = 6
    o, rows, _ = vc.synthetic_rows(out, n, locus="igh", seed=31)
    hip = load_library()
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    rb = np.array([r["likelihood"] for r in rows])
    clean = vc.run_viterbi(hip, fam, inp, log_offset=rb, want=("loglik", "states", "log_path", "weight_stats"))
    S = clean["states"].shape[1]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_rb = t(rb, np.float64)
    stream = torch.cuda.Stream(device=dev)

    def run(ops):
        d = {"ops": t(ops, np.int32), "brlen": t(inp["brlen"], np.float64), "er": t(inp["er"], np.float64),
             "pi": t(inp["pi"], np.float64), "alpha": t(inp["alpha"], np.float64)}
        ll = torch.zeros(n, dtype=torch.float64, device=dev)
        lp = torch.zeros(n, dtype=torch.float64, device=dev)
        st = torch.zeros((n, S), dtype=torch.int32, device=dev)
        stats = torch.zeros(3, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_viterbi_batch_device(fam, n, inp["n_tips"], inp["max_depth"], d["ops"].data_ptr(), d["brlen"].data_ptr(),
                                          d["er"].data_ptr(), d["pi"].data_ptr(), d["alpha"].data_ptr(), inp["R"],
                                          dict(log_offset=d_rb.data_ptr(), loglik=ll.data_ptr(), states=st.data_ptr(),
                                               log_path=lp.data_ptr(), weight_stats=stats.data_ptr()),
                                          stream=stream.cuda_stream)
        stream.synchronize()
        status = hip.lib.lh_family_status(fam.handle)
        message = hip.error() if status else ""
        return int(status), message, ll.cpu().numpy(), lp.cpu().numpy(), st.cpu().numpy(), stats.cpu().numpy()

    status0, _, ll0, lp0, st0, stats0 = run(inp["ops"])
    same = all(a.tobytes() == b.tobytes() for a, b in ((ll0, clean["loglik"]), (lp0, clean["log_path"]),
                                                        (st0, clean["states"]), (stats0, clean["weight_stats"])))
    ops = inp["ops"].copy()
    victim = 2
    k_tip = next(k for k in range(ops.shape[1]) if (ops[victim, k, 0] & 15) == 1)  # a tip-into-accumulator op
    ops[victim, k_tip, 1] = 1 << 20  # a tip number far outside the alignment
    status, message, ll, lp, st, stats = run(ops)
    second = int(hip.lib.lh_family_status(fam.handle))
    keep = [i for i in range(n) if i != victim]
    lw = clean["loglik"][keep] - rb[keep]
    m = lw.max()
    w = np.exp(lw - m)
    print(json.dumps({"clean_status": status0, "clean_equal_host": bool(same), "status": status, "message": message,
                      "second_status": second, "victim_states_minus_one": bool(np.all(st[victim] == -1)),
                      "victim_log_path_nan": bool(np.isnan(lp[victim])), "victim_loglik_nan": bool(np.isnan(ll[victim])),
                      "others_equal_clean": bool(np.array_equal(st[keep], clean["states"][keep]) and
                                                 lp[keep].tobytes() == clean["log_path"][keep].tobytes()),
                      "max_lw_equal": bool(stats[0] == m), "sum_w_rel": float(abs(stats[1] - w.sum()) / w.sum()),
                      "sum_w2_rel": float(abs(stats[2] - (w * w).sum()) / (w * w).sum())}))
    fam.close()
    shutil.rmtree(out, ignore_errors=True)


def launch_groups(workdir):
    """`viterbi_device_worker.py --groups DIR` (the parent sets LH_CHUNK, which is read once per process): the 257-row
    batch of tests/test_gpu_viterbi.py::batch_family through lh_eval_viterbi_batch, cut into launch groups; prints the
    SHA-256 of every output's bytes."""
    import hashlib
    import numpy as np
    from linearham_amd.capi import load_library
    from tests import viterbi_cases as vc
    o, rows, _ = vc.synthetic_rows(workdir, 257, locus="igh", seed=77)
    hip = load_library()
    fam = vc.device_family(hip, o)
    inp = vc.device_inputs(hip, o, rows)
    rb = np.array([r["likelihood"] for r in rows])
    res = vc.run_viterbi(hip, fam, inp, log_offset=rb, want=("loglik", "states", "log_path", "weight_stats"))
    fam.close()
    print(json.dumps({k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in res.items()}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--groups":
        launch_groups(sys.argv[2])
    else:
        main()
