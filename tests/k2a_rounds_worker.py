"""Helper of tests/test_gpu_k2a_consensus_rounds.py (its own process: LH_K2A_DIRECT is read when a family is created, and one
child runs with it and one without).

    k2a_rounds_worker.py CASES.pkl OUT.npz

CASES.pkl holds the oracle object of the crafted family and the emission vectors (one row per case).  All rows run as ONE
lh_forward_batch call (the caller's emissions: K2a's kFromSiteLik = false entry); log-likelihoods, forward arrays and
ScaleMatrix counts go to OUT.npz, and one JSON line {form, consensus_sets} is printed."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main(argv):
    import linearham_amd
    from tests import desc_builder as db
    with open(argv[0], "rb") as f:
        h, names, ems = pickle.load(f)
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    ll, res = fam.forward_batch(np.stack(ems), want=("forward", "scaler_counts"))
    info = {"form": fam.k2_form(), "consensus_sets": int(fam.consensus_sets), "cases": names}
    # every row again alone: a wave's ballot must not let a neighbour's round show in another row's bits
    alone = [fam.forward_batch(em[None], want=("forward", "scaler_counts")) for em in ems]
    fam.close()
    np.savez(argv[1], loglik=ll, forward=res["forward"], scaler_counts=res["scaler_counts"],
             alone_loglik=np.array([a[0][0] for a in alone]), alone_forward=np.stack([a[1]["forward"][0] for a in alone]),
             alone_scaler_counts=np.stack([a[1]["scaler_counts"][0] for a in alone]))
    print(json.dumps(info))


if __name__ == "__main__":
    main(sys.argv[1:])
