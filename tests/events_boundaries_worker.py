"""Helper of tests/test_gpu_events.py: tests/batch_boundaries_worker.py's scheme for lh_eval_events_batch, one case per
child process (LH_CHUNK, LH_HOST_SUB and LH_EVENTS_BLOCKS are read once per process).

    python -m tests.events_boundaries_worker <case> <directory> key=value ...

Prints one JSON line: {"failures": [...], "info": {...}}."""
import os
import sys

import numpy as np

from tests import batch_boundaries_worker as bw

def events(F, pk, R=4):
    ops, brl, er, pi, alpha = F.inputs(pk)
    return F.hip.eval_events_batch(F.fam, F.T, F.depth, ops, brl, er, pi, alpha, R,
                                   log_offset=np.ascontiguousarray(F.rb[pk]))


def build_anchors(d):
    """The 23 anchor rows as one call: writes d/events_anchors.npz and returns its contents."""
    F = bw.Fam(d, "igh")
    res = events(F, np.arange(bw.N_SETS))
    F.close()
    out = {k: res[k] for k in ("loglik", "events", "genes")}
    np.savez(os.path.join(d, "events_anchors.npz"), **out)
    return out


def case_events(d, rep, ns, G):
    """lh_eval_events_batch; group (LH_CHUNK) and slab (256) edges."""
    F = bw.Fam(d)
    A = np.load(os.path.join(d, "events_anchors.npz"))
    for n in ns:
        pk = bw.pick(n, G)
        what = "lh_eval_events_batch n=%d" % n
        res = events(F, pk)
        for k in ("events", "genes", "loglik"):
            rep.bits(what, k, res[k], A[k][pk], G)
        for rows, key in ((res["events"], "weighted_events"), (res["genes"], "weighted_genes")):
            bw._check_reduction(rep, what + " " + key, n, dict(res, weighted_sum=res[key].reshape(-1)), rows, F.rb[pk])
        again = events(F, pk)
        for k in ("weighted_events", "weighted_genes", "weight_stats"):
            rep.check(np.array_equal(again[k], res[k]), "%s %s: the same call twice gives different bits" % (what, k))
    F.close()


def main(argv):
    case, d = argv[0], argv[1]
    kw = {}
    for a in argv[2:]:
        k, v = a.split("=")
        kw[k] = [int(x) for x in v.split(",")] if k == "ns" else int(v)
    rep = bw.Report()
    {"events": case_events}[case](d, rep, **kw)
    rep.done()


if __name__ == "__main__":
    sys.path.insert(0, bw.ROOT)
    main(sys.argv[1:])
