"""K14 at a slot per row in extended range: the CPU side of tests/test_gpu_clade_slot.py's case on two rows of
tests/ext_deep_cases.py, one control row and one spread row of cad190 (the spread row's deep columns lie below 2^-1074: the
default mode has no finite log-likelihood for it).

For the chosen seed tip of lineage_cadence_worker.SEEDS and a partner tip whose common ancestor with the seed lies strictly
inside the seed's path in both rows, per row: the exact tables cond[slot] (tests/exact_lineage_oracle.py, mpmath) contracted
with the row's reference naive codon posterior Q_ref (node_codon_oracle.contraction / change), and d_ref, the distance of the
same contraction of the double-precision oracle's tables at that slot from it.  The device bound is ext_deep_cases.bound(d_ref)."""
import json
import os

import numpy as np

FAMILY = "cad190"
ROWS = ("control_b", "spread_a10")
FRAME = 0


def choose(trees, T, seeds):
    """(seed tip, partner tip, [slot per row]): the first seed of `seeds`, else the first other tip, that has a partner whose
    common ancestor with it is interior in every row."""
    from linearham_amd import host
    for tip in list(seeds) + [t for t in range(1, T) if t not in seeds]:
        lens = [len(host.seed_path(T, ch, rt, tip)) for ch, rt in trees]
        for u in range(1, T):
            if u == tip:
                continue
            slots = [host.clade_slot(T, ch, rt, tip, [u])[1] for ch, rt in trees]
            if all(0 < s < n - 1 for s, n in zip(slots, lens)):
                return tip, u, slots
    raise AssertionError("no tip of these trees has an interior common ancestor in every row")


def row_reference(args):
    """One row in a pool process: (name, dict for the row's npz) for the seed `tip` at `slot`."""
    from tests import ancestral_marginal_oracle as amo
    from tests import cadence_cases as cc
    from tests import ext_deep_cases as xd
    from tests import lineage_cadence_worker as lw
    from tests import node_codon_oracle as nco
    name, tip, slot = args
    row = {r[0]: r for r in list(cc.ROWS) + list(xd.SPREAD)}[name]
    _, keep = xd.build_row((FAMILY, row, False))
    Q = keep["Q%d" % FRAME]
    s = lw._row_setup(FAMILY, row)
    sample, T, children, root, brlen, rates, msa, lin, pre = (s[k] for k in ("sample", "T", "children", "root", "brlen", "rates",
                                                                            "msa", "lin", "pre"))
    path = amo.seed_path(children, root, T, tip)
    assert 0 < slot < len(path) - 1
    exact = lin.tables(path, tip)["cond"][slot]
    L = np.asarray(msa).shape[1]
    G = np.zeros((L, 5, 4))
    with np.errstate(all="ignore"):
        for b in range(5):
            q = np.zeros((L, 5))
            q[:, b] = 1.0
            marg, _ = amo.marginals(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, pre=pre)
            G[:, b] = marg[slot]
        want = {"codons": nco.contraction(Q, exact, FRAME), "change": nco.change(Q, exact, FRAME)}
        double = {"codons": nco.contraction(Q, G, FRAME), "change": nco.change(Q, G, FRAME)}
    d_ref = {k: float(np.abs(np.asarray(double[k], dtype=float) - np.asarray(want[k], dtype=float)).max()) for k in want}
    fig = json.loads(str(keep["figures"]))
    return name, dict(codons=np.asarray(want["codons"], dtype=float), change=np.asarray(want["change"], dtype=float),
                      d_ref=json.dumps(d_ref), kind=fig["kind"], numpy_finite=bool(fig["numpy_finite"]), slot=slot,
                      path_len=len(path), loglik=float(keep["loglik"]))


def rows():
    from tests import cadence_cases as cc
    from tests import ext_deep_cases as xd
    by = {r[0]: r for r in list(cc.ROWS) + list(xd.SPREAD)}
    return [by[n] for n in ROWS]


def build(out_dir, jobs=2):
    """DIR/clade_slot_ext_<row>.npz and DIR/clade_slot_ext.json (seed tip, partner, slots, d_ref per row); returns the json."""
    import shutil
    import tempfile
    from tests import cadence_cases as cc
    from tests import lineage_cadence_worker as lw
    os.makedirs(out_dir, exist_ok=True)
    work = tempfile.mkdtemp(prefix="lh_clade_ext_")
    try:
        h = cc.load_family(FAMILY, work)
        sched = [cc.schedule(h, cc.sample_of(r)[0]) for r in rows()]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    T = sched[0][0]
    tip, partner, slots = choose([(s[1], s[2]) for s in sched], T, lw.SEEDS[FAMILY])
    todo = [(name, tip, slot) for name, slot in zip(ROWS, slots)]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            done = pool.map(row_reference, todo, chunksize=1)
    else:
        done = [row_reference(t) for t in todo]
    meta = dict(family=FAMILY, rows=list(ROWS), frame=FRAME, seed_tip=tip, from_seeds=tip in lw.SEEDS[FAMILY], partner=partner,
                slots=slots, d_ref={}, kinds={}, numpy_finite={}, path_len={})
    for name, keep in done:
        np.savez(os.path.join(out_dir, "clade_slot_ext_%s.npz" % name), codons=keep["codons"], change=keep["change"])
        meta["d_ref"][name] = json.loads(keep["d_ref"])
        meta["kinds"][name], meta["numpy_finite"][name], meta["path_len"][name] = keep["kind"], keep["numpy_finite"], keep["path_len"]
    json.dump(meta, open(os.path.join(out_dir, "clade_slot_ext.json"), "w"))
    return meta
