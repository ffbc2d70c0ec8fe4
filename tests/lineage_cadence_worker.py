"""Helper of tests/test_gpu_lineage_cadence.py: K11 (lh_asr_marginals_batch) and K12 (lh_asr_edges_batch, full and lean) on
the rows of tests/cadence_cases.py where the upward pass needs more than one 2^256 rescaling per op (the compound family) or
runs deep (cad190's lossy and zeroed rows), against the exact lineage reference (tests/exact_lineage_oracle.py).

  python tests/lineage_cadence_worker.py --cpu DIR [--jobs N]   CPU: DIR/lineage_<row>.npz per row -- the exact tables per seed
                                                                tip on the alignment's distinct columns, and d_ref, the distance
                                                                of the double-precision oracles from them
  python tests/lineage_cadence_worker.py --gpu DIR --family F   GPU: every row of family F, three seed tips, three naive-base
                                                                distributions; one JSON line {"failures": .., "figures": ..}

d_ref: tests/ancestral_marginal_oracle.marginals and tests/edge_oracle.edges restate the device's formulas in doubles (per
rate one message passed down the path, every table normalised per rate).  Here they get the exact model's P-matrices rounded
to double and an upward pass with the device's arithmetic -- after every node, 2^256 until the largest entry is back at or
above 2^-256 (upward_until) -- so that d_ref is what double precision itself costs on the row.  The device is held to
max(1e-10, 8 d_ref) per row, seed tip and table (the rule of tests/test_gpu_extreme_parameters.py; 1e-10 is the project's
bound for these tables, ancestral_cases.BOUND)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# family -> seed tips (tip ids: alignment row + 1).  cmp180: under the block's first ladder a tip that differs on the deep
# columns (44) and one that does not (41), and a background tip on the ladder above the block (101).  cad190: a tip of the
# mutated stretch of four deep columns (26), a tip of tree A's cherries (151), a tip near the root (181).
SEEDS = {"cmp180": (44, 41, 101), "cad190": (26, 151, 181)}
ROW_CLASSES = ("compound_control", "compound_clear", "compound_lossy", "compound_zeroed", "lossy", "zeroed")
Q_KINDS = ("one_hot", "dirichlet", "all_n")
K11_TABLES = ("marg", "rate_post")
K12_TABLES = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
LEAN_TABLES = K12_TABLES[1:]          # without "edge" lh_asr_edges_batch runs the lean kernel
FLOOR = 1e-10


def rows_of(family):
    from tests import cadence_cases as cc
    return [r for r in cc.ROWS if r[1] == family and r[2] in ROW_CLASSES]


def naive_rows(h):
    """The naive sequence's base per site, as the family's xMSA has it."""
    from tests import cadence_cases as cc
    site = cc.kc.column_sites(h)
    col_of = {}
    for c in range(len(site)):
        col_of.setdefault(int(site[c]), c)
    return np.array([int(h.xmsa[0, col_of[t]]) for t in range(h.msa.shape[1])])


def q_of(kind, h, n):
    """[n][L][5]: the naive sequence one-hot, benign Dirichlet rows (exact zeros, mass on N and one-hot rows among them),
    all mass on N."""
    from tests.ancestral_cases import naive_dist
    L = h.msa.shape[1]
    if kind == "one_hot":
        return np.tile(np.eye(5)[naive_rows(h)], (n, 1, 1))
    if kind == "dirichlet":
        return naive_dist(np.random.default_rng(2311), n, L)
    return np.tile(np.eye(5)[4], (n, L, 1))


def upward_until(children, root, T, tips, P):
    """oracle/asr_oracle.upward with the device's rescaling: after every node, times 2^256 until the largest entry is back
    at or above 2^-256 (an all-zero vector once; the device's rescale_steps wherever an op's product is a normal number,
    cadence_cases.restate_walk says where they part).  Returns clv [2T-2][L][4] and the log of the scale taken out per site."""
    L = tips.shape[1]
    onehot = np.concatenate([np.eye(4), np.ones((1, 4))], axis=0)
    clv, count = np.zeros((2 * T - 2, L, 4)), np.zeros(L)
    for t in range(T):
        clv[t] = onehot[tips[t]]
    order, stack = [], [int(root)]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(int(c) for c in children[2 * (v - T):2 * (v - T) + 2] if c >= T)
    for v in reversed(order):
        a, b = children[2 * (v - T)], children[2 * (v - T) + 1]
        x = np.einsum("ij,lj->li", P[a], clv[a]) * np.einsum("ij,lj->li", P[b], clv[b])
        need = x.max(axis=1) < 2.0 ** -256
        while need.any():
            x = np.where(need[:, None], x * 2.0 ** 256, x)
            count += need
            need = need & (x.max(axis=1) < 2.0 ** -256) & (x.max(axis=1) > 0)
        clv[v] = x
    return clv, -256.0 * np.log(2.0) * count


def double_pre(children, root, T, msa, pi, P):
    """ancestral_marginal_oracle._per_rate on given P-matrices [2T-2][R][4][4] with upward_until."""
    from tests import ancestral_marginal_oracle as amo
    L, R = msa.shape[1], P.shape[1]
    tips = np.concatenate([np.full((1, L), 4, dtype=msa.dtype), msa], axis=0)
    clvs, logscale, w = [], np.zeros((R, L)), np.zeros((R, L, 5))
    for k in range(R):
        clv, ls = upward_until(children, root, T, tips, P[:, k])
        clvs.append(clv)
        logscale[k] = ls
        w[k] = (np.asarray(pi)[None, :] * clv[root]) @ (P[0, k] @ amo.ONEHOT.T)
    with np.errstate(under="ignore"):
        lik = w * np.exp(logscale - logscale.max(axis=0, keepdims=True))[:, :, None]
    return P, clvs, lik


def exact_of_row(args):
    """One row in a pool process: the exact tables per seed tip (on the distinct columns) and d_ref per seed, q and table."""
    import shutil
    import tempfile
    import time
    from tests import ancestral_marginal_oracle as amo
    from tests import ancestral_probs_oracle as apo
    from tests import cadence_cases as cc
    from tests import edge_oracle as eo
    from tests import exact_lineage_oracle as xl
    from tests import exact_model_oracle as ex
    family, row = args
    work = tempfile.mkdtemp(prefix="lh_lineage_cadence_")
    try:
        h = cc.load_family(family, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    t0 = time.perf_counter()
    sample, R = cc.sample_of(row)
    T, children, root, brlen, ops, depth = cc.schedule(h, sample)
    rates = ex.gamma_rates_mean(sample["alpha"], R)                       # doubles: what the entry points are given
    model = ex.ExactModel(sample["er"], sample["pi"], [float(r) for r in rates])
    msa = np.asarray(h.msa)
    lin = xl.ExactLineage(model, T, children, root, brlen, msa)
    first = [int(np.nonzero(lin.pattern_of == p)[0][0]) for p in range(len(lin.patterns))]
    pre = double_pre(np.asarray(children).ravel(), root, T, msa, sample["pi"], model.pmatrices_double(brlen))
    keep = {"pattern_of": lin.pattern_of, "rates": rates}
    d_ref = {}
    for si, tip in enumerate(SEEDS[family]):
        path = amo.seed_path(children, root, T, tip)
        tab = lin.tables(path, tip)
        for k in ("cond", "cond_edge"):
            keep["%s_%d" % (k, si)] = tab[k][:, first]
        keep["rate_%d" % si] = tab["rate"][first]
        d13 = {}
        for node, slot in (("parent", 0), ("mrca", len(path) - 1)):
            with np.errstate(all="ignore"):
                G = apo.cond_tables(children, root, brlen, T, msa, sample["er"], sample["pi"], rates, path,
                                    apo.PARENT if slot == 0 else apo.MRCA, pre=pre)
            d13["k13_" + node] = float(np.abs(G - tab["cond"][slot]).max())
        d_ref["%d_cond" % si] = d13
        for kind in Q_KINDS:
            q = q_of(kind, h, 1)[0]
            want = xl.mix(tab, q)
            with np.errstate(all="ignore"):
                marg, rp = amo.marginals(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, pre=pre)
                ed = eo.edges(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, tip, pre=pre)
            d = {"k11_marg": np.abs(marg - want["marg"]).max(), "k11_rate_post": np.abs(rp - want["rate_post"]).max()}
            d.update({"k12_" + k: np.abs(ed[k] - want[k]).max() for k in K12_TABLES})
            d_ref["%d_%s" % (si, kind)] = {k: float(v) for k, v in d.items()}
    keep["d_ref"] = json.dumps(d_ref)
    keep["seconds"] = time.perf_counter() - t0
    return row[0], keep


def cpu_side(out_dir, jobs=1):
    """DIR/lineage_<row>.npz for every row of both families; returns {row: (d_ref dict, seconds)}."""
    os.makedirs(out_dir, exist_ok=True)
    todo = [(family, row) for family in SEEDS for row in rows_of(family)]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            done = pool.map(exact_of_row, todo)
    else:
        done = [exact_of_row(t) for t in todo]
    out = {}
    for name, keep in done:
        np.savez(os.path.join(out_dir, "lineage_%s.npz" % name), **keep)
        out[name] = (json.loads(keep["d_ref"]), float(keep["seconds"]))
    return out


def exact_tables(x, si):
    """ExactLineage.tables of seed tip number si, spread from the distinct columns back over the sites."""
    po = x["pattern_of"]
    return dict(cond=x["cond_%d" % si][:, po], cond_edge=x["cond_edge_%d" % si][:, po], rate=x["rate_%d" % si][po])


def run_gpu(out_dir, family, workdir):
    import linearham_amd
    from linearham_amd import capi
    from tests import cadence_cases as cc
    from tests import desc_builder as db
    from tests import exact_lineage_oracle as xl
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    h = cc.load_family(family, workdir)
    rows = rows_of(family)
    R = cc.FAMILIES[family]["R"]
    samples = [cc.sample_of(r)[0] for r in rows]
    sched = [cc.schedule(h, s) for s in samples]
    T, depth = sched[0][0], max(s[5] for s in sched)
    ops, brl = np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched])
    er, pi = [s["er"] for s in samples], [s["pi"] for s in samples]
    ref = [np.load(os.path.join(out_dir, "lineage_%s.npz" % r[0])) for r in rows]
    rates = np.stack([x["rates"] for x in ref])
    d_ref = [json.loads(str(x["d_ref"])) for x in ref]
    n = len(rows)
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    failures, figures = [], []

    def note(cond, text):
        if not cond:
            failures.append(text)

    for si, tip in enumerate(SEEDS[family]):
        paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
        padded = capi.pad_paths(paths)
        tabs = [exact_tables(x, si) for x in ref]
        for kind in Q_KINDS:
            q = np.tile(q_of(kind, h, 1), (n, 1, 1))               # (the rows d_ref was measured with)
            marg, rp = fam.asr_marginals_batch(T, depth, ops, brl, er, pi, rates, q, padded)
            full = fam.asr_edges_batch(T, depth, ops, brl, er, pi, rates, q, padded, tip, want=K12_TABLES)
            lean = fam.asr_edges_batch(T, depth, ops, brl, er, pi, rates, q, padded, tip, want=LEAN_TABLES)
            if si == 0:             # every row alone: the same bits as in the batch
                for i, r in enumerate(rows):
                    m1, r1 = fam.asr_marginals_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                                     q[i:i + 1], capi.pad_paths(paths[i:i + 1]))
                    e1 = fam.asr_edges_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                             q[i:i + 1], capi.pad_paths(paths[i:i + 1]), tip, want=K12_TABLES)
                    l1 = fam.asr_edges_batch(T, depth, ops[i:i + 1], brl[i:i + 1], er[i:i + 1], pi[i:i + 1], rates[i:i + 1],
                                             q[i:i + 1], capi.pad_paths(paths[i:i + 1]), tip, want=LEAN_TABLES)
                    P = len(paths[i])

                    def load(v):            # a batch pads the paths to its longest: slots [0, P) and the naive edge's
                        return np.concatenate([v[:P], v[-1:]])
                    same = [np.array_equal(m1[0], marg[i, :P]), np.array_equal(r1[0], rp[i]),
                            np.array_equal(e1["edge"][0], full["edge"][i, :P])]
                    for alone, batch in ((e1, full), (l1, lean)):
                        same += [np.array_equal(alone[k][0], batch[k][i]) for k in ("naive_edge", "chain_counts", "rate_post")]
                        same.append(np.array_equal(alone["edge_load"][0], load(batch["edge_load"][i])))
                    note(all(same), "%s tip %d %s: not bit-identical alone and in the batch: %s" % (r[0], tip, kind, same))
            for i, r in enumerate(rows):
                P = len(paths[i])
                want = xl.mix(tabs[i], q[i])
                dr = d_ref[i]["%d_%s" % (si, kind)]
                where = "%s tip %d %s" % (r[0], tip, kind)
                got = {"k11_marg": marg[i, :P], "k11_rate_post": rp[i]}
                for key in K12_TABLES:
                    v = full[key][i]
                    got["k12_" + key] = v[:P] if key == "edge" else np.concatenate([v[:P], v[-1:]]) if key == "edge_load" else v
                for key in LEAN_TABLES:
                    v = lean[key][i]
                    got["k12lean_" + key] = np.concatenate([v[:P], v[-1:]]) if key == "edge_load" else v
                fig = dict(row=r[0], cls=r[2], tip=tip, q=kind, path=P)
                for key, v in got.items():
                    base = key.split("_", 1)[1]
                    ref_key = key if key in dr else "k12_" + base
                    bound = max(FLOOR, 8.0 * dr[ref_key])
                    with np.errstate(invalid="ignore"):
                        d = float(np.abs(v - want[base]).max()) if np.isfinite(v).all() else float("inf")
                    fig[key] = d
                    fig["ref_" + ref_key] = dr[ref_key]
                    note(d <= bound, "%s: %s off the exact reference by %.3g (bound %.3g, d_ref %.3g)" % (where, key, d, bound, dr[ref_key]))
                # distributions
                sums = [np.abs(marg[i, :P].sum(axis=-1) - 1).max(), np.abs(rp[i].sum(axis=-1) - 1).max(),
                        np.abs(full["rate_post"][i].sum(axis=-1) - 1).max(), np.abs(lean["rate_post"][i].sum(axis=-1) - 1).max()]
                fig["sum_to_one"] = float(np.nanmax(sums)) if np.isfinite(sums).all() else float("inf")
                note(fig["sum_to_one"] <= 1e-12, "%s: marginals or rate posteriors do not sum to 1: %s" % (where, sums))
                note(not marg[i, P:].any() and not full["edge"][i, P:].any(), "%s: the padding slots are not 0" % where)
                # K12's four margin identities against K11's device output
                e, ne, m = full["edge"][i, :P], full["naive_edge"][i], marg[i, :P]
                ident = [np.abs(e.sum(axis=-1) - m).max(), np.abs(e[1:].sum(axis=-2) - m[:-1]).max() if P > 1 else 0.0,
                         np.abs(ne.sum(axis=-1) - q[i]).max(), np.abs(ne.sum(axis=-2) - m[P - 1]).max()]
                fig["identities"] = float(max(ident)) if np.isfinite(ident).all() else float("inf")
                note(fig["identities"] <= 1e-12, "%s: K12's margins against K11: %s" % (where, ident))
                figures.append(fig)
    # ---- K13b's conditional tables: lh_eval_ancestral_candidates_batch's `cond` at both nodes, on the family as the host
    # library reads it, against the exact tables and against five one-hot calls of lh_asr_marginals_batch.  (Default mode:
    # the entry point refuses extended-range handles.  The deep columns' emissions are 0 there and the log-likelihood is
    # not finite; `cond` does not depend on either -- it is built from K1's unmixed planes and their counts.)
    from linearham_amd import host
    from tests.ancestral_cases import write_table
    yaml_path, pdir = cc.write_family_files(family, workdir, h)
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    tsv = os.path.join(workdir, "rows.tsv")
    write_table(tsv, samples[:1])
    hfam = hh.flatten_tsv(tsv, 1)["family"]
    L = h.msa.shape[1]
    hip.set_ancestral_candidates(hfam, np.full((1, L), 4, dtype=np.uint8))
    alpha = np.array([s["alpha"] for s in samples])
    cond_figures = []
    for si, tip in enumerate(SEEDS[family]):
        paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
        padded = capi.pad_paths(paths)
        tabs = [exact_tables(x, si) for x in ref]
        k11 = []
        for b in range(5):
            marg, _ = fam.asr_marginals_batch(T, depth, ops, brl, er, pi, rates, np.tile(np.eye(5)[b], (n, L, 1)), padded,
                                              want=("marg",))
            k11.append(marg)
        for node, name in ((capi.NODE_PARENT, "parent"), (capi.NODE_MRCA, "mrca")):
            res = hip.eval_ancestral_candidates_batch(hfam, T, depth, ops, brl, np.array(er), np.array(pi), alpha, R, padded, node,
                                                      want=("cond",))
            for i, r in enumerate(rows):
                slot = 0 if name == "parent" else len(paths[i]) - 1
                got = res["cond"][i]
                dr = d_ref[i]["%d_cond" % si]["k13_" + name]
                bound = max(FLOOR, 8.0 * dr)
                where = "%s tip %d %s" % (r[0], tip, name)
                ok = bool(np.isfinite(got).all())
                d = float(np.abs(got - tabs[i]["cond"][slot]).max()) if ok else float("inf")
                d11 = float(max(np.abs(got[:, b] - k11[b][i, slot]).max() for b in range(5))) if ok else float("inf")
                s1 = float(np.abs(got.sum(axis=-1) - 1).max()) if ok else float("inf")
                note(d <= bound, "%s: k13_cond off the exact reference by %.3g (bound %.3g, d_ref %.3g)" % (where, d, bound, dr))
                note(d11 <= 1e-12, "%s: K13's cond against five one-hot K11 calls: %.3g" % (where, d11))
                note(s1 <= 1e-12, "%s: K13's cond rows do not sum to 1: %.3g" % (where, s1))
                cond_figures.append(dict(row=r[0], cls=r[2], tip=tip, node=name, k13_cond=d, ref_k13=dr, k13_vs_k11=d11, sum_to_one=s1))
                if si == 0:         # the row alone: the same bits as in the batch
                    one = hip.eval_ancestral_candidates_batch(hfam, T, depth, ops[i:i + 1], brl[i:i + 1], np.array(er[i:i + 1]),
                                                              np.array(pi[i:i + 1]), alpha[i:i + 1], R,
                                                              capi.pad_paths(paths[i:i + 1]), node, want=("cond",))
                    note(np.array_equal(one["cond"][0], got), "%s: K13's cond not bit-identical alone and in the batch" % where)
    fam.close()
    print(json.dumps({"failures": failures, "figures": figures, "cond_figures": cond_figures, "rows": n}))


def main(argv):
    import shutil
    import tempfile

    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    if "--cpu" in argv:
        for name, (d, sec) in cpu_side(opt("--cpu"), int(opt("--jobs", "1"))).items():
            worst = {}
            for dd in d.values():
                for k, v in dd.items():
                    worst[k] = max(worst.get(k, 0.0), v)
            print("%-16s %.1f s  d_ref %s" % (name, sec, "  ".join("%s %.2g" % kv for kv in worst.items())))
        return 0
    work = tempfile.mkdtemp(prefix="lh_lineage_cadence_")
    try:
        run_gpu(opt("--gpu"), opt("--family"), work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
