"""Helper of tests/test_gpu_treepass_pattern_edges.py: the tree-pass kernels -- tree_upward under K3b / K11b / K12b, cond_kernel
in its three forms (K13b, and through it K14), K15b, and the down passes' site loops -- on the crafted families of
tests/pattern_edge_cases.TREEPASS, each kernel against the oracle its own module uses, at that module's bound.

    treepass_pattern_edges_worker.py <first case> <one past the last case> <workdir>

One JSON line: per case its figures (the largest deviation per quantity) and failures (what did not hold)."""
import json
import os
import pathlib
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K12_TABLES = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
LEAN_TABLES = K12_TABLES[1:]        # without "edge" lh_asr_edges_batch runs the lean kernel
FRAME = 1
K3_SEED, K3_FIRST = 20261004, 7


def block_edge_sites(n_sites):
    """The first and last site of every block of 64 sites."""
    s = sorted({b for b in range(0, n_sites, 64)} | {min(b + 63, n_sites - 1) for b in range(0, n_sites, 64)})
    return s


def pick_tips(c):
    """Two seed tips whose paths differ in length in row 0, each with an interior slot in both rows where the tree has one."""
    best = None
    for a in range(1, c.T):
        for b in range(a + 1, c.T):
            la, lb = len(c.path(0, a)), len(c.path(0, b))
            if la == lb:
                continue
            inner = sum(c.pick(r, t, "interior") is not None for r in (0, 1) for t in (a, b))
            key = (inner, min(la, lb) >= 2, abs(la - lb))
            if best is None or key > best[0]:
                best = (key, (a, b))
    assert best is not None, "every tip's path has the same length"
    return best[1]


def run_case(hip, case, R, workdir):
    import numpy as np
    from linearham_amd import capi
    from tests import ancestral_probs_oracle as apo
    from tests import codon_edge_oracle as ceo
    from tests import codon_edges_cases as cec
    from tests import node_codon_oracle as nco
    from tests import pattern_edge_cases as pe
    from tests.ancestral_cases import BOUND, naive_dist
    from tests.ancestral_probs_cases import MRCA, PARENT
    from tests.clade_slot_cases import LOG_CAND_BOUND, AtCase
    from tests.edges_cases import EdgeCase

    class TreeCase(AtCase, cec.CodonEdgesCase):
        pass

    import time
    t0 = time.perf_counter()
    failures, fig = [], {}

    def note(ok, text):
        if not ok:
            failures.append(text)

    def far(name, v):
        v = float(v) if np.isfinite(v) else float("inf")
        fig[name] = max(fig.get(name, 0.0), v)
        return fig[name]

    yaml_path, pdir = pe.write_case_files(case, workdir)
    rows = pe.samples(case.base, workdir)
    tmp = pathlib.Path(workdir) / ("tp_" + case.name + "_R%d" % R)
    tmp.mkdir(exist_ok=True)
    c = TreeCase(hip, yaml_path, pdir, rows, R, tmp)
    msa_want, site_pat = pe.alignment(case, c.T - 1, c.L)
    assert np.array_equal(c.o.msa, msa_want)
    fam = capi.Family.borrow(c.family, hip)
    note(fam.info()[0] == case.L, "n_prune is %d" % fam.info()[0])
    ec = EdgeCase(hip, c.o, rows, R)
    t1, t2 = pick_tips(c)
    pairs = [(0, t1), (1, t1), (0, t2), (1, t2)]
    paths = [c.path(*p) for p in pairs]
    lens = [len(p) for p in paths]
    slots = [c.pick(r, t, "interior") for r, t in pairs]
    slots = [s if s is not None else n // 2 for s, n in zip(slots, lens)]
    premises = dict(tips=[t1, t2], lengths=lens, slots=slots, n_pat=case.L + 1 + int(case.all_n), sites=c.L)
    rng = np.random.default_rng(1000 + case.L)
    same = [np.nonzero(site_pat == p)[0] for p in np.unique(site_pat) if (site_pat == p).sum() > 1]

    # ---- K11 (lh_asr_marginals_batch: tree_upward, the down pass a lane per site) and K12, full and lean
    q = naive_dist(rng, len(rows), c.L)
    epaths = [ec.path(*p) for p in pairs]       # (the oracle object's node numbers: desc_builder.tree_arrays)
    assert [len(p) for p in epaths] == lens
    marg, rp, _ = ec.batch(pairs, q)
    for i, (row, tip) in enumerate(pairs):
        P = lens[i]
        want, want_rp = ec.oracle(row, q[row], epaths[i])
        far("k11_marg", np.abs(marg[i, :P] - want).max()), far("k11_rate_post", np.abs(rp[i] - want_rp).max())
        far("k11_sum_to_one", max(np.abs(marg[i, :P].sum(axis=-1) - 1).max(), np.abs(rp[i].sum(axis=-1) - 1).max()))
        note(not marg[i, P:].any(), "K11: padding slots of pair %d are not 0" % i)
        m1, r1, _ = ec.batch([pairs[i]], q)
        note(np.array_equal(m1[0, :P], marg[i, :P]) and np.array_equal(r1[0], rp[i]), "K11: pair %d alone differs from the batch" % i)
    note(fig["k11_marg"] < BOUND and fig["k11_rate_post"] < BOUND, "K11 against the oracle")
    note(fig["k11_sum_to_one"] < 1e-12, "K11: tables do not sum to 1")
    for tip in (t1, t2):
        where = [i for i, p in enumerate(pairs) if p[1] == tip]
        rws = [pairs[i][0] for i in where]
        full, _ = ec.call(rws, tip, q, want=K12_TABLES)
        lean, _ = ec.call(rws, tip, q, want=LEAN_TABLES)
        for k, i in enumerate(where):
            P = lens[i]
            want = ec.edge_oracle(rws[k], q[rws[k]], epaths[i], tip)
            load = lambda v: np.concatenate([v[:P], v[-1:]])
            far("k12_edge", np.abs(full["edge"][k, :P] - want["edge"]).max())
            for tag, res in (("k12", full), ("k12lean", lean)):
                for key in ("naive_edge", "chain_counts", "rate_post"):
                    far("%s_%s" % (tag, key), np.abs(res[key][k] - want[key]).max())
                far(tag + "_edge_load", np.abs(load(res["edge_load"][k]) - want["edge_load"]).max())
                note(not res["edge_load"][k, P:-1].any(), "%s: padding slots of pair %d are not 0" % (tag, i))
            note(not full["edge"][k, P:].any(), "K12: padding slots of pair %d are not 0" % i)
            cells = full["chain_counts"][k].sum(axis=(-1, -2))
            far("k12_cells", np.abs(cells - (P + 1 - q[rws[k]][:, 4])).max())
            one_f, _ = ec.call([rws[k]], tip, q, want=K12_TABLES)
            one_l, _ = ec.call([rws[k]], tip, q, want=LEAN_TABLES)
            ok = np.array_equal(one_f["edge"][0, :P], full["edge"][k, :P])
            for alone, batch in ((one_f, full), (one_l, lean)):
                ok = ok and all(np.array_equal(alone[key][0], batch[key][k]) for key in ("naive_edge", "chain_counts", "rate_post"))
                ok = ok and np.array_equal(alone["edge_load"][0], load(batch["edge_load"][k]))
            note(ok, "K12: pair %d alone differs from the batch" % i)
    note(all(fig[k] < BOUND for k in fig if k.startswith("k12") and k != "k12_cells"), "K12 against the oracle")
    note(fig["k12_cells"] < 1e-12, "K12: chain_counts' sum rule")

    # ---- K13b's cond in its three forms, against the oracle's tables and against five one-hot K11 calls
    G_all = [c.tables_at(row, paths[i]) for i, (row, _) in enumerate(pairs)]
    c.hip.set_ancestral_candidates(c.family, np.full((1, c.L), apo.OPEN, dtype=np.uint8))
    a = c.args([p[0] for p in pairs])
    _, ev = fam.eval_batch(*a, want=("rates",))
    padded = capi.pad_paths(paths)
    k11 = np.zeros((len(pairs), max(lens), c.L, 5, 4))
    for b in range(5):
        hot = np.zeros((len(pairs), c.L, 5))
        hot[:, :, b] = 1.0
        m, _ = fam.asr_marginals_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], hot, padded, want=("marg",))
        k11[:, :, :, b] = m
    forms = (("parent", [0] * len(pairs), lambda: c.probs(pairs, PARENT, want=("cond",))[0]),
             ("mrca", [n - 1 for n in lens], lambda: c.probs(pairs, MRCA, want=("cond",))[0]),
             ("slot", slots, lambda: c.probs_at(pairs, slots, want=("cond",))[0]))
    for name, at, call in forms:
        cond = call()["cond"]
        for i in range(len(pairs)):
            far("k13_cond_" + name, np.abs(cond[i] - G_all[i][at[i]]).max())
            far("k13_cond_vs_k11", np.abs(cond[i] - k11[i, at[i]]).max())
            far("k13_cond_sum_to_one", np.abs(cond[i].sum(axis=-1) - 1).max())
            # a site's table is that of every other site with its pattern, bit for bit (site_gather_kernel, site_pat)
            note(all(np.array_equal(cond[i, s[0]], cond[i, j]) for s in same for j in s[1:]),
                 "K13b %s: sites of one pattern differ, pair %d" % (name, i))
            if name == "parent":
                alone = c.probs([pairs[i]], PARENT, want=("cond",))[0]["cond"]
            elif name == "mrca":
                alone = c.probs([pairs[i]], MRCA, want=("cond",))[0]["cond"]
            else:
                alone = c.probs_at([pairs[i]], [slots[i]], want=("cond",))[0]["cond"]
            note(np.array_equal(alone[0], cond[i]), "K13b %s: pair %d alone differs from the batch" % (name, i))
        note(fig["k13_cond_" + name] < BOUND, "K13b %s against the oracle" % name)
    note(fig["k13_cond_vs_k11"] < 1e-12 and fig["k13_cond_sum_to_one"] < 1e-12, "K13b against K11 / sums to 1")

    # ---- K13 log_cand at the interior slot: one-site candidates at the first and last site of every block of 64 sites
    sites = block_edge_sites(c.L)
    cands = np.concatenate([apo.one_site(c.L, s) for s in sites] + [np.full((1, c.L), apo.OPEN, dtype=np.uint8)])
    res, _ = c.probs_at(pairs, slots, cands, want=("log_cand",))
    note(bool((res["log_cand"][:, -1] == 0.0).all()), "K13: the all-open candidate is not exactly 0")
    for i in (0, 3):                     # (one dense sweep per candidate: two of the four pairs, one per row and tip)
        want = c.oracle_log_cand(pairs[i][0], G_all[i][slots[i]], cands)
        fin = np.isfinite(want)
        note(np.array_equal(np.isfinite(res["log_cand"][i]), fin), "K13 log_cand: finiteness differs, pair %d" % i)
        far("k13_log_cand", np.abs(res["log_cand"][i][fin] - want[fin]).max())
    note(fig["k13_log_cand"] < LOG_CAND_BOUND, "K13 log_cand against the oracle")
    premises["candidates"] = int(len(cands))
    c.hip.set_ancestral_candidates(c.family, np.full((1, c.L), apo.OPEN, dtype=np.uint8))

    # ---- K14, the given-rates form at the parent, the MRCA and the interior slot; K15, the given-rates form with cond_edge
    lay = c.set_frame(FRAME)
    nc = lay["n_codons"]
    Q = cec.dirichlet_codons(rng, (len(pairs), nc))
    for name, at, call in (("parent", [0] * len(pairs), lambda: c.given(pairs, PARENT, Q)),
                           ("mrca", [n - 1 for n in lens], lambda: c.given(pairs, MRCA, Q)),
                           ("slot", slots, lambda: c.given_at(pairs, slots, Q))):
        codons, change = call()
        for i in range(len(pairs)):
            G = G_all[i][at[i]]
            far("k14_codons_" + name, np.abs(codons[i] - nco.contraction(Q[i], G, FRAME)).max())
            far("k14_change_" + name, np.abs(change[i] - nco.change(Q[i], G, FRAME)).max())
            far("k14_sum_to_one", max(np.abs(codons[i].sum(axis=-1) - 1).max(), np.abs(change[i].sum(axis=-1) - 1).max()))
        note(fig["k14_codons_" + name] < BOUND and fig["k14_change_" + name] < BOUND, "K14 %s against the oracle" % name)
    note(fig["k14_sum_to_one"] < 1e-12, "K14: tables do not sum to 1")
    for tip in (t1, t2):
        where = [i for i, p in enumerate(pairs) if p[1] == tip]
        sub = [pairs[i] for i in where]
        res = c.given_edges(sub, tip, Q[where], want=cec.TABLES + ("cond_edge",))
        try:
            cec.rules(res, [paths[i] for i in where])
        except AssertionError as e:
            import traceback
            note(False, "K15 tip %d: sum rules: %s" % (tip, traceback.extract_tb(e.__traceback__)[-1].line))
        P = res["edge_change"].shape[1] - 1
        for k, i in enumerate(where):
            H = c.oracle_H(pairs[i][0], paths[i], tip)
            far("k15b_cond_edge", np.abs(res["cond_edge"][k, :lens[i]] - H).max())
            note(not res["cond_edge"][k, lens[i]:].any(), "K15b: padding slots of pair %d are not 0" % i)
            want = ceo.tables(Q[i], H, FRAME, P=P)
            for key in cec.TABLES:
                far("k15_" + key, np.abs(res[key][k] - want[key]).max())
            ce = res["cond_edge"][k]
            note(all(np.array_equal(ce[:, s[0]], ce[:, j]) for s in same for j in s[1:]), "K15b: sites of one pattern differ, pair %d" % i)
            one = c.given_edges([sub[k]], tip, Q[i:i + 1], want=("cond_edge", "codon_counts"))
            note(np.array_equal(one["cond_edge"][0], ce[:lens[i]]) and np.array_equal(one["codon_counts"][0], res["codon_counts"][k]),
                 "K15: pair %d alone differs from the batch" % i)
    note(all(fig[k] < BOUND for k in fig if k.startswith("k15")), "K15 against the oracle")

    # ---- K3 (lh_asr_batch): four rows against oracle/asr_oracle.py at the same sample numbers, the drawn strings equal
    if case.L in pe.K3_L and not case.mixed and R == 4:
        from tests.test_gpu_asr import _run
        mism, total, _, _ = _run(hip, c.o, [rows[0], rows[1], rows[1], rows[0]], R, K3_SEED, K3_FIRST, np.random.default_rng(3))
        fig["k3_mismatches"] = int(mism)
        premises["k3_draws"] = int(total)
        note(mism == 0, "K3: %d of %d drawn states differ from the oracle's" % (mism, total))
    ec.fam.close()
    premises["seconds"] = round(time.perf_counter() - t0, 2)
    return dict(key="%s_R%d" % (case.name, R), failures=failures, figures=fig, premises=premises)


if __name__ == "__main__":
    import linearham_amd
    from tests import pattern_edge_cases as pe
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    todo = pe.TREEPASS[int(sys.argv[1]):int(sys.argv[2])]
    print(json.dumps(dict(cases=[run_case(lib, case, R, sys.argv[3]) for case, R in todo])))
