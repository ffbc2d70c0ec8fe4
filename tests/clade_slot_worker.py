"""Helper of tests/test_gpu_clade_slot.py: one case per process, its verdict as one JSON line (failures: what did not hold;
figures: the largest deviations seen; premises: what the case claims about its own shapes).

tables    cond, log_cand and K14's tables at interior slots against the oracles and against K11 on the device.
identity  slot 0 / the last slot against node 0 / 1, rows alone and in mixed batches, the weighted sums; digests of rows alone.
cut       the 259 rows of cut_rows() in one call, under LH_CHUNK=256 and LH_ANC_PAIRS=7 (read once per process): digests.
draws     20 000 device draws read at the slot's node against two-site tables and one codon's table.
badslot   slots outside the path: the host forms' refusal, the device forms' NaN row and error word (torch first).
pipeline  --ancestral-probs-pipeline and --node-codons-pipeline with --node mrca-with:<name> on the five-row table.
ext DIR   K14 at an interior slot in extended range on the two rows of tests/clade_slot_ext_cases.py, whose references lie
          in DIR."""
import hashlib
import json
import os
import pathlib
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILY = dict(n_samples=5, seed=45)
# rows on both sides of the launch-group cut at 256, interior slots among them (254, 257); row 2's three pairs straddle a
# group of 7 pairs
CUT_N, CUT_CHECKED = 259, [0, 2, 254, 255, 256, 257, 258]


def _digest(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def _open(hip, tmp, **kw):
    from tests.clade_slot_cases import synth
    return synth(hip, pathlib.Path(tmp), **kw)


def _hip():
    import linearham_amd
    return linearham_amd.load_library()


def cut_rows(c):
    """259 (row, tip) pairs over the five tree samples with a slot each: first, last and interior slots in turn."""
    pairs, slots = [], []
    for i in range(CUT_N):
        row, tip = i % 5, 1 + (i * 3) % (c.T - 1)
        n = len(c.path(row, tip))
        s = c.pick(row, tip, "interior") if i % 3 == 2 else None
        pairs.append((row, tip))
        slots.append(s if s is not None else (0 if i % 3 == 0 else n - 1))
    return pairs, slots


def _junction_codon(lay):
    wc = lay["window_codon"]
    return int(wc[len(wc) // 2])


def tables(tmp):
    import numpy as np
    from linearham_amd import capi
    from linearham_amd import posterior as lp
    from tests import ancestral_probs_oracle as apo
    from tests import node_codon_oracle as nco
    from tests.ancestral_cases import BOUND
    from tests.clade_slot_cases import LOG_CAND_BOUND
    hip = _hip()
    failures, figures, premises = [], {}, {}

    def note(ok, text):
        if not ok:
            failures.append(text)

    def fig(name, v):
        figures[name] = max(figures.get(name, 0.0), float(v))

    def one_hot_k11(c, pairs, paths, slots):
        rows = [p[0] for p in pairs]
        a = c.args(rows)
        fam = capi.Family.borrow(c.family, c.hip)
        _, ev = fam.eval_batch(*a, want=("rates",))
        G = np.zeros((len(pairs), c.L, 5, 4))
        for b in range(5):
            q = np.zeros((len(pairs), c.L, 5))
            q[:, :, b] = 1.0
            marg, _ = fam.asr_marginals_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], q, capi.pad_paths(paths), want=("marg",))
            for i in range(len(pairs)):
                G[i, :, b] = marg[i, slots[i]]
        return G

    def cond_check(c, pairs, slots, tag):
        c.hip.set_ancestral_candidates(c.family, np.full((1, c.L), apo.OPEN))
        res, paths = c.probs_at(pairs, slots, want=("cond",))
        note(all(0 < s < len(p) - 1 for s, p in zip(slots, paths)), tag + ": a slot is not interior")
        fig(tag + "_cond_vs_k11", np.abs(res["cond"] - one_hot_k11(c, pairs, paths, slots)).max())
        fig(tag + "_cond_rowsum", np.abs(res["cond"].sum(axis=-1) - 1).max())
        for i, (row, _) in enumerate(pairs):
            fig(tag + "_cond_vs_oracle", np.abs(res["cond"][i] - c.tables_at(row, paths[i])[slots[i]]).max())
        note(figures[tag + "_cond_vs_k11"] < 1e-12 and figures[tag + "_cond_rowsum"] < 1e-12, tag + ": cond against K11 / row sums")
        note(figures[tag + "_cond_vs_oracle"] < BOUND, tag + ": cond against the oracle")
        return res, paths

    # the 17-leaf family: every tip with an interior slot, both rows
    c17 = _open(hip, os.path.join(tmp, "f17"), n_leaves=17, n_samples=2, seed=9)
    pairs17 = [(i, t) for i in range(2) for t in range(1, c17.T) if c17.pick(i, t, "interior") is not None]
    slots17 = [c17.pick(i, t, "interior") for i, t in pairs17]
    _, paths17 = cond_check(c17, pairs17, slots17, "f17")
    premises["f17"] = dict(n=len(pairs17), slots=sorted(set(slots17)), longest=max(len(p) for p in paths17))

    # the small family
    c = _open(hip, os.path.join(tmp, "f8"), **FAMILY)
    pairs, slots = c.interior_pairs(range(5))
    _, paths = cond_check(c, pairs, slots, "f8")
    premises["f8"] = dict(n=len(pairs), slots=slots, lengths=[len(p) for p in paths])
    lay = c.set_frame(0)
    nc, jc = lay["n_codons"], _junction_codon(lay)
    jsites = [3 * jc, 3 * jc + 1, 3 * jc + 2]
    k11, _ = c.run(pairs, want=("marg",))
    for i, (pair, s) in enumerate(zip(pairs, slots)):
        row, tip = pair
        whole = np.where(c.o.msa[tip - 1] < 4, c.o.msa[tip - 1], 0).astype(np.uint8)   # the seed's own sequence
        half = whole.copy()
        half[1::2] = apo.OPEN
        parts = [("v", apo.one_site(c.L, 1)), ("j", apo.one_site(c.L, jsites[1])), ("J", apo.one_site(c.L, c.L - 2)),
                 ("three", apo.constrained(c.L, jsites)), ("whole", whole[None]), ("half", half[None]),
                 ("open", np.full((1, c.L), apo.OPEN, dtype=np.uint8))]
        where, at = {}, 0
        for name, a in parts:
            where[name] = slice(at, at + len(a))
            at += len(a)
        cands = np.concatenate([a for _, a in parts])
        res, _ = c.probs_at([pair], [s], cands)
        lc = res["log_cand"][0]
        want = c.oracle_log_cand(row, c.tables_at(row, paths[i])[s], cands)
        finite = np.isfinite(want)
        note(np.array_equal(np.isfinite(lc), finite) and finite[where["three"]].any(), "log_cand: finiteness differs, row %d" % i)
        fig("log_cand_vs_oracle", np.abs(lc[finite] - want[finite]).max())
        note(lc[where["open"]][0] == 0.0, "log_cand: the all-open candidate is not exactly 0, row %d" % i)
        fig("three_sites_sum", abs(np.exp(lc[where["three"]]).sum() - 1))
        for name, site in (("v", 1), ("j", jsites[1]), ("J", c.L - 2)):
            fig("one_site_vs_k11", np.abs(np.exp(lc[where[name]]) - k11["marg"][i, s, site]).max())
    note(figures["log_cand_vs_oracle"] < LOG_CAND_BOUND, "log_cand against the oracle")
    note(figures["three_sites_sum"] < 1e-10 and figures["one_site_vs_k11"] < 1e-10, "log_cand: sums / one-site candidates")

    # K14 at the slot
    res14, _ = c.node_codons_at(pairs, slots)
    fig("k14_codons_rowsum", np.abs(res14["codons"].sum(axis=-1) - 1).max())
    fig("k14_change_rowsum", np.abs(res14["change"].sum(axis=-1) - 1).max())
    picked = [0, jc, nc - 1]
    k13, _ = c.probs_at(pairs, slots, np.concatenate([nco.triple_candidates(c.L, 0, k) for k in picked]), want=("log_cand",))
    Qo = {row: c.naive_codons(row) for row in sorted({p[0] for p in pairs})}
    for i, (pair, s) in enumerate(zip(pairs, slots)):
        for j, k in enumerate(picked):
            fig("k14_vs_k13", np.abs(np.exp(k13["log_cand"][i, 64 * j:64 * j + 64]) - res14["codons"][i, k]).max())
        fig("k14_sites_vs_k11", np.abs(nco.site_marginals(res14["codons"][i]).reshape(-1, 4) - k11["marg"][i, s, :3 * nc]).max())
        G = c.tables_at(pair[0], paths[i])[s]
        fig("k14_vs_oracle", max(np.abs(res14["codons"][i] - nco.contraction(Qo[pair[0]], G, 0)).max(),
                                 np.abs(res14["change"][i] - nco.change(Qo[pair[0]], G, 0)).max()))
    note(figures["k14_codons_rowsum"] < 1e-12 and figures["k14_change_rowsum"] < 1e-12, "K14: row sums")
    note(figures["k14_vs_k13"] < BOUND and figures["k14_vs_oracle"] < BOUND, "K14 against K13 / the oracle")
    note(figures["k14_sites_vs_k11"] < 1e-12, "K14's site marginals against K11")
    rows = [p[0] for p in pairs]
    k9 = c.hip.eval_codons_batch(c.family, *c.args(rows), want=("windows", "genes"))
    Q = np.stack([lp.codon_table(c.state_space, k9["windows"][i], k9["genes"][i], lay) for i in range(len(pairs))])
    codons, change = c.given_at(pairs, slots, Q)
    note(np.array_equal(codons, res14["codons"]) and np.array_equal(change, res14["change"]),
         "K14: the given-rates form on the evaluation's rates and K9 table does not give the evaluation form's bits")
    return dict(failures=failures, figures=figures, premises=premises)


def _mixed(c):
    """A batch of the five rows that holds slot 0, a last slot and interior ones."""
    pairs, slots = c.interior_pairs(range(5))
    lens = [len(c.path(*p)) for p in pairs]
    slots = [0, lens[1] - 1] + slots[2:]
    return pairs, slots, lens


def identity(tmp):
    import numpy as np
    from linearham_amd import posterior as lp
    from tests import ancestral_probs_worker as apw
    from tests.ancestral_probs_cases import MRCA, PARENT
    hip = _hip()
    c = _open(hip, tmp, **FAMILY)
    failures, figures, premises = [], {}, {}

    def note(ok, text):
        if not ok:
            failures.append(text)
    cands = apw.pairs_candidates(c.L)
    c.set_frame(0)
    rng = np.random.default_rng(8)
    pairs = [(i, 1 + (2 * i) % (c.T - 1)) for i in range(5)] + [(i, 1 + (2 * i + 3) % (c.T - 1)) for i in range(5)]
    off = -1000.0 + 3.0 * rng.standard_normal(len(pairs))
    lens = [len(c.path(*p)) for p in pairs]
    premises["lengths"] = lens
    w13 = ("loglik", "cond", "log_cand", "weighted_sum", "weight_stats")
    w14 = ("loglik", "codons", "change", "weighted_codons", "weighted_change", "weight_stats")
    for node, slots in ((PARENT, [0] * len(pairs)), (MRCA, [n - 1 for n in lens])):
        a, _ = c.probs(pairs, node, cands, log_offset=off, want=w13)
        b, _ = c.probs_at(pairs, slots, log_offset=off, want=w13)
        for k in w13:
            note(np.array_equal(a[k], b[k]), "K13 %s at node %d: the slot form's bits differ" % (k, node))
        a, _ = c.node_codons(pairs, node, log_offset=off, want=w14)
        b, _ = c.node_codons_at(pairs, slots, log_offset=off, want=w14)
        for k in w14:
            note(np.array_equal(a[k], b[k]), "K14 %s at node %d: the slot form's bits differ" % (k, node))
    # a row alone, in a batch of unlike slots, and second in a batch of two
    mp, ms, ml = _mixed(c)
    premises["mixed_slots"], premises["mixed_lengths"] = ms, ml
    full13, _ = c.probs_at(mp, ms, cands)
    full14, _ = c.node_codons_at(mp, ms)
    for i in range(len(mp)):
        j = (i + 1) % len(mp)
        alone13, _ = c.probs_at([mp[i]], [ms[i]])
        second13, _ = c.probs_at([mp[j], mp[i]], [ms[j], ms[i]])
        alone14, _ = c.node_codons_at([mp[i]], [ms[i]])
        second14, _ = c.node_codons_at([mp[j], mp[i]], [ms[j], ms[i]])
        for k in ("loglik", "cond", "log_cand"):
            note(np.array_equal(alone13[k][0], full13[k][i]) and np.array_equal(second13[k][1], full13[k][i]), "K13 %s row %d depends on its batch" % (k, i))
        for k in ("loglik", "codons", "change"):
            note(np.array_equal(alone14[k][0], full14[k][i]) and np.array_equal(second14[k][1], full14[k][i]), "K14 %s row %d depends on its batch" % (k, i))
    # the weighted sums over rows with unlike slots
    n = 40
    wp = [mp[i % 5] for i in range(n)]
    wslots = [ms[i % 5] if i % 2 == 0 else (i // 5) % ml[i % 5] for i in range(n)]
    woff = -1000.0 + 3.0 * rng.standard_normal(n)
    premises["weighted_slots"] = sorted(set(wslots))

    def weights(res, tables):
        lw = res["loglik"] - woff[:len(res["loglik"])]
        m = lw.max()
        w = np.exp(lw - m)
        st = res["weight_stats"]
        rel = [abs(st[1] - w.sum()) / w.sum(), abs(st[2] - (w * w).sum()) / (w * w).sum()]
        for rows_key, sum_key in tables:
            ref = np.tensordot(w.astype(np.longdouble), res[rows_key].astype(np.longdouble), axes=1).astype(np.float64)
            got = res[sum_key]
            rel.append((np.abs(got - ref) / np.where(ref != 0, np.abs(ref), 1.0)).max())
        return st[0] == m, max(rel)
    r13, _ = c.probs_at(wp, wslots, log_offset=woff, want=("loglik", "log_cand", "weighted_sum", "weight_stats"))
    r13["prob"] = np.exp(r13["log_cand"])
    ok, figures["k13_weighted_rel"] = weights(r13, [("prob", "weighted_sum")])
    note(ok and figures["k13_weighted_rel"] < 1e-12, "K13: weighted_sum / weight_stats against numpy")
    r14, _ = c.node_codons_at(wp, wslots, log_offset=woff, want=w14)
    ok, figures["k14_weighted_rel"] = weights(r14, [("codons", "weighted_codons"), ("change", "weighted_change")])
    note(ok and figures["k14_weighted_rel"] < 1e-12, "K14: weighted sums / weight_stats against numpy")
    h = 17
    a, _ = c.probs_at(wp[:h], wslots[:h], log_offset=woff[:h], want=("weighted_sum", "weight_stats"))
    b, _ = c.probs_at(wp[h:], wslots[h:], log_offset=woff[h:], want=("weighted_sum", "weight_stats"))
    mean, mx, s1, s2 = lp.combine([(a["weighted_sum"], a["weight_stats"]), (b["weighted_sum"], b["weight_stats"])])
    st = r13["weight_stats"]
    whole = r13["weighted_sum"] / st[1]
    figures["k13_combine_rel"] = float(max((np.abs(mean - whole) / np.where(whole != 0, whole, 1.0)).max(), abs(s1 - st[1]) / st[1],
                                           abs(s2 - st[2]) / st[2]))
    note(mx == st[0] and figures["k13_combine_rel"] < 1e-13, "K13: two batches combined differ from the single call")
    # the rows the cut process compares with, alone
    cp, cs = cut_rows(c)
    alone = {}
    for i in CUT_CHECKED:
        r, _ = c.probs_at([cp[i]], [cs[i]], cands)
        alone[str(i)] = {k: _digest(r[k][0]) for k in ("loglik", "cond", "log_cand")}
    premises["cut_slots"] = {str(i): cs[i] for i in CUT_CHECKED}
    return dict(failures=failures, figures=figures, premises=premises, alone=alone)


def cut(tmp):
    from linearham_amd import capi
    from tests import ancestral_probs_worker as apw
    hip = _hip()
    c = _open(hip, tmp, **FAMILY)
    cp, cs = cut_rows(c)
    capi.Family.borrow(c.family, hip).profile_enable(True)
    full, _ = c.probs_at(cp, cs, apw.pairs_candidates(c.L))
    groups = hip.ancestral_candidates_profile_read(c.family)[3]
    rows = {str(i): {k: _digest(full[k][i]) for k in ("loglik", "cond", "log_cand")} for i in CUT_CHECKED}
    return dict(n=len(cp), groups=int(groups), distinct_slots=sorted(set(cs)), rows=rows)


def draws(tmp):
    import numpy as np
    from linearham_amd import capi
    from tests import ancestral_probs_oracle as apo
    from tests.test_gpu_ancestral_probs import _sample_states
    hip = _hip()
    c = _open(hip, tmp, **FAMILY)
    failures, premises = [], {}
    pairs, slots = c.interior_pairs([1])
    (row, tip), s = pairs[0], slots[0]
    path = c.path(row, tip)
    premises.update(slot=s, length=len(path))
    N = 20000
    T, depth, ops, brl, er, pi, alpha, R = c.args([row])
    rep = lambda a: np.ascontiguousarray(np.repeat(np.asarray(a), N, axis=0))
    fam = capi.Family.borrow(c.family, hip)
    _, ev = fam.eval_batch(T, depth, ops, brl, er, pi, alpha, R, want=("rates",))
    states = _sample_states(hip, c.family, T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(alpha), R, 5)
    naive, _ = hip.naive_sequences(c.family, states)
    anc, _ = fam.asr_batch(T, depth, rep(ops), rep(brl), rep(er), rep(pi), rep(ev["rates"]), naive, 23, 0)
    seqs = anc[:, path[s] - T]
    lay = c.set_frame(0)
    jc = _junction_codon(lay)
    pairs_of_sites = ((3 * jc, 3 * jc + 1), (1, c.L - 2))
    res, _ = c.probs_at([(row, tip)], [s], np.concatenate([apo.constrained(c.L, list(p)) for p in pairs_of_sites]), want=("log_cand",))
    worst = 0.0
    for k, (a, b) in enumerate(pairs_of_sites):
        p = np.exp(res["log_cand"][0, 16 * k:16 * k + 16]).reshape(4, 4)
        freq = np.zeros((4, 4))
        np.add.at(freq, (seqs[:, a], seqs[:, b]), 1.0 / N)
        room = 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N
        worst = max(worst, (np.abs(freq - p) / room).max())
        if abs(p.sum() - 1) > 1e-10 or (np.abs(freq - p) > room).any():
            failures.append("two-site table of sites %d, %d" % (a, b))
    r14, _ = c.node_codons_at([(row, tip)], [s], want=("codons",))
    p = r14["codons"][0, jc]
    freq = np.zeros(64)
    np.add.at(freq, 16 * seqs[:, 3 * jc].astype(int) + 4 * seqs[:, 3 * jc + 1] + seqs[:, 3 * jc + 2], 1.0 / N)
    room = 5 * np.sqrt(p * (1 - p) / N) + 1.0 / N
    worst = max(worst, (np.abs(freq - p) / room).max())
    if (np.abs(freq - p) > room).any():
        failures.append("the table of codon %d" % jc)
    return dict(failures=failures, figures=dict(worst_share_of_the_room=float(worst)), premises=premises)


def badslot(tmp):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    from linearham_amd import capi
    from tests import ancestral_probs_worker as apw
    hip = _hip()
    c = _open(hip, tmp, **FAMILY)
    fam = capi.Family.borrow(c.family, hip)
    failures = []

    def note(ok, text):
        if not ok:
            failures.append(text)
    cands = apw.pairs_candidates(c.L)
    K = len(cands)
    pairs, slots, lens = _mixed(c)
    n, victim = len(pairs), 2          # (a path shorter than the batch's P: its length and P are two bad slots)
    lay = c.set_frame(0)
    nc = lay["n_codons"]
    host13, paths = c.probs_at(pairs, slots, cands, want=("loglik", "cond", "log_cand", "weighted_sum", "weight_stats"))
    host14, _ = c.node_codons_at(pairs, slots, want=("loglik", "codons", "change", "weighted_codons", "weight_stats"))
    P = max(lens)
    bad_values = [-1, lens[victim], P]
    # the host forms refuse, naming the row
    Q = np.full((n, nc, 125), 1.0 / 125)
    for v in bad_values:
        bad = list(slots)
        bad[victim] = v
        for name, call in (("K13", lambda: c.probs_at(pairs, bad)), ("K14", lambda: c.node_codons_at(pairs, bad)),
                           ("K14 given", lambda: c.given_at(pairs, bad, Q))):
            try:
                call()
                failures.append("%s: slot %d was not refused" % (name, v))
            except RuntimeError as e:
                note("slot %d of sample %d lies outside" % (v, victim) in str(e), "%s: slot %d: %s" % (name, v, e))
    # the device forms
    rows = [p[0] for p in pairs]
    T, depth, ops, brl, er, pi, alpha, R = c.args(rows)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    d = [t(ops, np.int32), t(brl, np.float64), t(er, np.float64), t(pi, np.float64), t(alpha, np.float64),
         t(capi.pad_paths(paths), np.int32)]

    def status():
        try:
            fam.status()
        except RuntimeError as e:
            return str(e)
        return ""

    def run13(slot_list):
        sl = t(slot_list, np.int32)
        outs = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev),
                "cond": torch.full((n, c.L, 5, 4), 7.0, dtype=torch.float64, device=dev),
                "log_cand": torch.full((n, K), 7.0, dtype=torch.float64, device=dev),
                "weighted_sum": torch.zeros(K, dtype=torch.float64, device=dev),
                "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_ancestral_candidates_at_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                          d[3].data_ptr(), d[4].data_ptr(), R, d[5].data_ptr(), P, sl.data_ptr(),
                                                          {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
        st = status()
        return {k: v.cpu().numpy() for k, v in outs.items()}, st, status()

    def run14(slot_list):
        sl = t(slot_list, np.int32)
        outs = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev),
                "codons": torch.full((n, nc, 64), 7.0, dtype=torch.float64, device=dev),
                "change": torch.full((n, nc, 4), 7.0, dtype=torch.float64, device=dev),
                "weighted_codons": torch.zeros((nc, 64), dtype=torch.float64, device=dev),
                "weight_stats": torch.zeros(3, dtype=torch.float64, device=dev)}
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            hip.eval_node_codons_at_batch_device(c.family, n, T, depth, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                 d[3].data_ptr(), d[4].data_ptr(), R, d[5].data_ptr(), P, sl.data_ptr(),
                                                 {k: v.data_ptr() for k, v in outs.items()}, stream.cuda_stream)
        st = status()
        return {k: v.cpu().numpy() for k, v in outs.items()}, st, status()
    keep = [i for i in range(n) if i != victim]
    for name, run, host, tabs, wkey, rowkey in (("K13", run13, host13, ("cond", "log_cand"), "weighted_sum", "log_cand"),
                                                ("K14", run14, host14, ("codons", "change"), "weighted_codons", "codons")):
        clean, st, _ = run(slots)
        note(st == "" and all(np.array_equal(clean[k], host[k]) for k in host), name + ": the device form differs from the host form")
        for v in bad_values:
            bad = list(slots)
            bad[victim] = v
            o, st, st2 = run(bad)
            note("slot of sample %d lies outside" % victim in st and "not a chain" not in st and st2 == "",
                 "%s slot %d: status %r then %r" % (name, v, st, st2))
            note(all(np.isnan(o[k][victim]).all() for k in tabs), "%s slot %d: the row is not NaN" % (name, v))
            note(all(np.array_equal(o[k][i], clean[k][i]) for i in keep for k in tabs), "%s slot %d: another row changed" % (name, v))
            lw = o["loglik"][keep]
            w = np.exp(lw - lw.max())
            vals = np.exp(o[rowkey][keep]) if rowkey == "log_cand" else o[rowkey][keep]
            ref = np.tensordot(w, vals, axes=1)
            note(np.allclose(o[wkey], ref, rtol=1e-13, atol=1e-300) and abs(o["weight_stats"][1] - w.sum()) < 1e-13 * w.sum(),
                 "%s slot %d: the row carries weight" % (name, v))
    return dict(failures=failures, premises=dict(slots=slots, lengths=lens, bad=bad_values))


def pipeline(tmp):
    import subprocess
    import numpy as np
    from linearham_amd import capi, host
    from tests import ancestral_probs_oracle as apo
    from tests.clade_slot_cases import AtCase
    from tools import synth_family as sf
    hip = _hip()
    failures, figures, premises = [], {}, {}

    def note(ok, text):
        if not ok:
            failures.append(text)
    out = os.path.join(tmp, "fam")
    sf.generate(sf.Spec.small(**FAMILY), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    rows = sf.read_trees_tsv(tsv)
    c = AtCase(hip, yaml_path, pdir, rows, 4, pathlib.Path(tmp))
    labels = list(c.o.xmsa_labels)
    n = len(rows)
    # on the CPU: a seed with a partner whose common ancestor is interior in every row, and one across the root in every row
    # (the root may take two partners: the node is then the higher of their two common ancestors with the seed)
    import itertools
    choice = None
    for tip in range(1, c.T):
        part = [c.partners(i, tip) for i in range(n)]
        lens = [len(c.path(i, tip)) for i in range(n)]
        inner = [u for u in part[0] if all(0 < part[i][u] < lens[i] - 1 for i in range(n))]
        sets = [(u,) for u in part[0]] + list(itertools.combinations(part[0], 2))
        top = [q for q in sets if all(max(part[i][u] for u in q) == lens[i] - 1 for i in range(n))]
        if inner and top:
            inner.sort(key=lambda u: -len({part[i][u] for i in range(n)}))
            choice = (tip, inner[0], list(top[0]), [part[i][inner[0]] for i in range(n)], lens)
            break
    assert choice, "no seed of this family has both kinds of partner"
    tip, inner, top, slots, lens = choice
    premises.update(seed_tip=tip, partner=inner, root_partners=top, slots=slots, lengths=lens)
    top_node = "mrca-with:" + ",".join(labels[u] for u in top)
    seed_seq, exe = labels[tip], os.path.join(os.path.dirname(host.host_library_path()), "linearham")
    L = c.L
    cands = np.concatenate([apo.constrained(L, [2, L // 2]), apo.one_site(L, 5),
                            np.where(c.o.msa[tip - 1] < 4, c.o.msa[tip - 1], 0).astype(np.uint8)[None]])
    names = ["cand%d" % k for k in range(len(cands))]
    text = ["".join("ACGTN"[x] for x in row) for row in cands]
    fasta = os.path.join(tmp, "cands.fa")
    open(fasta, "w").write("".join(">%s\n%s\n" % (a, q) for a, q in zip(names, text)))
    common = ["--yaml-path", yaml_path, "--cluster-ind", "0", "--hmm-param-dir", pdir, "--num-rates", "4", "--seed-seq", seed_seq]

    def cli(sub, node, prefix, table=tsv, env=None, extra=()):
        r = subprocess.run([exe, sub, "--input-path", table, "--output-path", os.path.join(tmp, prefix), "--node", node] + common +
                           list(extra), capture_output=True, text=True, timeout=200, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, r.stderr[-2000:]
        return os.path.join(tmp, prefix)

    def same(a, b, exts):
        return [e for e in exts if open(a + "." + e, "rb").read() != open(b + "." + e, "rb").read()]
    node = "mrca-with:" + labels[inner]
    pairs = [(i, tip) for i in range(n)]
    # K13
    ext13 = ("probs.tsv", "rows.tsv", "summary.tsv")
    p2 = cli("--ancestral-probs-pipeline", node, "p2", env={"LH_PIPELINE_BATCH": "2"}, extra=["--candidates", fasta])
    p4 = cli("--ancestral-probs-pipeline", node, "p4", env={"LH_PIPELINE_BATCH": "4"}, extra=["--candidates", fasta])
    note(same(p2, p4, ext13) == [], "K13: the files depend on LH_PIPELINE_BATCH: %s" % same(p2, p4, ext13))
    got = host.read_ancestral_probs(p2)
    res, _ = c.probs_at(pairs, slots, cands, want=("loglik", "log_cand"))
    lw = res["loglik"] - np.array([r["likelihood"] for r in rows])
    w = np.exp(lw - lw.max())
    want = np.tensordot(w, np.exp(res["log_cand"]), axes=1) / w.sum()
    byname = dict(zip(got["names"], got["prob"]))
    figures["k13_vs_python"] = float(max(abs(byname[a] - want[k]) / max(want[k], 1e-300) for k, a in enumerate(names)))
    note(figures["k13_vs_python"] < 1e-12, "K13: the pipeline's table differs from the Python route")
    note([r[3] for r in got["rows"]] == slots and [r[2] for r in got["rows"]] == lens, "K13: rows.tsv's slots or lengths: %s" % got["rows"])
    note(np.allclose([r[1] for r in got["rows"]], w, rtol=1e-9), "K13: rows.tsv's weights")
    sm = got["summary"]
    note(sm.get("node") == node and sm.get("slot_min") == min(slots) and sm.get("slot_max") == max(slots), "K13: summary %s" % sm)
    lib = c.hh.run_ancestral_probs_pipeline(tsv, seed_seq, node, fasta, os.path.join(tmp, "lib13"), 4)
    note(same(p2, os.path.join(tmp, "lib13"), ext13) == [], "K13: the library's files differ from the program's")
    del lib
    at_root = cli("--ancestral-probs-pipeline", top_node, "pr", extra=["--candidates", fasta])
    mrca = cli("--ancestral-probs-pipeline", "mrca", "pm", extra=["--candidates", fasta])
    note(same(at_root, mrca, ("probs.tsv",)) == [], "K13: a partner across the root does not give --node mrca's probs.tsv")
    rows_m = open(mrca + ".rows.tsv").read().split("\n")[0]
    note(rows_m == "row\tweight\tchain_length" and "node" not in open(mrca + ".summary.tsv").read(), "K13: --node mrca's files changed")
    # K14
    ext14 = ("codons.tsv", "aa.tsv", "changes.tsv", "rows.tsv", "summary.tsv")
    c2 = cli("--node-codons-pipeline", node, "c2", env={"LH_PIPELINE_BATCH": "2"}, extra=["--frame", "1"])
    c4 = cli("--node-codons-pipeline", node, "c4", env={"LH_PIPELINE_BATCH": "4"}, extra=["--frame", "1"])
    note(same(c2, c4, ext14) == [], "K14: the files depend on LH_PIPELINE_BATCH: %s" % same(c2, c4, ext14))
    got = host.read_node_codons(c2)
    c.set_frame(1)
    r14, _ = c.node_codons_at(pairs, slots)
    for key in ("codons", "change"):
        want = np.tensordot(w, r14[key], axes=1) / w.sum()
        figures["k14_%s_vs_python" % key] = float(np.abs(got[key] - want).max())
        note(figures["k14_%s_vs_python" % key] < 1e-12, "K14: %s differs from the Python route" % key)
    note([r[3] for r in got["rows"]] == slots, "K14: rows.tsv's slots")
    sm = got["summary"]
    note(sm.get("node") == node and sm.get("slot_min") == min(slots) and sm.get("slot_max") == max(slots) and sm.get("frame") == 1,
         "K14: summary %s" % sm)
    at_root = cli("--node-codons-pipeline", top_node, "cr", extra=["--frame", "1"])
    mrca = cli("--node-codons-pipeline", "mrca", "cm", extra=["--frame", "1"])
    note(same(at_root, mrca, ext14[:3]) == [], "K14: a partner across the root does not give --node mrca's tables")
    # one row: the single-tree commands give the pipeline's numbers
    one = os.path.join(tmp, "one.tsv")
    lines = open(tsv).read().split("\n")
    open(one, "w").write("\n".join(lines[:2]) + "\n")
    row = rows[0]
    newick = os.path.join(tmp, "row0.tree")
    open(newick, "w").write(row["tree"] + "\n")
    model = ["--newick-path", newick, "--alpha", repr(row["alpha"])] + sum([["--er", repr(x)] for x in row["er"]], []) + \
        sum([["--pi", repr(x)] for x in row["pi"]], [])
    p1 = host.read_ancestral_probs(cli("--ancestral-probs-pipeline", node, "p1", table=one, extra=["--candidates", fasta]))
    r = subprocess.run([exe, "--ancestral-probs", "--node", node, "--candidates", fasta] + common + model, capture_output=True,
                       text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    single = {ln.split("\t")[0]: float(ln.split("\t")[2]) for ln in r.stdout.strip().split("\n")[1:]}
    pipe = dict(zip(p1["names"], p1["prob"]))
    figures["k13_single_vs_pipeline"] = float(max(abs(single[a] - pipe[a]) / max(pipe[a], 1e-300) for a in names))
    note(figures["k13_single_vs_pipeline"] < 1e-14, "K13: --ancestral-probs differs from the one-row pipeline")
    c.hh.initialize_phylo_parameters(row["tree"], row["er"], row["pi"], row["alpha"], 4, is_path=False)
    one13 = c.hh.ancestral_candidate_posterior(seed_seq, node, text)
    note(one13["node"] == c.path(0, tip)[slots[0]], "K13: the library's node id")
    c1 = host.read_node_codons(cli("--node-codons-pipeline", node, "c1", table=one, extra=["--frame", "1"]))
    r = subprocess.run([exe, "--node-codons", "--node", node, "--frame", "1"] + common + model, capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    single = host.parse_node_codons(r.stdout)
    figures["k14_single_vs_pipeline"] = float(max(np.abs(single[k] - c1[k]).max() for k in ("codons", "change")))
    note(figures["k14_single_vs_pipeline"] < 1e-14, "K14: --node-codons differs from the one-row pipeline")
    one14 = c.hh.node_codon_marginals(seed_seq, node, frame=1)
    note(one14["node"] == c.path(0, tip)[slots[0]] and np.abs(one14["codons"] - r14["codons"][0]).max() < 1e-14,
         "K14: the library's single-tree tables")
    return dict(failures=failures, figures=figures, premises=premises)


def ext(tmp, out_dir):
    import numpy as np
    from linearham_amd import capi, host
    from tests import cadence_cases as cc
    from tests import clade_slot_ext_cases as xe
    from tests import ext_deep_cases as xd
    from tests.ancestral_cases import write_table
    hip = _hip()
    failures, figures = [], {}

    def note(ok, text):
        if not ok:
            failures.append(text)
    meta = json.load(open(os.path.join(out_dir, "clade_slot_ext.json")))
    family, frame, tip, slots = meta["family"], meta["frame"], meta["seed_tip"], meta["slots"]
    h = cc.load_family(family, tmp)
    samples = [cc.sample_of(r)[0] for r in xe.rows()]
    sched = [cc.schedule(h, s) for s in samples]
    R, T, depth = cc.FAMILIES[family]["R"], sched[0][0], max(s[5] for s in sched)
    a = (T, depth, np.stack([s[4] for s in sched]), np.stack([s[3] for s in sched]), np.array([s["er"] for s in samples]),
         np.array([s["pi"] for s in samples]), np.array([s["alpha"] for s in samples]), R)
    yaml_path, pdir = cc.write_family_files(family, tmp, h)
    hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
    tsv = os.path.join(tmp, "rows.tsv")
    write_table(tsv, samples[:1])
    hfam = hh.flatten_tsv(tsv, 1)["family"]
    fam = capi.Family.borrow(hfam, hip)
    hip.set_codons(hfam, frame)
    paths = [capi.seed_path(T, s[1], s[2], tip) for s in sched]
    note(all(0 < s < len(p) - 1 for s, p in zip(slots, paths)), "a slot is not interior under the device's own paths")
    padded = capi.pad_paths(paths)
    want = ("loglik", "codons", "change")
    plain = hip.eval_node_codons_at_batch(hfam, *a, padded, slots, want=want)
    default_finite = [bool(np.isfinite(x)) for x in plain["loglik"]]
    hh.set_extended_range(True)
    fam.set_extended_range(True)
    res = hip.eval_node_codons_at_batch(hfam, *a, padded, slots, want=want)
    for i, name in enumerate(meta["rows"]):
        ref = np.load(os.path.join(out_dir, "clade_slot_ext_%s.npz" % name))
        for k in ("codons", "change"):
            far = float(np.abs(res[k][i] - ref[k]).max()) if np.isfinite(res[k][i]).all() else float("inf")
            figures["%s_%s" % (name, k)] = far
            figures["%s_%s_bound" % (name, k)] = xd.bound(meta["d_ref"][name][k])
            note(far <= xd.bound(meta["d_ref"][name][k]), "%s %s: %.3g from the exact contraction, bound %.3g" %
                 (name, k, far, xd.bound(meta["d_ref"][name][k])))
            figures["%s_%s_rowsum" % (name, k)] = float(np.abs(res[k][i].sum(axis=-1) - 1).max())
            note(figures["%s_%s_rowsum" % (name, k)] < 1e-12, "%s %s: rows do not sum to 1" % (name, k))
    # the end slots in this mode: the bits of the two fixed nodes
    for node, ends in ((capi.NODE_PARENT, [0] * len(paths)), (capi.NODE_MRCA, [len(p) - 1 for p in paths])):
        x = hip.eval_node_codons_batch(hfam, *a, padded, node, want=want)
        y = hip.eval_node_codons_at_batch(hfam, *a, padded, ends, want=want)
        note(all(np.array_equal(x[k], y[k]) for k in want), "extended range: the end slot differs from node %d" % node)
    return dict(failures=failures, figures=figures, premises=dict(default_finite=default_finite, slots=slots,
                                                                  lengths=[len(p) for p in paths]))


MODES = {"tables": tables, "identity": identity, "cut": cut, "draws": draws, "badslot": badslot, "pipeline": pipeline}

if __name__ == "__main__":
    tmp = tempfile.mkdtemp(prefix="lh_clade_")
    try:
        if sys.argv[1] == "tables":
            os.makedirs(os.path.join(tmp, "f17")), os.makedirs(os.path.join(tmp, "f8"))
        print(json.dumps(ext(tmp, sys.argv[2]) if sys.argv[1] == "ext" else MODES[sys.argv[1]](tmp)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
