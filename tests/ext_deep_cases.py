"""TEST INFRASTRUCTURE (CPU only): rows on which the default mode underflows and the posteriors are SPREAD, and references
for everything that reads the extended-range forward arrays and K1's (value, 2^-256 count) columns afterwards.

tests/cadence_cases.py's deep rows (alpha = 0.005) are the hard ones for K1 and for RatePlanes, but their posteriors are
one-hot: the live category's rate is 3.5e-61, a naive-base mismatch costs 2^-214 and the HMM is deterministic given the
alignment -- a subtly wrong smoothing kernel gives the same table as a right one.  With alpha = 1 (R = 2) and every branch of
the row's tree times 0.05 to 0.2 the deep columns still fall below 2^-1074 (0 in the default mode), the per-site counts
floor(-max_b log2 E / 256) differ from site to site (0 or 1 on ordinary sites, 4 to 14 on the deep ones) and the posteriors
are spread (check_row).  Rows:
  spread   SPREAD: cad190 tree B at 0.05 and 0.2, tree A at 0.1, cmp180 tree C at 0.1
  hard     lossy_long, zeroed_cherries, compound_lossy, compound_zeroed as they are in cadence_cases.ROWS
  control  control_b, compound_control: finite in the default mode

References (build_row), all on the references alone, never on the device.  Every path emits each site once, so one integer
k_t per site (cadence_cases.site_shifts) moves no posterior; on E 2^k_t, in doubles:
  alpha_rows          the forward rows, each normalised by its own sum (posterior_oracle.forward_backward's recursion, which
                      shares nothing with ScaleMatrix), in the shape of the oracle's *_forward members
  state posteriors    posterior_oracle.forward_backward; posterior_oracle.smoothing(h, forward=alpha) must equal it to 1e-12
  Q per frame         codon_oracle.dense(h, frame, forward=alpha); its site marginals must equal site_base to 1e-12
  events              events_oracle.dense with the alpha rows installed as the forward members
  Viterbi             viterbi_oracle.viterbi, log_path - ln 2 sum k_t
  log-likelihood      cadence_cases.mp_loglik (mpmath, no scaling)
  lineage tables      exact_lineage_oracle.ExactLineage as lineage_cadence_worker builds it, mixed with the row's own reference
                      site_base (exact_lineage_oracle.mix) and contracted with its reference Q (node_codon_oracle,
                      codon_edge_oracle)
and the pins (pin_row): P(naive base of site t = b | data) = exp(mp_loglik(E, every other column of site t at 0) -
mp_loglik(E)) -- an mpmath value that uses no backward pass at all --, the same with three sites clamped for one codon of Q
per frame, and with every other allele of a set switched off for the gene posteriors.  d_ref, the largest difference per
table, is stored with the row; a device bound is max(1e-10, 8 d_ref)."""
import json
import math
import os

import numpy as np

from tests import cadence_cases as cc

SHORT = cc.SHORT
SPREAD = [
    ("spread_b05", "cad190", "spread", "B", 1.0, None, SHORT, 0.05),
    ("spread_a10", "cad190", "spread", "A", 1.0, None, SHORT, 0.1),
    ("spread_c10", "cmp180", "spread", "C", 1.0, None, SHORT, 0.1),
    ("spread_b20", "cad190", "spread", "B", 1.0, None, SHORT, 0.2),
]
HARD = ("lossy_long", "zeroed_cherries", "compound_lossy", "compound_zeroed")
CONTROL = ("control_b", "compound_control")
FAMILIES = ("cad190", "cmp180")
FULL_PIN = ("spread_b05", "spread_c10")          # one spread row per family: every site and base, and one codon of Q per frame
FLOOR = 1e-10
K4_SEED = 2701
K4_MARGIN = 1e-7
K11_TABLES = ("marg", "rate_post")
K12_TABLES = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")
K15_TABLES = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")
K14_TABLES = ("codons", "change")


def kind_of(row):
    return "control" if row[0] in CONTROL else "spread" if row[2] == "spread" else "hard"


def rows_of(family):
    """The family's rows in the order of the device call: control and deep rows alternating (the control row again where the
    deep rows outnumber it), so that wave mates differ in their counts."""
    by = {r[0]: r for r in cc.ROWS}
    ctrl = [by[n] for n in CONTROL if by[n][1] == family]
    deep = [r for r in SPREAD if r[1] == family] + [by[n] for n in HARD if by[n][1] == family]
    assert len(ctrl) == 1
    out = []
    for r in deep:
        out += [ctrl[0], r]
    return out


def distinct_rows(family):
    seen, out = set(), []
    for r in rows_of(family):
        if r[0] not in seen:
            seen.add(r[0])
            out.append(r)
    return out


def combos_of(row):
    """(seed tip number, frame) of the row's lineage tables: lineage_cadence_worker.COMBOS on the hard rows, the first seed
    tip in frame 0 on the rest."""
    from tests import lineage_cadence_worker as lw
    return lw.COMBOS if kind_of(row) == "hard" else ((0, 0),)


def lw_combos():
    """Every (seed tip number, frame) some row has lineage tables for."""
    from tests import lineage_cadence_worker as lw
    return lw.COMBOS


def alpha_rows(h):
    """The forward rows of the emissions on `h`, each normalised by its own sum, as {vgerm_forward, vd_junction_forward, ...}:
    what posterior_oracle.forward_backward computes and does not return."""
    from tests import posterior_oracle as po
    out, prev = {}, None
    for name, i, e, T in po._rows(*po._chain(h)):
        a = e.copy() if T is None else (prev @ T) * e
        prev = a / a.sum()
        if i is None:
            out[name + "_forward"] = prev
        else:
            out.setdefault(name + "_forward", []).append(prev)
    return {k: np.array(v) for k, v in out.items()}


def k4_words(h, name):
    """The row's engine words for K4: a fixed stream per row name (K4_SEED + the name's bytes)."""
    from tests import k4_draw_cases as k4
    rng = np.random.default_rng([K4_SEED] + list(name.encode()))
    return rng.integers(0, 2 ** 32, k4.words_per_sample(h), dtype=np.uint64).astype(np.uint32)


def k4_reference(h, alpha, words):
    """(states of the oracle's dense draws on the reference alpha rows, the smallest relative distance of a uniform from a
    partial sum at which the answer changes): a row whose margin exceeds K4_MARGIN must draw these states on the device."""
    from tests import k4_draw_cases as k4
    st, used, draws = k4.draws_on_forward(h, alpha, words, record=True)
    assert used == len(words), (used, len(words))
    return st, float(min(k4.margin(d) for d in draws))


def site_counts(k):
    """floor(-max_b log2 E / 256) per site from site_shifts' k_t = -ceil(max_b log2 E)."""
    return np.maximum(np.asarray(k), 0) // 256      # (a site of all-N tips has log2 E = 0 within rounding, on either side)


def _far(a, b):
    with np.errstate(invalid="ignore"):
        return float(np.abs(np.asarray(a) - np.asarray(b)).max()) if np.isfinite(a).all() and np.isfinite(b).all() else float("inf")


def references(h, l2):
    """The double-precision references of a row from its exact emissions l2 (log2 per xMSA column); leaves the shifted
    emissions and the alpha rows on `h`."""
    from tests import codon_oracle as co
    from tests import events_oracle as eo
    from tests import posterior_oracle as po
    from tests import viterbi_oracle as vo
    site, k, shifted = cc.site_shifts(h, l2)
    ec = vo.set_emissions(h, np.exp2(shifted))
    post, lls = po.forward_backward(h, ec)
    alpha = alpha_rows(h)
    sm = po.smoothing(h, forward=alpha)
    ref = dict(k=k, counts=site_counts(k), alpha=alpha, post=post, ec=ec,
               d_smoothing=max(_far(sm[r], post[r]) for r in post),
               ll_fb=float(np.mean(lls)) - cc.LN2 * float(k.sum()), ll_fb_spread=float(np.ptp(lls)))
    ref["compact"] = po.to_compact(h, post)
    ref["site_base"] = po.site_base(h, post)
    ref["genes"] = po.gene_posteriors(h, post)
    for f in (0, 1, 2):
        table, _ = co.dense(h, f, forward=alpha)
        ref["Q%d" % f] = table
    L = h.msa.shape[1]
    from linearham_amd import posterior as lp
    ref["d_q_sites"] = max(_far(lp.codon_site_base(ref["Q%d" % f], f, L)[f:f + 3 * ((L - f) // 3)],
                                ref["site_base"][f:f + 3 * ((L - f) // 3)]) for f in (0, 1, 2))
    for key, v in alpha.items():
        setattr(h, key, v)
    ref["events"] = eo.flat(eo.dense(h, post))
    v = vo.viterbi(h, ec)
    ref["viterbi_states"] = vo.to_states(h, v["path"])
    ref["viterbi_log_path"] = v["log_path"] - cc.LN2 * float(k.sum())
    ref["viterbi_margin"] = v["margin"]
    return ref


def clamp(h, l2, sites_bases):
    """l2 with every column of the given sites other than the (site, base) pairs' own set to 2^-inf; None where a pair has no
    column (no state writes that base there: its posterior is 0)."""
    out = np.array(l2, dtype=float)
    site = cc.kc.column_sites(h)
    for t, b in sites_bases:
        if (int(b), int(t)) not in h.xmsa_ids:
            return None
        keep = h.xmsa_ids[(int(b), int(t))]
        cols = np.nonzero(site == t)[0]
        out[cols[cols != keep]] = -np.inf
    return out


def pin_row(h, l2, ref, full, family):
    """The mpmath pins of site_base, of one codon of Q per frame (full rows) and of the gene posteriors.  Returns d_ref per
    table and how many clamped sweeps went into each."""
    ll = cc.mp_loglik(h, l2)
    L = h.msa.shape[1]
    deep = cc.deep_sites(family)
    sites = list(range(L)) if full else sorted(set(deep) | set(np.linspace(0, L - 1, 6).astype(int).tolist()))

    def ratio(em):
        return 0.0 if em is None else math.exp(cc.mp_loglik(h, em) - ll)
    out = dict(n_site_sweeps=0, n_q_sweeps=0, n_gene_sweeps=0, site_base=0.0, Q=0.0, genes=0.0)
    for t in sites:
        for b in range(5):
            em = clamp(h, l2, [(t, b)])
            out["n_site_sweeps"] += em is not None
            out["site_base"] = max(out["site_base"], abs(ratio(em) - ref["site_base"][t, b]))
    if full:
        for f in (0, 1, 2):
            c = next(c for c in range((L - f) // 3) if any(f + 3 * c <= t < f + 3 * c + 3 for t in deep) and
                     ((ref["Q%d" % f][c] > 0.01) & (ref["Q%d" % f][c] < 0.99)).any())
            row, big = ref["Q%d" % f][c], 0.0

            def entry(e):
                b = (e // 25, (e // 5) % 5, e % 5)
                em = clamp(h, l2, [(f + 3 * c + o, b[o]) for o in range(3)])
                out["n_q_sweeps"] += em is not None
                return ratio(em)
            for e in np.nonzero(row > 1e-6)[0]:
                got = entry(int(e))
                big += got
                out["Q"] = max(out["Q"], abs(got - row[e]))
            # the entries at or below 1e-6: below 1e-6 in mpmath as well -- together they hold what the others leave of 1;
            # where that is not below 1e-6 itself, each one's own clamp
            if 1.0 - big >= 1e-6:
                for e in np.nonzero(row <= 1e-6)[0]:
                    got = entry(int(e))
                    assert got <= 1e-6, (f, c, int(e), got)
                    out["Q"] = max(out["Q"], abs(got - row[e]))
    # genes: every other allele of the set switched off -- V through gene_prob, D and J through the transition into the set
    names = {"V": sorted(h.vgerm.ggene_ranges), "D": sorted(h.dgerm.ggene_ranges), "J": sorted(h.jgerm.ggene_ranges)}
    for seg, genes in names.items():
        for g, name in enumerate(genes):
            if seg == "V":
                saved = {n: h.ggenes[n].gene_prob for n in genes}
                for n in genes:
                    if n != name:
                        h.ggenes[n].gene_prob = 0.0
            else:
                key = "vd_junction_dgerm_transition" if seg == "D" else "dj_junction_jgerm_transition"
                saved = getattr(h, key)
                T = saved.copy()
                T[:, [i for i in range(len(genes)) if i != g]] = 0.0
                setattr(h, key, T)
            try:
                got = math.exp(cc.mp_loglik(h, l2) - ll)
            finally:
                if seg == "V":
                    for n in genes:
                        h.ggenes[n].gene_prob = saved[n]
                else:
                    setattr(h, key, saved)
            out["n_gene_sweeps"] += 1
            out["genes"] = max(out["genes"], abs(got - ref["genes"][seg][name]))
    out["loglik"] = ll
    return out


def lineage_references(family, row, ref):
    """The exact lineage tables of the row's seed tips mixed with the reference site_base and contracted with the reference Q,
    and their d_ref (the double-precision oracles of tests/lineage_cadence_worker.py on the same q and Q)."""
    from tests import ancestral_marginal_oracle as amo
    from tests import ancestral_probs_oracle as apo
    from tests import codon_edge_oracle as ceo
    from tests import edge_oracle as eo
    from tests import exact_lineage_oracle as xl
    from tests import lineage_cadence_worker as lw
    from tests import node_codon_oracle as nco
    s = lw._row_setup(family, row)
    sample, T, children, root, brlen, rates, msa, lin, pre = (s[k] for k in ("sample", "T", "children", "root", "brlen", "rates",
                                                                            "msa", "lin", "pre"))
    q = ref["site_base"]
    keep, d_ref = {"rates": np.asarray(rates, dtype=float)}, {}
    combos = combos_of(row)
    for si in sorted({c[0] for c in combos}):
        tip = lw.SEEDS[family][si]
        path = amo.seed_path(children, root, T, tip)
        tab = lin.tables(path, tip)
        want = xl.mix(tab, q)
        with np.errstate(all="ignore"):
            marg, rp = amo.marginals(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, pre=pre)
            ed = eo.edges(children, root, brlen, T, msa, q, sample["er"], sample["pi"], rates, path, tip, pre=pre)
            H = ceo.cond_edges(children, root, brlen, T, msa, sample["er"], sample["pi"], rates, path, tip, pre=pre)
            G = {node: apo.cond_tables(children, root, brlen, T, msa, sample["er"], sample["pi"], rates, path,
                                       apo.PARENT if slot == 0 else apo.MRCA, pre=pre)
                 for node, slot in (("parent", 0), ("mrca", len(path) - 1))}
        d = {"k11_marg": _far(marg, want["marg"]), "k11_rate_post": _far(rp, want["rate_post"])}
        keep["k11_%d_marg" % si], keep["k11_%d_rate_post" % si] = want["marg"], want["rate_post"]
        for k in K12_TABLES:
            keep["k12_%d_%s" % (si, k)] = want[k]
            d["k12_" + k] = _far(ed[k], want[k])
        for frame in [f for i, f in combos if i == si]:
            Q = ref["Q%d" % frame]
            with np.errstate(all="ignore"):
                w15, dbl = ceo.tables(Q, tab["cond_edge"], frame), ceo.tables(Q, H, frame)
            for k in K15_TABLES:
                keep["k15_%d_%d_%s" % (si, frame, k)] = w15[k]
                d["k15_%d_%s" % (frame, k)] = _far(dbl[k], w15[k])
            for node, slot in (("parent", 0), ("mrca", len(path) - 1)):
                for k, f in (("codons", nco.contraction), ("change", nco.change)):
                    w14 = f(Q, tab["cond"][slot], frame)
                    keep["k14_%d_%d_%s_%s" % (si, frame, node, k)] = w14
                    d["k14_%d_%s_%s" % (frame, node, k)] = _far(f(Q, G[node], frame), w14)
        d_ref[str(si)] = d
    return keep, d_ref


def check_row(row, h, l2, ref, numpy_finite):
    """The builder's conditions (module docstring), on the references alone.  Returns the figures."""
    kind = kind_of(row)
    site = cc.kc.column_sites(h)
    deep = cc.deep_sites(row[1])
    deep_cols = np.isin(site, deep)
    counts = ref["counts"]
    fig = dict(kind=kind, deep_max_log2=float(l2[deep_cols].max()), columns_below=int((l2 < -1074).sum()),
               numpy_finite=bool(numpy_finite), spread_bits=float(cc.ext_spread_bits(h, l2)),
               counts=sorted(set(int(c) for c in counts)), deep_counts=[int(counts[t]) for t in deep],
               vd_spread=int(((ref["post"]["vd_junction"] > 0.01) & (ref["post"]["vd_junction"] < 0.99)).sum()),
               dj_spread=int(((ref["post"]["dj_junction"] > 0.01) & (ref["post"]["dj_junction"] < 0.99)).sum()),
               spread_sites=int(((ref["site_base"] > 0.01) & (ref["site_base"] < 0.99)).any(axis=1).sum()),
               alleles=max(sum(1 for p in g.values() if p > 0.01) for g in ref["genes"].values()),
               margin=float(ref["viterbi_margin"]), d_smoothing=ref["d_smoothing"], d_q_sites=ref["d_q_sites"])
    name = row[0]
    assert ref["d_smoothing"] <= 1e-12, (name, "smoothing over the alpha rows is not forward_backward", ref["d_smoothing"])
    assert ref["d_q_sites"] <= 1e-12, (name, "Q's site marginals are not site_base", ref["d_q_sites"])
    if kind == "control":
        assert numpy_finite, (name, "a control row must be finite in the default mode")
        return fig
    assert fig["deep_max_log2"] < -1074, (name, "a deep column at or above 2^-1074", fig["deep_max_log2"])
    assert not numpy_finite, (name, "the numpy oracle's default-mode log-likelihood is finite")
    # (the shifted window within [2^-256, 1]: cadence_cases.site_shifts asserted it)
    assert fig["spread_bits"] < cc.EXT_SPREAD_BITS, (name, fig["spread_bits"])
    assert len(fig["counts"]) >= 3, (name, "fewer than three distinct per-site counts", fig["counts"])
    if kind == "spread":
        from tests import test_gpu_viterbi as tv
        assert fig["vd_spread"] >= 30 and fig["dj_spread"] >= 30, (name, fig["vd_spread"], fig["dj_spread"])
        assert fig["spread_sites"] >= 15, (name, fig["spread_sites"])
        assert fig["alleles"] >= 2, (name, ref["genes"])
        assert fig["margin"] > tv.MIN_MARGIN, (name, fig["margin"])
    return fig


def build_row(args):
    """One row in a pool process: exact emissions, references, conditions, pins, lineage tables.  Returns (name, dict for the
    row's npz)."""
    import shutil
    import tempfile
    import time
    from tests import extreme_worker as xw
    family, row, with_lineage = args
    t0 = time.perf_counter()
    work = tempfile.mkdtemp(prefix="lh_ext_deep_")
    try:
        h = cc.load_family(family, work)
        sample, R = cc.sample_of(row)
        x = cc.exact_row(h, sample, R, entries=False)
        l2 = x["log2_emission"]
        with np.errstate(all="ignore"):
            numpy_ll = xw.oracle_results(h, sample, R)["loglik"]
        ref = references(h, l2)
        fig = check_row(row, h, l2, ref, np.isfinite(numpy_ll))
        pin = pin_row(h, l2, ref, row[0] in FULL_PIN, family)
        fig["d_ll_fb"] = abs(ref["ll_fb"] - pin["loglik"]) / abs(pin["loglik"])
        words = k4_words(h, row[0])
        k4_states, fig["k4_margin"] = k4_reference(h, ref["alpha"], words)
        d_c = 0.0
        if kind_of(row) == "control":       # cadence_worker.ll_bound's d_C: the C restatement's own distance from exact
            from oracle import oracle_c
            with np.errstate(all="ignore"):
                c_ext = float(oracle_c.COracleFamily(h, R).eval([(x["children"], x["root"], x["brlen"])], [sample["er"]], [sample["pi"]],
                                                                [sample["alpha"]], extended=True)[0])
            d_c = abs(c_ext - pin["loglik"]) / abs(pin["loglik"])
        fig["d_c"] = d_c
    finally:
        shutil.rmtree(work, ignore_errors=True)
    d_ref = dict(site_base=pin["site_base"], genes=pin["genes"], posterior=max(ref["d_smoothing"], pin["site_base"]),
                 events=max(ref["d_smoothing"], pin["site_base"]))
    # Q: pinned on the full rows; elsewhere its site marginals are site_base's, whose pin stands for it
    d_ref["Q"] = max(pin["Q"], pin["site_base"], ref["d_q_sites"])
    keep = dict(l2=l2, k=ref["k"], counts=ref["counts"], loglik=pin["loglik"], compact=ref["compact"], site_base=ref["site_base"],
                genes=np.concatenate([[ref["genes"][s][n] for n in sorted(ref["genes"][s])] for s in ("V", "D", "J")]),
                Q0=ref["Q0"], Q1=ref["Q1"], Q2=ref["Q2"], events=ref["events"], viterbi_states=ref["viterbi_states"],
                viterbi_log_path=ref["viterbi_log_path"], k4_words=words, k4_states=k4_states, k4_margin=fig["k4_margin"], d_c=d_c)
    keep.update({"alpha_" + k: v for k, v in ref["alpha"].items()})
    fig.update({k: int(v) for k, v in pin.items() if k.startswith("n_")})
    if with_lineage:
        lk, ld = lineage_references(family, row, ref)
        keep.update(lk)
        d_ref["lineage"] = ld
    fig["seconds"] = time.perf_counter() - t0
    keep["d_ref"], keep["figures"] = json.dumps(d_ref), json.dumps(fig)
    return row[0], keep


def build(out_dir, jobs=1, with_lineage=True):
    """DIR/ext_deep_<row>.npz for every row of both families; returns {row: (figures, d_ref)}."""
    os.makedirs(out_dir, exist_ok=True)
    todo = [(family, row, with_lineage) for family in FAMILIES for row in distinct_rows(family)]
    if jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(jobs, len(todo))) as pool:
            done = pool.map(build_row, todo, chunksize=1)
    else:
        done = [build_row(t) for t in todo]
    out = {}
    for name, keep in done:
        np.savez(os.path.join(out_dir, "ext_deep_%s.npz" % name), **keep)
        out[name] = (json.loads(keep["figures"]), json.loads(keep["d_ref"]))
    return out


def bound(d_ref):
    return max(FLOOR, 8.0 * float(d_ref))


def report(built):
    lines = ["rows of tests/ext_deep_cases.py: the conditions' figures and d_ref per table (a device bound is max(1e-10, 8 d_ref))"]
    for name, (f, d) in built.items():
        lines.append("%-16s %-7s deep columns below 2^%.0f (%d columns below 2^-1074)  numpy oracle %s  allele spread %.0f bits  counts %s "
                     "(deep sites %s)" % (name, f["kind"], f["deep_max_log2"], f["columns_below"],
                                          "finite" if f["numpy_finite"] else "not finite", f["spread_bits"], f["counts"], f["deep_counts"]))
        lines.append("%-16s         junction state posteriors in (0.01, 0.99): V-D %d, D-J %d  sites with a spread naive base %d  alleles "
                     "above 0.01 in one set %d  Viterbi margin %.3g  forward_backward log-likelihood against mpmath %.2g" %
                     ("", f["vd_spread"], f["dj_spread"], f["spread_sites"], f["alleles"], f["margin"], f["d_ll_fb"]))
        lin = d.get("lineage", {})
        worst = {}
        for dd in lin.values():
            for k, v in dd.items():
                key = k.split("_")[0]
                worst[key] = max(worst.get(key, 0.0), v)
        lines.append("%-16s         d_ref: site_base %.2g (%d clamped sweeps)  Q %.2g (%d)  genes %.2g (%d)  smoothing against "
                     "forward_backward %.2g  Q's site marginals %.2g  %s  (%.1f s)" %
                     ("", d["site_base"], f["n_site_sweeps"], d["Q"], f["n_q_sweeps"], d["genes"], f["n_gene_sweeps"], f["d_smoothing"],
                      f["d_q_sites"], "  ".join("%s %.2g" % kv for kv in sorted(worst.items())), f["seconds"]))
    return "\n".join(lines) + "\n"
