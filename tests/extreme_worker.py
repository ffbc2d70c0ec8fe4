"""Helper of tests/test_gpu_extreme_parameters.py and tests/test_exact_model_oracle.py: the rows of
test_gpu_extreme_parameters.ROWS made concrete, their exact side (tests/exact_model_oracle.py) and, in a process of its own
(the K1 form hooks are environment variables read once per process), their evaluation through the C ABI.

  python tests/extreme_worker.py --oracle-only [--rows 0,5,..]     CPU: the numpy oracle's log-likelihood of every row (it must
                                                                   be finite on every row the list keeps)
  python tests/extreme_worker.py --exact DIR [--rows ..] [--jobs N]
                                                                   CPU: DIR/row<i>.npz -- exact rates, P-matrices rounded to
                                                                   double, emissions, per-rate values, the four-op fall, the
                                                                   numpy oracle's results with those P-matrices, and the
                                                                   deviations of both double-precision restatements
  python tests/extreme_worker.py --gpu DIR --tag NAME [--extended] [--rows ..]
                                                                   GPU: every row through run_family + compare under the
                                                                   hooks of this process's environment; DIR/gpu_<NAME>.npz
                                                                   (log-likelihoods, emissions, counts) and one JSON line
                                                                   {"forms": .., "failures": [..], "figures": [..]}
Nothing here asserts on its own account what test_gpu_parity.compare asserts: run_family and compare are called."""
import json
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MAX_COLUMNS = {"mixed_500": 40}      # the exact side's columns (those with the most distinct states); 120 elsewhere
KEYS = ["vgerm_forward", "vd_junction_forward", "jgerm_forward", "dgerm_forward", "dj_junction_forward"]


def family_specs():
    from tests import forms_worker
    from tools import synth_family as sf
    return {"ragged14": sf.Spec.small(n_leaves=14, n_samples=8, seed=3, ragged=4, ambiguous=0.02),
            "plain14": sf.Spec.small(n_leaves=14, n_samples=8, seed=31),
            "balanced64": sf.Spec.small(n_leaves=64, n_samples=3, seed=47, tree_shape="balanced", n_nni=0),
            "mixed_500": forms_worker.specs()["mixed_500"]}


class Families:
    """Generates each family once (a temporary directory, removed by close())."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="lh_extreme_")
        self.cache = {}

    def get(self, name):
        from oracle import linearham_oracle as orc
        from tools import synth_family as sf
        if name not in self.cache:
            out = os.path.join(self.dir, name)
            sf.generate(family_specs()[name], out)
            h = orc.PhyloHMM(os.path.join(out, "cluster.yaml"), 0, os.path.join(out, "hmm_params"), 0)
            self.cache[name] = (h, sf.read_trees_tsv(os.path.join(out, "trees.tsv")))
        return self.cache[name]

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)


def model_parameters(i, er_class, pi_class):
    """(er, pi) of row i: the named classes of the test file's docstring; the random ones seeded by the row number."""
    rng = np.random.default_rng(7000 + i)
    k = 1.0 + 1e-9
    er = {"EQ": [1.0] * 6, "K2": [1.0, 2.0, 1.0, 1.0, 2.0, 1.0], "K1e9": [1.0, k, 1.0, 1.0, k, 1.0],
          "TNe": [1.0, 3.0, 1.0, 1.0, 3.0, 1.0], "TNu": [1.0, 3.0, 1.0, 1.0, 3.0 * k, 1.0],
          "LU": (10.0 ** rng.uniform(-3, 3, 6)).tolist()}[er_class]
    if pi_class == "U":
        pi = np.full(4, 0.25)
    elif pi_class == "D":
        pi = np.maximum(rng.dirichlet(np.ones(4) * 0.2), 1e-6)
    else:
        n_small = 1 if pi_class == "P1" else 2
        pi = np.zeros(4)
        small = [(i + j) % 4 for j in range(n_small)]
        rest = [j for j in range(4) if j not in small]
        pi[small] = 1e-6
        pi[rest] = rng.dirichlet(np.ones(len(rest)) * 2) * (1.0 - n_small * 1e-6)
    pi = pi / pi.sum()
    return [float(x) for x in er], [float(x) for x in pi]


def branch_lengths(newick, branch_class):
    if branch_class.startswith("x"):
        f = lambda t: max(t * float(branch_class[1:]), 1e-6)
    elif branch_class.startswith("all"):
        f = lambda t: float(branch_class[3:])
    else:                                    # "q1": the sample's own lengths on 16 logarithmic levels between 1e-6 and 1
        f = lambda t: 10.0 ** (round(np.log10(min(max(t, 1e-6), 1.0)) * 15 / 6) * 6 / 15)
    return re.sub(r":([0-9.eE+-]+)", lambda m: ":%.12g" % f(float(m.group(1))), newick)


def sample_of(i, row, base):
    """Row i of ROWS as the dict(tree, er, pi, alpha) run_family takes, and R."""
    fam, er_class, pi_class, alpha, R, branch_class = row
    er, pi = model_parameters(i, er_class, pi_class)
    return dict(tree=branch_lengths(base[i % len(base)]["tree"], branch_class), er=er, pi=pi, alpha=float(alpha)), R


def label(i, row):
    return "row %d %s %s/%s alpha=%g R=%d %s" % ((i,) + tuple(row))


def p_substitute(P, brl):
    """What to monkeypatch linearham_oracle.gtr_pmatrices with: the row's exact matrices (checked to be asked for the branches
    they were made for)."""
    def gtr_pmatrices(er, pi, rates, brlens, small_qt_form=False, plain_exp=False):
        assert P.shape[:2] == (len(brlens), len(rates)) and np.array_equal(np.asarray(brlens, float), brl)
        return P
    return gtr_pmatrices


def pick_columns(xmsa, n_max):
    """The xmsa columns the exact side prunes: those with the most distinct states among the non-naive rows first."""
    distinct = np.array([len(set(xmsa[1:, c])) for c in range(xmsa.shape[1])])
    return np.sort(np.argsort(-distinct, kind="stable")[:n_max])


def reldev(a, b):
    """Largest relative deviation of a from b over b's nonzero entries (inf where a is not finite there)."""
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    m = b != 0
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(a[m] - b[m]) / np.abs(b[m])
    return float(np.nan_to_num(d, nan=np.inf).max())


def oracle_results(h, sample, R, gtr=None):
    """The numpy oracle's results of one row as run_family collects them (optionally with substituted P-matrices)."""
    import pytest
    from oracle import linearham_oracle as orc
    with pytest.MonkeyPatch.context() as mp:
        if gtr is not None:
            mp.setattr(orc, "gtr_pmatrices", gtr)
        with np.errstate(all="ignore"):
            h.initialize_phylo_parameters(sample["tree"], sample["er"], sample["pi"], sample["alpha"], R, is_path=False)
            h.initialize_phylo_emission()
            r = {"loglik": float(h.log_likelihood()), "xmsa_emission": h.xmsa_emission.copy()}
        for k in KEYS:
            if hasattr(h, k) and (h.locus == "igh" or not k.startswith("d")):
                r[k] = np.asarray(getattr(h, k)).copy()
    return r


def exact_row(args):
    """Everything the CPU knows about row i (runs in a pool process): see the module docstring."""
    i, row, out_dir = args
    from oracle import linearham_oracle as orc
    from oracle import oracle_c
    from tests import desc_builder as db
    from tests import exact_model_oracle as ex
    import linearham_amd
    fams = Families()
    try:
        h, base = fams.get(row[0])
        sample, R = sample_of(i, row, base)
        tree = orc.parse_newick(sample["tree"])
        T = h.msa.shape[0] + 1
        children, root, brlen = db.tree_arrays(tree, h.xmsa_labels)
        ops, depth = linearham_amd.load_library().schedule_tree(T, children, root)
        rates_mp = ex.gamma_rates_mean(sample["alpha"], R, as_double=False)
        model = ex.ExactModel(sample["er"], sample["pi"], rates_mp)
        brl = np.asarray(ex.branch_order(tree), float)
        P = model.pmatrices_double(brl)
        cols = pick_columns(h.xmsa, MAX_COLUMNS.get(row[0], 120))
        pr = model.prune(T, children, root, brlen, h.xmsa, cols)
        fall = ex.four_op_drop(T, children, ops, pr["node_log2max"])
        # ... and over sixteen ops, in the categories within 2^-60 of the column's best (those that reach the mixture)
        fall16 = ex.four_op_drop(T, children, ops, pr["node_log2max"], window=16, live_within=60)
        # the double-precision restatements: numpy (eigh) as it is, numpy with the exact P-matrices, C (cyclic Jacobi)
        plain = oracle_results(h, sample, R)
        exactp = oracle_results(h, sample, R, p_substitute(P, brl))
        ofam = oracle_c.COracleFamily(h, R)
        trees = [(children, root, brlen)]
        with np.errstate(all="ignore"):
            c_ll, c_em = ofam.eval(trees, [sample["er"]], [sample["pi"]], [sample["alpha"]], want_em=True)
            c_fwd = ofam.eval_forward(trees, [sample["er"]], [sample["pi"]], [sample["alpha"]])[0]
        e = pr["emission"]
        out = dict(columns=cols, rates=np.array([float(x) for x in rates_mp]), P=P, brl=brl, emission=e,
                   log2_emission=pr["log2_emission"], per_rate_log2=pr["per_rate_log2"], four_op_fall=fall, live_16_op_fall=fall16,
                   loglik_exactp=exactp["loglik"], loglik_numpy=plain["loglik"], loglik_c=float(c_ll[0]),
                   # deviations from the exact side: emissions on the exact columns, log-likelihood and forward arrays
                   # through the numpy oracle run with the exact P-matrices
                   d_c_em=reldev(c_em[0][cols], e), d_np_em=reldev(plain["xmsa_emission"][cols], e),
                   d_exactp_em=reldev(exactp["xmsa_emission"][cols], e),
                   d_c_ll=abs(float(c_ll[0]) - exactp["loglik"]) / abs(exactp["loglik"]),
                   d_np_ll=abs(plain["loglik"] - exactp["loglik"]) / abs(exactp["loglik"]),
                   d_c_fwd=max(reldev(c_fwd[k], exactp[k]) for k in KEYS if k in exactp),
                   d_c_em_all=reldev(c_em[0], exactp["xmsa_emission"]))
        if out_dir:
            np.savez(os.path.join(out_dir, "row%d.npz" % i), **out)
        return i, {k: (float(v) if np.ndim(v) == 0 else None) for k, v in out.items() if np.ndim(v) == 0}
    finally:
        fams.close()


def run_exact(out_dir, rows, jobs):
    """DIR/row<i>.npz for the rows given, on `jobs` processes (spawned: the caller may hold the GPU)."""
    import multiprocessing as mp
    from tests.test_gpu_extreme_parameters import ROWS
    work = [(i, ROWS[i], out_dir) for i in rows]
    # the costly rows first
    work.sort(key=lambda w: -({"mixed_500": 100, "balanced64": 10}.get(w[1][0], 1) * w[1][4]))
    if jobs <= 1:
        return dict(exact_row(w) for w in work)
    with mp.get_context("spawn").Pool(jobs) as pool:
        return dict(pool.imap_unordered(exact_row, work))


def tolerances(x):
    """compare()'s bounds for a row, by the rule of the test file's docstring (b): max(its own bound, 8 d_C)."""
    return dict(rtol=max(1e-12, 8 * float(x["d_c_ll"])), em_rtol=max(1e-10, 8 * max(float(x["d_c_em"]), float(x["d_c_em_all"]))),
                fwd_rtol=max(1e-9, 8 * float(x["d_c_fwd"])))


def run_gpu(out_dir, tag, rows, extended):
    import pytest
    import linearham_amd
    from oracle import linearham_oracle as orc
    from tests import test_gpu_parity as tp
    from tests.test_gpu_extreme_parameters import ROWS
    hip = linearham_amd.load_library()
    assert hip.device_count() >= 1, "no HIP device visible"
    fams = Families()
    forms, failures, figures = {}, [], []
    keep = {}
    try:
        for i in rows:
            row = ROWS[i]
            h, base = fams.get(row[0])
            sample, R = sample_of(i, row, base)
            x = np.load(os.path.join(out_dir, "row%d.npz" % i))
            tol = tolerances(x)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(orc, "gtr_pmatrices", p_substitute(x["P"], x["brl"]))
                with np.errstate(all="ignore"):
                    desc, ll, res, ref = tp.run_family(hip, h, [sample], R, extended=extended)
            forms.setdefault(row[0], set()).add(tp.LAST_RUN["form"])
            keep["ll%d" % i], keep["em%d" % i], keep["sc%d" % i] = ll[0], res["xmsa_emission"][0], res["scaler_counts"][0]
            cols, e = x["columns"], x["emission"]
            got = res["xmsa_emission"][0][cols]
            fig = dict(row=i, loglik=float(ll[0]), d_ll=abs(ll[0] - ref[0]["loglik"]) / abs(ref[0]["loglik"]),
                       d_em_exact=reldev(got, e), d_em=reldev(res["xmsa_emission"][0], ref[0]["xmsa_emission"]),
                       d_rates=reldev(res["rates"][0], x["rates"]), **{k: float(v) for k, v in tol.items()})
            figures.append(fig)
            if extended:      # (e): the parent compares with the default mode's log-likelihood
                if not np.isfinite(ll[0]):
                    failures.append("%s: extended-range log-likelihood %r" % (label(i, row), ll[0]))
                continue
            try:
                assert np.isfinite(ref[0]["loglik"]), "the reference is not finite on this row"
                # (a) rates against the exact means
                np.testing.assert_allclose(res["rates"][0], x["rates"], rtol=1e-9, atol=1e-13)
                assert abs(res["rates"][0].mean() - 1.0) < 1e-12
                # (b) everything against the numpy oracle with the exact P-matrices
                tp.compare(h, desc, ll, res, ref, **tol)
                # (c) emissions against the exact entries
                np.testing.assert_allclose(got, e, rtol=tol["em_rtol"], atol=0)
                assert np.all(got[e < 1e-308] == 0)
            except AssertionError as err:
                failures.append("%s [%s]: %s" % (label(i, row), tp.LAST_RUN["form"], " ".join(str(err).split())[:600]))
    finally:
        fams.close()
    np.savez(os.path.join(out_dir, "gpu_%s.npz" % tag), **keep)
    print(json.dumps({"forms": {k: sorted(v) for k, v in forms.items()}, "failures": failures, "figures": figures,
                      "rows": len(rows)}))


def main(argv):
    from tests.test_gpu_extreme_parameters import ROWS

    def opt(name, default=None):
        return argv[argv.index(name) + 1] if name in argv else default
    rows = [int(x) for x in opt("--rows").split(",")] if "--rows" in argv else list(range(len(ROWS)))
    if "--oracle-only" in argv:
        fams = Families()
        bad = 0
        try:
            for i in rows:
                h, base = fams.get(ROWS[i][0])
                sample, R = sample_of(i, ROWS[i], base)
                ll = oracle_results(h, sample, R)["loglik"]
                bad += 0 if np.isfinite(ll) else 1
                print("%s: %.12g" % (label(i, ROWS[i]), ll), flush=True)
        finally:
            fams.close()
        print("%d rows, %d not finite in the numpy oracle" % (len(rows), bad))
        return 1 if bad else 0
    if "--exact" in argv:
        out = run_exact(opt("--exact"), rows, int(opt("--jobs", "1")))
        print(json.dumps(out))
        return 0
    run_gpu(opt("--gpu"), opt("--tag", "default"), rows, "--extended" in argv)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
