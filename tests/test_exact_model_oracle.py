"""The exact reference of the substitution-model step (tests/exact_model_oracle.py): its self-checks, its agreement with both
double-precision oracles inside the comfortable box of parameters, and -- on the fixed extreme rows of
tests/test_gpu_extreme_parameters.py -- the measurement of how far each double-precision restatement (numpy / LAPACK eigh,
C / cyclic Jacobi, the algorithm K0a runs) is from it.  No GPU.

python tests/test_exact_model_oracle.py --table profiles/r06_extreme_parameters_cpu.txt [--jobs N] writes that measurement for
every row (the file committed under profiles/)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import linearham_oracle as orc  # noqa: E402
from tests import exact_model_oracle as ex  # noqa: E402

ER, PI, ALPHA = [1.0] * 6, [0.17, 0.19, 0.25, 0.39], 1.0       # the toy families' constants (tests/test_gpu_parity.py)
MODELS = {"toy_f81": (ER, PI), "jc69": ([1.0] * 6, [0.25] * 4), "k80": ([1.0, 2.0, 1.0, 1.0, 2.0, 1.0], [0.25] * 4),
          "near_k80": ([1.0, 1.0 + 1e-9, 1.0, 1.0, 1.0 + 1e-9, 1.0], [0.25] * 4),
          "gtr": ([0.3, 2.1, 0.7, 1.3, 4.0, 1.0], [0.1, 0.2, 0.3, 0.4]),
          "small_pi": ([1e-3, 5.0, 0.2, 30.0, 1.0, 1e2], [1e-6, 0.3, 0.2, 0.5 - 1e-6])}


def _mp():
    mpmath = pytest.importorskip("mpmath")
    return mpmath


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("s", [1e-186, 1e-6, 0.1, 3.0, 1e4])
def test_p_is_stochastic_and_reversible(name, s):
    """Rows of P sum to 1 and pi_i P_ij = pi_j P_ji, to the working precision RELATIVE to the off-diagonal entries (P - I is what
    is carried -- expm1_q -- so a 1e-186 entry is held to 80 digits of its own)."""
    mp = _mp()
    er, pi = MODELS[name]
    with mp.workdps(ex.DPS):
        E = ex.expm1_q(er, pi, s)
        pim = [mp.mpf(x) for x in pi]
        tol = mp.mpf(10) ** (-(ex.DPS - 8))
        for i in range(4):
            off = sum(E[i][j] for j in range(4) if j != i)
            assert abs(E[i][i] + off) <= tol * off and -1 < E[i][i] < 0
            for j in range(4):
                if j != i:
                    assert E[i][j] > 0
                    assert abs(pim[i] * E[i][j] - pim[j] * E[j][i]) <= tol * pim[i] * E[i][j]


@pytest.mark.parametrize("name", list(MODELS))
def test_semigroup(name):
    mp = _mp()
    er, pi = MODELS[name]
    with mp.workdps(ex.DPS):
        a, b, c = ex.expm_q(er, pi, 0.37), ex.expm_q(er, pi, 2.5), ex.expm_q(er, pi, mp.mpf(0.37) + mp.mpf(2.5))
        ab = ex._mm(a, b)
        assert max(abs(ab[i][j] - c[i][j]) / c[i][j] for i in range(4) for j in range(4)) < mp.mpf(10) ** (-(ex.DPS - 8))


@pytest.mark.parametrize("s", [1e-186, 1e-6, 0.1, 3.0, 100.0])
def test_closed_forms_of_jc69_and_f81(s):
    """JC69: P_ij = 1/4 - 1/4 exp(-4 s / 3).  F81: P_ij = pi_j (1 - exp(-beta s)), beta = 1 / (1 - sum pi^2) for frequencies that sum to 1.  Both have a
    triple eigenvalue; the scaling-and-squaring reference has no special case for it."""
    mp = _mp()
    with mp.workdps(ex.DPS):
        tol = mp.mpf(10) ** (-(ex.DPS - 8))
        P = ex.expm_q([1.0] * 6, [0.25] * 4, s)
        want = -mp.expm1(-4 * mp.mpf(s) / 3) / 4
        assert all(abs(P[i][j] - want) <= tol * want for i in range(4) for j in range(4) if i != j)
        P = ex.expm_q(ER, PI, s)
        pim = [mp.mpf(x) for x in PI]
        # (the four doubles do not sum to 1 exactly, and the reference takes them as given: S = sum pi, mu = sum pi_i (S - pi_i))
        S = sum(pim)
        beta = S / sum(x * (S - x) for x in pim)
        for i in range(4):
            for j in range(4):
                if i != j:
                    want = -pim[j] / S * mp.expm1(-beta * s)
                    assert abs(P[i][j] - want) <= tol * want


def test_doubling_the_precision_changes_nothing_in_30_digits():
    mp = _mp()
    er, pi = MODELS["small_pi"]
    for s in (1e-6 * 1e-180, 0.01, 50.0):
        a, b = ex.expm_q(er, pi, s, dps=ex.DPS), ex.expm_q(er, pi, s, dps=2 * ex.DPS)
        with mp.workdps(2 * ex.DPS):
            assert max(abs(a[i][j] - b[i][j]) / b[i][j] for i in range(4) for j in range(4)) < mp.mpf(10) ** -60
    for alpha, R in ((0.005, 8), (0.7, 4), (1e4, 8)):
        a, b = ex.gamma_rates_mean(alpha, R, ex.DPS, as_double=False), ex.gamma_rates_mean(alpha, R, 2 * ex.DPS, as_double=False)
        with mp.workdps(2 * ex.DPS):
            assert max(abs(x - y) / y for x, y in zip(a, b)) < mp.mpf(10) ** -30


def test_decimal_backend_gives_the_same_matrices(monkeypatch):
    """Where mpmath does not import the module runs on the standard library's decimal: same algorithm, same digits."""
    mp = _mp()
    er, pi = MODELS["small_pi"]
    for s in (1e-186, 0.3, 40.0):
        a = ex.expm_q(er, pi, s)
        monkeypatch.setattr(ex, "BACKEND", "decimal")
        b = ex.expm_q(er, pi, s)
        monkeypatch.undo()
        with mp.workdps(ex.DPS):
            assert max(abs(a[i][j] - mp.mpf(str(b[i][j]))) / a[i][j] for i in range(4) for j in range(4)) < mp.mpf(10) ** -70


def test_category_means():
    """Mean 1 exactly (to the working precision); scipy's values (linearham_oracle.gamma_rates_mean) inside the shapes the
    suite has always checked; R = 1."""
    mp = _mp()
    assert ex.RATES_ARE_EXACT
    for alpha in (0.005, 0.05, 0.37, 1.0, 20.0, 150.0, 1e4):
        for R in (2, 4, 8):
            r = ex.gamma_rates_mean(alpha, R, as_double=False)
            with mp.workdps(ex.DPS):
                assert abs(sum(r) / R - 1) < mp.mpf(10) ** -(ex.DPS - 10)
                assert all(r[k] < r[k + 1] for k in range(R - 1)) and r[0] > 0
            if 0.05 <= alpha <= 150:
                np.testing.assert_allclose(ex.gamma_rates_mean(alpha, R), orc.gamma_rates_mean(alpha, R), rtol=1e-11, atol=1e-16)
    assert ex.gamma_rates_mean(0.3, 1).tolist() == [1.0]


def test_numpy_pmatrices_inside_the_comfortable_box():
    rng = np.random.default_rng(2)
    for er, pi in [(ER, PI)] + [(rng.dirichlet(np.ones(6)).tolist(), rng.dirichlet(np.ones(4) * 2).tolist()) for _ in range(4)]:
        rates = orc.gamma_rates_mean(0.7, 4)
        brl = [1e-6, 0.003, 0.2, 1.5]
        got = orc.gtr_pmatrices(er, pi, rates, brl)
        want = ex.ExactModel(er, pi, [float(x) for x in rates]).pmatrices_double(brl)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(ex.exact_gtr_pmatrices()(er, pi, rates, brl), want)


@pytest.mark.parametrize("model", ["toy", "dirichlet"])
def test_both_oracles_emissions_inside_the_comfortable_box(data_dir, model):
    """The toy family with its own constants and with a Dirichlet(1) / Dirichlet(2) draw: numpy oracle, C oracle and the exact
    entries agree at the 1e-12 the suite uses between the two oracles (tests/test_oracle_c.py)."""
    from oracle import oracle_c
    from tests import desc_builder as db
    rng = np.random.default_rng(4)
    er, pi, alpha = (ER, PI, ALPHA) if model == "toy" else (rng.dirichlet(np.ones(6)).tolist(),
                                                            rng.dirichlet(np.ones(4) * 2).tolist(), 0.4)
    ll, h = orc.phylo_loglik(os.path.join(data_dir, "phylo_hmm_input_extra.yaml"), os.path.join(data_dir, "hmm_params"),
                             os.path.join(data_dir, "newton.tree"), er, pi, alpha, 4)
    children, root, brlen = db.tree_arrays(h.tree, h.xmsa_labels)
    _, em_c = oracle_c.COracleFamily(h, 4).eval([(children, root, brlen)], [er], [pi], [alpha], want_em=True)
    model_ = ex.ExactModel(er, pi, ex.gamma_rates_mean(alpha, 4, as_double=False))
    cols = list(range(h.xmsa.shape[1]))
    pr = model_.prune(h.xmsa.shape[0], children, root, brlen, h.xmsa, cols)
    np.testing.assert_allclose(h.xmsa_emission, pr["emission"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(em_c[0], pr["emission"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.log2(pr["emission"]), pr["log2_emission"], rtol=0, atol=1e-9)
    # the unmixed per-rate values give the mixture back
    naive = h.xmsa[0, cols]
    mix = np.mean(2.0 ** pr["per_rate_log2"], axis=0) / np.where(naive < 4, np.asarray(pi)[np.minimum(naive, 3)], 1.0)
    np.testing.assert_allclose(mix, pr["emission"], rtol=1e-9)


def test_rows_cover_every_factor_and_pair():
    from tests.test_gpu_extreme_parameters import ROWS
    fam, er, pi, alpha, R, br = (sorted(set(r[k] for r in ROWS), key=str) for k in range(6))
    assert set(fam) == {"ragged14", "plain14", "balanced64", "mixed_500"}
    assert set(er) == {"EQ", "K2", "K1e9", "TNe", "TNu", "LU"} and set(pi) == {"U", "D", "P1", "P2"}
    assert set(alpha) == {0.005, 0.02, 0.05, 1, 150, 1000, 1e4} and set(R) == {1, 2, 4, 8}
    assert set(br) == {"x0.01", "x1", "x100", "all1e-6", "all100", "q1"}
    classes = {(e, p) for e in er for p in pi}
    assert {(r[1], r[2], r[3]) for r in ROWS} >= {c + (a,) for c in classes for a in alpha}
    assert {(r[1], r[2], r[5]) for r in ROWS} >= {c + (b,) for c in classes for b in br if b != "q1"}
    assert {(r[3], r[4]) for r in ROWS} == {(a, n) for a in alpha for n in R}
    assert 150 <= len(ROWS) <= 200


# Four of the extreme rows in the suite itself (all of them: the --table run below): the smallest alpha on 1e-6 branches, two
# components of pi at 1e-6 under a triple eigenvalue, a nearly repeated eigenvalue, six decades of exchangeabilities.
@pytest.mark.parametrize("i", [21, 23, 49, 165])
def test_extreme_rows_on_the_cpu(i):
    """What holds whichever restatement is the accurate one: with the exact P-matrices handed to it, the numpy oracle's emissions
    are the exact ones to 1e-12 (the P-matrix is the one ill-conditioned step: pruning is sums and products of non-negative
    numbers), and both plain restatements are finite and within 1e-5 of them (the worst figure of
    profiles/r06_extreme_parameters_cpu.txt is 2.3e-6: LAPACK's eigh at two components of pi at 1e-6)."""
    from tests import extreme_worker as xw
    from tests.test_gpu_extreme_parameters import ROWS
    _, fig = xw.exact_row((i, ROWS[i], None))
    assert fig["d_exactp_em"] <= 1e-12, fig
    assert fig["d_np_em"] <= 1e-5 and fig["d_c_em"] <= 1e-5, fig
    assert np.isfinite(fig["loglik_exactp"]) and fig["four_op_fall"] <= 0


def write_table(path, jobs):
    from tests import extreme_worker as xw
    from tests.test_gpu_extreme_parameters import ROWS
    figs = xw.run_exact(None, list(range(len(ROWS))), jobs)
    with open(path, "w") as f:
        f.write("Extreme substitution-model parameters on the CPU: the two double-precision restatements of\n"
                "P = I + U expm1(lambda t r) U^-1 against the exact reference (tests/exact_model_oracle.py, %s, %d digits).\n"
                "np = numpy oracle (LAPACK eigh), C = oracle_kernels.c (cyclic Jacobi, the algorithm of K0a).\n"
                "em: largest relative deviation of an xmsa_emission entry from the exact one (the exact side's columns);\n"
                "ll: relative deviation of the log-likelihood from the numpy oracle's run with the exact P-matrices;\n"
                "fwd(C): the same for the forward arrays; exactP em: that run's own emissions against the exact ones;\n"
                "fall: the largest fall in binades over four consecutive schedule ops (exact_model_oracle.four_op_drop).\n"
                "(written by python tests/test_exact_model_oracle.py --table)\n\n" % (ex.BACKEND, ex.DPS))
        f.write("%4s %-10s %-5s %-3s %7s %2s %-8s %9s %9s %9s %9s %9s %9s %9s\n" % (
            "row", "family", "er", "pi", "alpha", "R", "branches", "em(np)", "em(C)", "ll(np)", "ll(C)", "fwd(C)", "exactP em", "fall"))
        for i, r in enumerate(ROWS):
            g = figs[i]
            f.write("%4d %-10s %-5s %-3s %7g %2d %-8s %9.1e %9.1e %9.1e %9.1e %9.1e %9.1e %9.1f\n" % (
                (i,) + tuple(r) + (g["d_np_em"], g["d_c_em"], g["d_np_ll"], g["d_c_ll"], g["d_c_fwd"], g["d_exactp_em"], g["four_op_fall"])))
        f.write("\nworst per class of base frequencies       em(np)    em(C)   ll(np)    ll(C)\n")
        for p in ("U", "D", "P1", "P2"):
            sel = [figs[i] for i, r in enumerate(ROWS) if r[2] == p]
            f.write("%-38s %9.1e %9.1e %9.1e %9.1e\n" % ((p,) + tuple(max(g[k] for g in sel) for k in ("d_np_em", "d_c_em", "d_np_ll", "d_c_ll"))))
        closer_c = sum(1 for i, r in enumerate(ROWS) if r[2] in ("P1", "P2") and figs[i]["d_c_em"] < figs[i]["d_np_em"])
        n_small = sum(1 for r in ROWS if r[2] in ("P1", "P2"))
        f.write("\nrows with a component of pi at 1e-6: %d; C (Jacobi) closer to exact than numpy (eigh) on %d, further on %d\n"
                % (n_small, closer_c, n_small - closer_c))
        f.write("\nlargest four-op fall in binades per alpha (all rows; then per family)\n")
        for a in sorted(set(r[3] for r in ROWS)):
            per_fam = {}
            for i, r in enumerate(ROWS):
                if r[3] == a:
                    per_fam[r[0]] = min(per_fam.get(r[0], 0.0), figs[i]["four_op_fall"])
            f.write("alpha %7g: %9.1f   %s\n" % (a, min(per_fam.values()), "  ".join("%s %.1f" % kv for kv in sorted(per_fam.items()))))
        w16 = min((figs[i]["live_16_op_fall"], i) for i in range(len(ROWS)))
        f.write("\nlargest fall over SIXTEEN consecutive ops in a rate category within 2^-60 of its column's best (the categories that\n"
                "reach the mixture): %.1f binades (row %d) -- below the 2^-256 threshold that leaves %.0f binades above the subnormals\n"
                % (w16[0], w16[1], 1074 - 256 + w16[0]))
        need = [i for i in range(len(ROWS)) if 8 * figs[i]["d_c_ll"] > 1e-12 or 8 * max(figs[i]["d_c_em"], figs[i]["d_c_em_all"]) > 1e-10
                or 8 * figs[i]["d_c_fwd"] > 1e-9]
        f.write("\nrows on which 8 d_C exceeds one of compare()'s bounds (1e-12 / 1e-10 / 1e-9): %d: %s\n" % (len(need), need))


if __name__ == "__main__":
    a = sys.argv[1:]
    write_table(a[a.index("--table") + 1], int(a[a.index("--jobs") + 1]) if "--jobs" in a else 8)
