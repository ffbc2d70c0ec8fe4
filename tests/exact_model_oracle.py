"""EXACT REFERENCE OF THE SUBSTITUTION-MODEL STEP -- TEST INFRASTRUCTURE ONLY.

Arbitrary-precision restatement (mpmath, 80 digits by default) of what K0a and K1 compute, for judging the double-precision
paths -- the numpy oracle (LAPACK eigh), the C oracle and the kernels (cyclic Jacobi), all of which form
P = I + U expm1(lambda t r) U^-1 -- at model parameters where that form is ill-conditioned:

* gtr_q:                Q from (er, pi) in the project's order (AC, AG, AT, CG, CT, GT; Q_ij = er_ij pi_j; mean rate 1).
* expm_q, expm1_q:      P(t r) = exp(Q t r) WITHOUT an eigen-decomposition: halve until ||Q t r|| < 2^-8, sum the Taylor series
                        of exp - I to the working precision, square back as E <- 2E + E^2 (P = I + E, so that the off-diagonal
                        entries of a 1e-6 branch at a rate of 1e-180 keep their full relative precision).  A repeated or nearly
                        repeated eigenvalue is no special case here.
* gamma_rates_mean:     discrete-Gamma category means (PLL_GAMMA_RATES_MEAN, equal weights) from the regularised incomplete
                        gamma function at the same precision.
* ExactModel.prune:     Felsenstein pruning per alignment column, N = (1,1,1,1), all R categories with equal weights, the naive
                        state closed through the naive branch, the division by pi[naive] (none for a naive N): the exact
                        xmsa_emission entries, with NO rescaling (mpmath's exponent range is unbounded), as log2 next to the
                        value rounded to double; the same per rate category, unmixed.
* ExactModel.pmatrices_double, exact_gtr_pmatrices:
                        the exact P-matrices rounded to double in linearham_oracle.gtr_pmatrices' shape [branches, R, 4, 4].
* four_op_drop:         from the exact per-rate conditional likelihoods, the largest fall in binades over four consecutive
                        ops of a lh_schedule_tree schedule (see its docstring for what is counted).
* entry_window_drop:    the same windows, for EVERY entry of the vectors that can still reach the result, not the largest alone.

mpmath comes with torch's sympy.  Where it does not import, BACKEND is "decimal": the same algorithms run on the standard
library's decimal module at the same number of digits, except the category means, for which scipy's gammaincinv / gammainc (as
in linearham_oracle.gamma_rates_mean) then stay the reference -- gamma_rates_mean says so through RATES_ARE_EXACT.
It restates published formulas (Felsenstein 1981; Yang 1994; Moler & Van Loan 2003, method 3) and this project's conventions."""
import decimal as _dec
import math

import numpy as np

DPS = 80

try:
    import mpmath as _mpm
    BACKEND = "mpmath"
except ImportError:          # pragma: no cover - exercised only where mpmath is missing
    _mpm = None
    BACKEND = "decimal"
RATES_ARE_EXACT = BACKEND == "mpmath"


# ------------------------------------------------------------------------------------------------------------------------
# the two number back-ends: exact conversion from a double, +, *, /, log2, rounding to double
# ------------------------------------------------------------------------------------------------------------------------
class _Work:
    """Context manager: the working precision, and the handful of operations that differ between the back-ends."""

    def __init__(self, dps):
        self.dps = dps

    def __enter__(self):
        if BACKEND == "mpmath":
            self._ctx = _mpm.workdps(self.dps)
            self._ctx.__enter__()
            self.num = lambda x: _mpm.mpf(x)
            self.log2 = lambda x: float(_mpm.log(x, 2)) if x > 0 else -math.inf
            self.eps = _mpm.mpf(10) ** (-self.dps)
        else:
            self._ctx = _dec.localcontext()
            c = self._ctx.__enter__()
            c.prec, c.Emax, c.Emin = self.dps, _dec.MAX_EMAX, _dec.MIN_EMIN
            c.traps[_dec.Inexact] = c.traps[_dec.Rounded] = c.traps[_dec.Subnormal] = False
            self.num = lambda x: _dec.Decimal(x) if not isinstance(x, _dec.Decimal) else x
            ln2 = _dec.Decimal(2).ln()
            self.log2 = lambda x: float(x.ln() / ln2) if x > 0 else -math.inf
            self.eps = _dec.Decimal(10) ** (-self.dps)
        return self

    def __exit__(self, *a):
        return self._ctx.__exit__(*a)


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] + A[i][3] * B[3][j] for j in range(4)] for i in range(4)]


def _q(w, er, pi):
    er, pi = [w.num(float(x)) for x in er], [w.num(float(x)) for x in pi]
    S = [[w.num(0)] * 4 for _ in range(4)]
    k = 0
    for i in range(4):
        for j in range(i + 1, 4):
            S[i][j] = S[j][i] = er[k]            # AC AG AT CG CT GT
            k += 1
    Q = [[S[i][j] * pi[j] if i != j else w.num(0) for j in range(4)] for i in range(4)]
    for i in range(4):
        Q[i][i] = -(Q[i][0] + Q[i][1] + Q[i][2] + Q[i][3])
    mu = -(pi[0] * Q[0][0] + pi[1] * Q[1][1] + pi[2] * Q[2][2] + pi[3] * Q[3][3])
    return [[Q[i][j] / mu for j in range(4)] for i in range(4)], pi


def _expm1_q(w, Q, s):
    """E = exp(Q s) - I, s >= 0: scaling and squaring of the Taylor series, no eigen-decomposition."""
    zero = w.num(0)
    if s == 0:
        return [[zero] * 4 for _ in range(4)]
    norm = max(sum(abs(x) for x in row) for row in Q) * s
    halvings = 0
    while norm >= w.num(1) / 256:
        norm /= 2
        halvings += 1
    sc = s / w.num(2) ** halvings
    A = [[x * sc for x in row] for row in Q]
    E = [row[:] for row in A]
    term = [row[:] for row in A]
    n = 1
    while True:
        n += 1
        term = [[x / n for x in row] for row in _mm(term, A)]
        E = [[E[i][j] + term[i][j] for j in range(4)] for i in range(4)]
        # the tail after term n is below 2 ||term_n|| (||A|| < 2^-8); every entry of E is of the order of A's own entry or
        # larger, so a tail below eps times the SMALLEST entry of A is beyond the working precision of every entry
        if max(abs(x) for row in term for x in row) <= w.eps * min(abs(x) for row in A for x in row if x != 0):
            break
    for _ in range(halvings):
        E2 = _mm(E, E)
        E = [[2 * E[i][j] + E2[i][j] for j in range(4)] for i in range(4)]
    return E


def gtr_q(er, pi, dps=DPS):
    """Q (mean rate 1) as nested lists of working-precision numbers."""
    with _Work(dps) as w:
        return _q(w, er, pi)[0]


def expm1_q(er, pi, s, dps=DPS):
    """E = exp(Q s) - I: what the module carries (an off-diagonal entry of 1e-186 next to a diagonal of 1 - 3e-186)."""
    with _Work(dps) as w:
        return _expm1_q(w, _q(w, er, pi)[0], w.num(s))


def expm_q(er, pi, s, dps=DPS):
    """P = exp(Q s) as nested lists of working-precision numbers (s: a double or a working-precision number)."""
    with _Work(dps) as w:
        Q, _ = _q(w, er, pi)
        E = _expm1_q(w, Q, w.num(s))
        return [[E[i][j] + (1 if i == j else 0) for j in range(4)] for i in range(4)]


# ------------------------------------------------------------------------------------------------------------------------
# discrete-Gamma category means
# ------------------------------------------------------------------------------------------------------------------------
_RATES_CACHE = {}


def _gamma_quantile(a, p):
    """y with P(a, y) = p (regularised lower incomplete gamma), to the working precision; solved in u = log y."""
    mp = _mpm
    lp = mp.log(p)
    f = lambda u: mp.log(mp.gammainc(a, 0, mp.exp(u), regularized=True)) - lp
    # start: the leading term y^a / Gamma(a + 1) for small shapes, Wilson-Hilferty for large ones
    u_small = (lp + mp.loggamma(a + 1)) / a
    z = mp.sqrt(2) * mp.erfinv(2 * p - 1)
    wh = a * (1 - 1 / (9 * a) + z / (3 * mp.sqrt(a))) ** 3
    u0 = u_small if (a < 1 and u_small < mp.log(a / 4)) or wh <= 0 else mp.log(wh)
    step = max(mp.mpf(1) / 8, abs(u0) / 64)
    lo, hi = u0 - step, u0 + step
    while f(lo) > 0:
        lo -= step
        step *= 2
    while f(hi) < 0:
        hi += step
        step *= 2
    u = mp.findroot(f, (lo, hi), solver="illinois", tol=mp.mpf(10) ** (-(mp.mp.dps - 10)), maxsteps=400, verify=False)
    return mp.exp(u)


def gamma_rates_mean(alpha, R, dps=DPS, as_double=True):
    """Means of R equiprobable categories of Gamma(shape alpha, rate alpha).  Exact (mpmath) when RATES_ARE_EXACT, else
    linearham_oracle.gamma_rates_mean's scipy values."""
    if not RATES_ARE_EXACT:         # pragma: no cover
        from oracle import linearham_oracle as orc
        return orc.gamma_rates_mean(alpha, R)
    key = (float(alpha), int(R), dps)
    if key not in _RATES_CACHE:
        with _mpm.workdps(dps + 20):
            a = _mpm.mpf(float(alpha))
            if R == 1:
                out = [_mpm.mpf(1)]
            else:
                ys = [_gamma_quantile(a, _mpm.mpf(k) / R) for k in range(1, R)]
                low = [_mpm.mpf(0)] + [_mpm.gammainc(a + 1, 0, y, regularized=True) for y in ys]
                out = [R * (low[k + 1] - low[k]) for k in range(R - 1)]
                out.append(R * _mpm.gammainc(a + 1, ys[-1], _mpm.inf, regularized=True))
            _RATES_CACHE[key] = out
    out = _RATES_CACHE[key]
    return np.array([float(x) for x in out]) if as_double else out


# ------------------------------------------------------------------------------------------------------------------------
# P-matrices and pruning
# ------------------------------------------------------------------------------------------------------------------------
class ExactModel:
    """One (er, pi, rates) model: caches E = P - I per distinct product t * r.  `rates`: doubles (the values a test wants the
    P-matrices AT, e.g. the oracle's own) or working-precision numbers (gamma_rates_mean(..., as_double=False))."""

    def __init__(self, er, pi, rates, dps=DPS):
        self.dps = dps
        self.rates = list(rates)
        with _Work(dps) as w:
            self.Q, self.pi = _q(w, er, pi)
        self._cache = {}

    def _e(self, w, t, r):
        key = (float(t), r)
        if key not in self._cache:
            self._cache[key] = _expm1_q(w, self.Q, w.num(float(t)) * w.num(self.rates[r]))
        return self._cache[key]

    def p(self, t, r):
        """P(t * rates[r]) at the working precision."""
        with _Work(self.dps) as w:
            E = self._e(w, t, r)
            return [[E[i][j] + (1 if i == j else 0) for j in range(4)] for i in range(4)]

    def pmatrices_double(self, brlens):
        """[len(brlens), R, 4, 4] doubles: what linearham_oracle.gtr_pmatrices returns, correctly rounded."""
        out = np.zeros((len(brlens), len(self.rates), 4, 4))
        for b, t in enumerate(brlens):
            for r in range(len(self.rates)):
                out[b, r] = [[float(x) for x in row] for row in self.p(t, r)]
        return out

    def prune(self, T, children, root, brlen, xmsa, columns, entries=False):
        """Exact per-column likelihoods of the tree in lh_schedule_tree's rooted-at-naive form (tests/desc_builder.py
        tree_arrays): tips 0..T-1 (0 = naive), inner nodes T..2T-3, brlen[v] the branch above node v.
        xmsa [T, C] states 0..3, 4 = N; columns: the xmsa columns wanted.
        Returns dict(emission [n] doubles, log2_emission [n], per_rate_log2 [R, n] (log2 of the unmixed per-rate site
        likelihood, before the division by pi[naive]), node_log2max {inner node: [R, n_patterns]}, pattern_of [n]);
        entries=True adds node_log2 {inner node: [R, n_patterns, 4]}, every entry of the conditional-likelihood vectors
        (entry_window_drop reads them)."""
        R = len(self.rates)
        children = np.asarray(children).reshape(-1, 2)
        with _Work(self.dps) as w:
            one, zero = w.num(1), w.num(0)
            # site patterns of the non-naive rows: the subtree below `root` is shared by the five naive states
            pats, pattern_of = {}, []
            for c in columns:
                pattern_of.append(pats.setdefault(tuple(int(x) for x in xmsa[1:, c]), len(pats)))
            pat_list = sorted(pats, key=pats.get)
            order, stack = [], [int(root)]
            while stack:                       # pre-order; reversed = children first
                v = stack.pop()
                order.append(v)
                stack.extend(int(c) for c in children[v - T] if c >= T)
            root_clv = [[None] * len(pat_list) for _ in range(R)]
            node_log2max = {v: np.zeros((R, len(pat_list))) for v in order}
            node_log2 = {v: np.zeros((R, len(pat_list), 4)) for v in order} if entries else None
            for r in range(R):
                Pm = {}
                for v in range(1, 2 * T - 2):
                    if v != root:
                        E = self._e(w, brlen[v], r)
                        Pm[v] = [[E[i][j] + (one if i == j else zero) for j in range(4)] for i in range(4)]
                rowsum = {v: [sum(P[i]) for i in range(4)] for v, P in Pm.items()}
                for pi_, pat in enumerate(pat_list):
                    clv = {}
                    for v in reversed(order):
                        acc = [one] * 4
                        for c in children[v - T]:
                            c = int(c)
                            if c < T:
                                s = pat[c - 1]
                                m = rowsum[c] if s == 4 else [Pm[c][i][s] for i in range(4)]
                            else:
                                x, P = clv[c], Pm[c]
                                m = [P[i][0] * x[0] + P[i][1] * x[1] + P[i][2] * x[2] + P[i][3] * x[3] for i in range(4)]
                            acc = [acc[i] * m[i] for i in range(4)]
                        clv[v] = acc
                        node_log2max[v][r, pi_] = w.log2(max(acc))
                        if entries:
                            node_log2[v][r, pi_] = [w.log2(x) for x in acc]
                    root_clv[r][pi_] = clv[root]
            # the naive branch: emission(c) = mean_r sum_i pi_i clv_root_i P_naive[i, s] / pi_s   (s = N: row sums, no division)
            n = len(columns)
            em, l2, per_rate = np.zeros(n), np.zeros(n), np.zeros((R, n))
            for k, c in enumerate(columns):
                s = int(xmsa[0, c])
                tot = zero
                for r in range(R):
                    E = self._e(w, brlen[0], r)
                    x = root_clv[r][pattern_of[k]]
                    if s == 4:
                        col = [sum(E[i]) + one for i in range(4)]
                    else:
                        col = [E[i][s] + (one if i == s else zero) for i in range(4)]
                    lr = sum(self.pi[i] * x[i] * col[i] for i in range(4))
                    per_rate[r, k] = w.log2(lr)
                    tot += lr
                tot = tot / R
                if s != 4:
                    tot = tot / self.pi[s]
                em[k], l2[k] = float(tot), w.log2(tot)
        out = {"emission": em, "log2_emission": l2, "per_rate_log2": per_rate, "node_log2max": node_log2max,
               "pattern_of": np.array(pattern_of)}
        if entries:
            out["node_log2"] = node_log2
        return out


def branch_order(tree):
    """The branch lengths in the order linearham_oracle.per_site_loglik hands them to gtr_pmatrices (its pre-order from
    the last inner node): what a substitute for gtr_pmatrices has to index its result by."""
    root = len(tree.adj) - 1
    out, stack = [], [(root, -1, 0.0)]
    while stack:
        node, par, bl = stack.pop()
        if par >= 0:
            out.append(bl)
        for nb, l in tree.adj[node]:
            if nb != par:
                stack.append((nb, node, l))
    return out


def exact_gtr_pmatrices(dps=DPS):
    """A drop-in for linearham_oracle.gtr_pmatrices (monkeypatch it in): the same signature and shape, every matrix the
    exact exp(Q t r) rounded to double.  Matrices are cached across calls by (er, pi, rate, t)."""
    models = {}

    def gtr_pmatrices(er, pi, rates, brlens, small_qt_form=False, plain_exp=False):
        key = (tuple(float(x) for x in er), tuple(float(x) for x in pi), tuple(float(x) for x in rates))
        if key not in models:
            models[key] = ExactModel(er, pi, [float(x) for x in rates], dps)
        return models[key].pmatrices_double(list(brlens))
    return gtr_pmatrices


def op_nodes(T, children, ops):
    """The inner node each op of a lh_schedule_tree schedule computes: the parent of the op's two operands."""
    children = np.asarray(children).reshape(-1, 2)
    parent = {}
    for k, (a, b) in enumerate(children):
        parent[int(a)] = parent[int(b)] = T + k
    ops = np.asarray(ops).reshape(-1, 4)
    out = []
    for op in ops:
        a, b = int(op[1]), int(op[2])
        assert parent[a] == parent[b], "an op's operands are siblings"
        out.append(parent[a])
    return out


def four_op_drop(T, children, ops, node_log2max, window=4, live_within=None):
    """The largest fall, in binades, over `window` consecutive ops of the schedule (K1's assembly walk tests for rescaling
    after every fourth op).  An op multiplies two conditional-likelihood vectors; its own fall is
        log2 max(result) - sum over its inner-node operands of log2 max(operand)        (a tip operand counts 0),
    i.e. what the op takes from the largest entry beyond what its operands had already lost (<= 0), per rate category and
    site pattern; the figure returned is the minimum over categories, patterns and windows of the sum over the window's
    ops -- an upper bound of what any chain of `window` ops can lose between two tests, whether or not the ops feed each other.
    live_within: count only the rate categories whose value at the root is within 2^-live_within of the pattern's best one
    (the categories that reach the mixture; the others vanish from it in any arithmetic).
    node_log2max: ExactModel.prune()'s."""
    children = np.asarray(children).reshape(-1, 2)
    nodes = op_nodes(T, children, ops)
    falls = []
    for v in nodes:
        f = node_log2max[v].copy()
        for c in children[v - T]:
            if c >= T:
                f = f - node_log2max[int(c)]
        falls.append(f)
    falls = np.stack(falls)                                   # [ops, R, patterns]
    at_root = node_log2max[nodes[-1]]
    live = np.ones(at_root.shape, bool) if live_within is None else at_root >= at_root.max(axis=0, keepdims=True) - live_within
    worst = 0.0
    for k in range(len(nodes)):
        worst = min(worst, float(falls[k:k + window].sum(axis=0)[live].min()))
    return worst


def entry_window_drop(T, children, ops, node_log2, window=4, matters_within=60):
    """four_op_drop for EVERY entry of the conditional-likelihood vectors: [ops, R, patterns, 4], for each op k and entry i
    how far entry i of op k's result lies below where the largest entry stood `window` ops earlier,
        (sum over the window's earlier ops of their falls as four_op_drop counts them) + (entry i's own fall in op k),
    an entry's own fall being log2 result_i - sum over the op's inner-node operands of log2 max(operand).

    Why the largest entry is not enough.  A walk that tests for the 2^256 rescaling only after every `window`-th op looks at
    the largest entry (so does K1's assembly walk).  Between two tests the vector is multiplied down unscaled, and an entry
    that lies d binades below the largest reaches the subnormals (2^-1022, bits lost) or zero (2^-1074) when the largest is
    still d binades clear of them.  That smaller entry may be the one the column's best path runs through -- a state that
    is unlikely here and exactly right for the tips joined next -- so the result is finite, plausible and wrong while
    four_op_drop reports a fall far from anything.  A test after every op leaves at most one op's fall between tests.

    Entries that cannot reach the result are nan: every factor still to come is a probability, so an entry contributes at
    most its own value, and one more than 2^-matters_within below the root's largest entry (per category and pattern)
    changes nothing in any arithmetic.  node_log2: ExactModel.prune(..., entries=True)'s."""
    children = np.asarray(children).reshape(-1, 2)
    nodes = op_nodes(T, children, ops)
    top, own = [], []
    for v in nodes:
        below = np.zeros(node_log2[v].shape[:2])
        for c in children[v - T]:
            if c >= T:
                below = below + node_log2[int(c)].max(axis=2)
        top.append(node_log2[v].max(axis=2) - below)
        own.append(node_log2[v] - below[..., None])
    top, own = np.stack(top), np.stack(own)                 # [ops, R, patterns], [ops, R, patterns, 4]
    at_root = node_log2[nodes[-1]].max(axis=2)
    out = np.full(own.shape, np.nan)
    for k, v in enumerate(nodes):
        before = top[max(k - window + 1, 0):k].sum(axis=0)
        fall = before[..., None] + own[k]
        out[k] = np.where(node_log2[v] >= at_root[..., None] - matters_within, fall, np.nan)
    return out
