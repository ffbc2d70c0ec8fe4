"""EXACT REFERENCE OF THE LINEAGE TABLES (K11, K12, K13b) -- TEST INFRASTRUCTURE ONLY.

tests/exact_model_oracle.ExactModel's arithmetic (mpmath at its working precision, exact P-matrices, NO rescaling anywhere:
the exponent range is unbounded) carried through what tests/ancestral_marginal_oracle.py, tests/edge_oracle.py and
tests/ancestral_probs_oracle.py restate in doubles.  Per rate category r and alignment column it computes the upward
conditional-likelihood vectors of every inner node and, along a seed path v_0 (the seed's parent) .. v_{P-1} (the root,
naive's neighbour), the message from above A_s for each of the five naive bases b (A, C, G, T, N):
    A_{P-1}[i] = pi_i P_naive[i][b]            (N: the row sum)
    A_{s-1}    = (A_s o m_s)^T P_below         m_s = P_sib CLV_sib, the message of v_s's child off the path
so that
    joint_r(b; x_{v_s} = c)               = A_s[c] CLV_{v_s}[c]
    joint_r(b; x_{v_s} = a, x_below = c)  = (A_s o m_s)[a] P_below[a][c] L_below[c]        (L: CLV, or the seed tip's column)
    lik_r(b)                              = sum_c joint_r(b; x_root = c)
Everything the kernels emit is a ratio of such sums with Z(b) = sum_r lik_r(b) -- a probability, which a double holds:
    cond[s][j][b][c]      = sum_r joint_r(b; x_{v_s} = c) / Z(b)                 K13b's five-basis conditional tables
    cond_edge[s][j][b]    = sum_r joint_r(b; a, c) / Z(b)                        [4][4], [ancestor][descendant]
    rate[j][b][r]         = lik_r(b) / Z(b)
and with a naive-base distribution q [L][5]
    marg[s][j]      = sum_b q_j(b) cond[s][j][b]                                 K11
    edge[s][j]      = sum_b q_j(b) cond_edge[s][j][b]                            K12
    naive_edge[j][b]= q_j(b) cond[P-1][j][b]
    rate_post[j]    = sum_b q_j(b) rate[j][b]
(the mixing over b is done in doubles: at most five terms of probabilities).  The device normalises per rate and weights by
the rate posterior, the double-precision oracles do the same; in exact arithmetic both equal the formulas above, because the
normaliser of rate r's table is lik_r(b) itself.

Columns with the same tip states share their tables; a column whose tips are all N is served like any other.
Tree form: the C ABI's rooted-at-naive arrays (tests/desc_builder.tree_arrays)."""
import numpy as np

from tests import exact_model_oracle as ex


class ExactLineage:
    """The upward pass of one tree sample over the distinct columns of msa [T-1][L] (tip states 0..3, 4 = N), once;
    tables(path, seed_tip) then costs one downward pass per distinct column."""

    def __init__(self, model, T, children, root, brlen, msa):
        self.model, self.T, self.root = model, int(T), int(root)
        self.children = np.asarray(children).reshape(-1, 2)
        self.brlen = np.asarray(brlen, dtype=float)
        msa = np.asarray(msa)
        pats, self.pattern_of = {}, []
        for j in range(msa.shape[1]):
            self.pattern_of.append(pats.setdefault(tuple(int(x) for x in msa[:, j]), len(pats)))
        self.pattern_of = np.array(self.pattern_of)
        self.patterns = sorted(pats, key=pats.get)
        self.R = len(model.rates)
        with ex._Work(model.dps) as w:
            one, zero = w.num(1), w.num(0)
            self.P = []                                           # [r]{node: 4x4}
            for r in range(self.R):
                Pm = {}
                for v in range(0, 2 * self.T - 2):
                    if v != self.root:
                        E = model._e(w, self.brlen[v], r)
                        Pm[v] = [[E[i][j] + (one if i == j else zero) for j in range(4)] for i in range(4)]
                self.P.append(Pm)
            order, stack = [], [self.root]
            while stack:
                v = stack.pop()
                order.append(v)
                stack.extend(int(c) for c in self.children[v - self.T] if c >= self.T)
            self.clv = [[None] * len(self.patterns) for _ in range(self.R)]      # [r][pattern]{inner node: [4]}
            for r in range(self.R):
                for p, pat in enumerate(self.patterns):
                    clv = {}
                    for v in reversed(order):
                        acc = [one] * 4
                        for c in self.children[v - self.T]:
                            m = self._message(r, clv, pat, int(c))
                            acc = [acc[i] * m[i] for i in range(4)]
                        clv[v] = acc
                    self.clv[r][p] = clv

    def _tip_vec(self, pat, tip, one, zero):
        s = pat[tip - 1]
        return [one] * 4 if s == 4 else [one if i == s else zero for i in range(4)]

    def _message(self, r, clv, pat, c):
        """P_c L_c: what child c tells its parent."""
        P = self.P[r][c]
        if c < self.T:
            s = pat[c - 1]
            return [sum(P[i]) for i in range(4)] if s == 4 else [P[i][s] for i in range(4)]
        x = clv[c]
        return [P[i][0] * x[0] + P[i][1] * x[1] + P[i][2] * x[2] + P[i][3] * x[3] for i in range(4)]

    def tables(self, path, seed_tip):
        """dict(cond [P][L][5][4], cond_edge [P][L][5][4][4], rate [L][5][R]) as doubles (module docstring)."""
        path = [int(v) for v in path]
        assert path[-1] == self.root
        n, NP, R, T = len(path), len(self.patterns), self.R, self.T
        cond, cedge, rate = np.zeros((n, NP, 5, 4)), np.zeros((n, NP, 5, 4, 4)), np.zeros((NP, 5, R))
        with ex._Work(self.model.dps) as w:
            one, zero = w.num(1), w.num(0)
            pi = self.model.pi
            for p, pat in enumerate(self.patterns):
                node = [[None] * 5 for _ in range(R)]             # [r][b][s][c]
                pair = [[None] * 5 for _ in range(R)]             # [r][b][s][a][c]
                lik = [[None] * 5 for _ in range(R)]
                for r in range(R):
                    clv, Pn = self.clv[r][p], self.P[r][0]
                    # the messages off the path and the factors below do not depend on the naive base
                    sib_m, below_P, below_L = [], [], []
                    for s, v in enumerate(path):
                        kids = [int(c) for c in self.children[v - T]]
                        below = path[s - 1] if s > 0 else int(seed_tip)
                        assert below in kids, "path entry %d is not a child of %d" % (below, v)
                        sib = kids[1] if kids[0] == below else kids[0]
                        sib_m.append(self._message(r, clv, pat, sib))
                        below_P.append(self.P[r][below])
                        below_L.append(clv[below] if below >= T else self._tip_vec(pat, below, one, zero))
                    for b in range(5):
                        A = [pi[i] * (sum(Pn[i]) if b == 4 else Pn[i][b]) for i in range(4)]
                        nt, pt = [None] * n, [None] * n
                        for s in range(n - 1, -1, -1):
                            x = clv[path[s]]
                            nt[s] = [A[c] * x[c] for c in range(4)]
                            M = [A[a] * sib_m[s][a] for a in range(4)]
                            Pb, Lb = below_P[s], below_L[s]
                            pt[s] = [[M[a] * Pb[a][c] * Lb[c] for c in range(4)] for a in range(4)]
                            A = [M[0] * Pb[0][c] + M[1] * Pb[1][c] + M[2] * Pb[2][c] + M[3] * Pb[3][c] for c in range(4)]
                        node[r][b], pair[r][b] = nt, pt
                        lik[r][b] = sum(nt[n - 1])
                for b in range(5):
                    Z = sum(lik[r][b] for r in range(R))
                    for r in range(R):
                        rate[p, b, r] = float(lik[r][b] / Z)
                    for s in range(n):
                        for a in range(4):
                            cond[s, p, b, a] = float(sum(node[r][b][s][a] for r in range(R)) / Z)
                            for c in range(4):
                                cedge[s, p, b, a, c] = float(sum(pair[r][b][s][a][c] for r in range(R)) / Z)
        po = self.pattern_of
        return dict(cond=cond[:, po], cond_edge=cedge[:, po], rate=rate[po])

    def per_rate_log2(self, path_tables=None):
        """log2 lik_r(b) [R][L][5] of the columns (what decides which category is live)."""
        out = np.zeros((self.R, len(self.patterns), 5))
        with ex._Work(self.model.dps) as w:
            pi = self.model.pi
            for r in range(self.R):
                Pn = self.P[r][0]
                for p in range(len(self.patterns)):
                    x = self.clv[r][p][self.root]
                    for b in range(5):
                        out[r, p, b] = w.log2(sum(pi[i] * (sum(Pn[i]) if b == 4 else Pn[i][b]) * x[i] for i in range(4)))
        return out[:, self.pattern_of]


def mix(tables, q):
    """dict(marg [P][L][4], edge [P][L][4][4], naive_edge [L][5][4], chain_counts [L][4][4], edge_load [P+1],
    rate_post [L][R]) of ExactLineage.tables for the naive-base distribution q [L][5]."""
    q = np.asarray(q, dtype=float)
    cond, cedge, rate = tables["cond"], tables["cond_edge"], tables["rate"]
    marg = np.einsum("lb,slbc->slc", q, cond)
    edge = np.einsum("lb,slbac->slac", q, cedge)
    naive_edge = q[:, :, None] * cond[-1]
    cc = naive_edge[:, :4, :] + edge.sum(axis=0)
    offd = 1.0 - np.eye(4)
    load = np.concatenate([(edge * offd).sum(axis=(1, 2, 3)), [(naive_edge[:, :4, :] * offd).sum()]])
    return dict(marg=marg, edge=edge, naive_edge=naive_edge, chain_counts=cc, edge_load=load,
                rate_post=np.einsum("lb,lbr->lr", q, rate))
