"""CPU restatement (numpy) of the exact ancestral-state marginals along a seed's lineage (K11) -- TEST INFRASTRUCTURE ONLY.

Per node v_s of the lineage path (slot 0 = the seed's parent, last slot = the root, naive's neighbour) and alignment site j
    marg[s][j][c] = sum_b q_j(b) sum_r [lik_r(j, b) / Z_j(b)] P(x_{v_s, j} = c | column j, naive_j = b, rate r)
with q_j the distribution of the naive base (tests/posterior_oracle.site_base gives the HMM's posterior; a one-hot row
conditions on a fixed naive sequence, which is what oracle/asr_oracle.asr_sample draws under), lik_r the column's
likelihood on the tree scaled by rate r and Z_j(b) = sum_r lik_r(j, b).  Built on asr_oracle.upward and
orc.gtr_pmatrices(..., small_qt_form=True), the forms the ancestral sampler's oracle uses.

`marginals` restates the one-down-pass formulas the device uses (linear in the naive tip's vector);
`marginals_by_enumeration` is the brute force they are checked against (tests/test_ancestral_marginal_oracle.py).
Tree form: the C ABI's rooted-at-naive arrays, as in oracle/asr_oracle.py.
"""
import numpy as np

from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc

ONEHOT = np.concatenate([np.eye(4), np.ones((1, 4))], axis=0)


def seed_path(children, root, T, seed_tip):
    """Inner nodes from the tip's parent up to the root."""
    children = np.asarray(children).ravel()
    parent = {int(c): T + i // 2 for i, c in enumerate(children)}
    path, v = [], int(seed_tip)
    while v != root:
        v = parent[v]
        path.append(v)
    return path


def _per_rate(children, root, brlen, T, msa, er, pi, rates):
    """Per rate the CLVs, and the column likelihoods lik[R][L][5] on a common scale per site."""
    msa = np.asarray(msa)
    L = msa.shape[1]
    R = len(rates)
    tips = np.concatenate([np.full((1, L), 4, dtype=msa.dtype), msa], axis=0)   # (the naive tip's row is not read)
    P = orc.gtr_pmatrices(er, pi, rates, brlen, small_qt_form=True)              # [2T-2, R, 4, 4]
    clvs, logscale = [], np.zeros((R, L))
    w = np.zeros((R, L, 5))
    for k in range(R):
        clv, ls, _ = ao.upward(children, root, brlen, T, tips, P[:, k])
        clvs.append(clv)
        logscale[k] = ls
        down = P[0, k] @ ONEHOT.T                                                # [4 (i), 5 (b)]
        w[k] = (pi[None, :] * clv[root]) @ down
    lik = w * np.exp(logscale - logscale.max(axis=0, keepdims=True))[:, :, None]
    return P, clvs, lik


def _weights(lik, q):
    """t[L][5] = q / Z (0 where q is 0, also where Z is 0) and the rate posterior rho[L][R]."""
    Z = lik.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q == 0, 0.0, q / Z)
    rho = np.einsum("lb,rlb->lr", t, lik)
    return t, rho


def prepare(children, root, brlen, T, msa, er, pi, rates):
    """What `marginals` needs of a tree sample whatever the path and q: pass it as `pre` to share it among paths."""
    return _per_rate(np.asarray(children).ravel(), root, brlen, T, msa, er, np.asarray(pi, dtype=float), rates)


def marginals(children, root, brlen, T, msa, q, er, pi, rates, path, pre=None):
    """(marg [P][L][4], rate_post [L][R]) by the formulas of the device: per rate one message from above, passed down
    the path, every table normalised before it is weighted by the rate posterior."""
    children = np.asarray(children).ravel()
    pi = np.asarray(pi, dtype=float)
    q = np.asarray(q, dtype=float)
    P, clvs, lik = pre if pre is not None else _per_rate(children, root, brlen, T, msa, er, pi, rates)
    t, rho = _weights(lik, q)
    L, R = q.shape[0], len(rates)
    assert path[-1] == root
    marg = np.zeros((len(path), L, 4))
    for k in range(R):
        clv = clvs[k]
        A = pi[None, :] * (t @ (P[0, k] @ ONEHOT.T).T)                           # [L][4]
        for s in range(len(path) - 1, -1, -1):
            v = path[s]
            post = A * clv[v]
            tot = post.sum(axis=1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                norm = np.where(tot == 0, 0.0, post / tot)
            marg[s] += np.where(rho[:, k:k + 1] == 0, 0.0, rho[:, k:k + 1] * norm)
            if s == 0:
                break
            kids = [int(c) for c in children[2 * (v - T):2 * (v - T) + 2]]
            below = path[s - 1]
            assert below in kids, "path entry %d is not a child of %d" % (below, v)
            sib = kids[1] if kids[0] == below else kids[0]
            M = A * (clv[sib] @ P[sib, k].T)
            A = M @ P[below, k]
            top = A.max(axis=1, keepdims=True)
            A = A / np.where(top > 0, top, 1.0)
    return marg, rho


def marginals_by_enumeration(children, root, brlen, T, msa, q, er, pi, rates, path):
    """The same tables from asr_oracle.exact_joint_posterior: per (site, naive base, rate) the joint posterior of all
    inner states by enumeration, marginalised per node, mixed over the base with q and over the rate with lik_r / Z.
    Small T only."""
    children = np.asarray(children).ravel()
    pi = np.asarray(pi, dtype=float)
    q = np.asarray(q, dtype=float)
    msa = np.asarray(msa)
    _, _, lik = _per_rate(children, root, brlen, T, msa, er, pi, rates)
    Z = lik.sum(axis=0)
    L, R, I = q.shape[0], len(rates), T - 2
    marg = np.zeros((len(path), L, 4))
    rate_post = np.zeros((L, R))
    for j in range(L):
        for b in range(5):
            if q[j, b] == 0:
                continue
            column = np.concatenate([[b], msa[:, j]])
            for k in range(R):
                wgt = q[j, b] * lik[k, j, b] / Z[j, b]
                rate_post[j, k] += wgt
                if wgt == 0:
                    continue
                joint = ao.exact_joint_posterior(children, root, brlen, T, column, er, pi, rates[k])
                for s, v in enumerate(path):
                    axes = tuple(a for a in range(I) if a != v - T)
                    marg[s, j] += wgt * joint.sum(axis=axes)
    return marg, rate_post

