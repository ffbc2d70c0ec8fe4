"""CPU restatement (numpy) of the exact substitution posteriors along the edges of a seed's lineage (K12) -- TEST
INFRASTRUCTURE ONLY.

For a path v_0 (the seed's parent) .. v_{len-1} (the root, naive's neighbour) of seed tip u, tables indexed
[ancestor state][descendant state] with naive the oldest node:
    edge[s][j][a][c]      = P(x_{v_s, j} = a, x_{below, j} = c | data), below = v_{s-1} for s >= 1, the seed tip for s = 0
    naive_edge[j][b][i]   = P(naive_j = b, x_{root, j} = i | data), b over A, C, G, T, N
    chain_counts[j][a][c] = naive_edge[j][a][c] (a < 4) + sum_s edge[s][j][a][c]
    edge_load[e]          = sum_j of the off-diagonal mass of edge e; e = len(path) is the naive edge (rows b < 4)
mixed over the naive base with q and over the rate with lik_r / Z as tests/ancestral_marginal_oracle.py does.

`edges` restates the device's formulas (per rate one message from above passed down the path, the 16 cells it would sum
over kept) on top of ancestral_marginal_oracle._per_rate and _weights; `edges_by_enumeration` is the brute force from
asr_oracle.exact_joint_posterior they are checked against (tests/test_edge_oracle.py)."""
import numpy as np

from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo

ONEHOT = amo.ONEHOT


def _norm(J, rho_k):
    """J [L][..cells] normalised per site and weighted by rho_k [L]; 0 where the sum or the weight is 0."""
    tot = J.reshape(J.shape[0], -1).sum(axis=1).reshape((-1,) + (1,) * (J.ndim - 1))
    w = rho_k.reshape(tot.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((tot == 0) | (w == 0), 0.0, w * J / tot)


def reductions(edge, naive_edge):
    """(chain_counts [L][4][4], edge_load [P+1]) from edge [P][L][4][4] and naive_edge [L][5][4]."""
    cc = naive_edge[:, :4, :] + edge.sum(axis=0)
    offd = 1.0 - np.eye(4)
    load = np.concatenate([(edge * offd).sum(axis=(1, 2, 3)), [(naive_edge[:, :4, :] * offd).sum()]])
    return cc, load


def edges(children, root, brlen, T, msa, q, er, pi, rates, path, seed_tip, pre=None):
    """dict(edge [P][L][4][4], naive_edge [L][5][4], chain_counts, edge_load [P+1], rate_post [L][R]) by the device's
    formulas."""
    children = np.asarray(children).ravel()
    pi = np.asarray(pi, dtype=float)
    q = np.asarray(q, dtype=float)
    msa = np.asarray(msa)
    P, clvs, lik = pre if pre is not None else amo._per_rate(children, root, brlen, T, msa, er, pi, rates)
    t, rho = amo._weights(lik, q)
    L, R, n = q.shape[0], len(rates), len(path)
    assert path[-1] == root
    kids0 = [int(c) for c in children[2 * (path[0] - T):2 * (path[0] - T) + 2]]
    assert seed_tip in kids0, "tip %d is not a child of %d" % (seed_tip, path[0])
    edge = np.zeros((n, L, 4, 4))
    naive_edge = np.zeros((L, 5, 4))
    tip_vec = ONEHOT[msa[seed_tip - 1]]                                          # [L][4], all ones for N
    for k in range(R):
        clv = clvs[k]
        down = P[0, k] @ ONEHOT.T                                                # [4 (i), 5 (b)]: P_naive[i][b], row sums for N
        Jn = t[:, :, None] * pi[None, None, :] * down.T[None, :, :] * clv[root][:, None, :]
        naive_edge += _norm(Jn, rho[:, k])
        A = pi[None, :] * (t @ down.T)                                           # [L][4]
        for s in range(n - 1, -1, -1):
            v = path[s]
            kids = [int(c) for c in children[2 * (v - T):2 * (v - T) + 2]]
            below = path[s - 1] if s > 0 else seed_tip
            assert below in kids
            sib = kids[1] if kids[0] == below else kids[0]
            M = A * (clv[sib] @ P[sib, k].T)
            Lb = clv[below] if s > 0 else tip_vec
            J = M[:, :, None] * P[below, k][None, :, :] * Lb[:, None, :]
            edge[s] += _norm(J, rho[:, k])
            if s == 0:
                break
            A = M @ P[below, k]
            top = A.max(axis=1, keepdims=True)
            A = A / np.where(top > 0, top, 1.0)
    cc, load = reductions(edge, naive_edge)
    return dict(edge=edge, naive_edge=naive_edge, chain_counts=cc, edge_load=load, rate_post=rho)


def edges_by_enumeration(children, root, brlen, T, msa, q, er, pi, rates, path, seed_tip):
    """The same from asr_oracle.exact_joint_posterior: per (site, naive base, rate) the joint posterior of all inner states
    by enumeration, its pair marginal per edge.  An unobserved seed tip hangs off its parent alone: P(a, c) = post(a)
    P_u[a][c].  Small T only."""
    children = np.asarray(children).ravel()
    pi = np.asarray(pi, dtype=float)
    q = np.asarray(q, dtype=float)
    msa = np.asarray(msa)
    _, _, lik = amo._per_rate(children, root, brlen, T, msa, er, pi, rates)
    Z = lik.sum(axis=0)
    L, R, I, n = q.shape[0], len(rates), T - 2, len(path)
    Pu = orc.gtr_pmatrices(er, pi, rates, brlen)[seed_tip]                       # [R][4][4]
    edge = np.zeros((n, L, 4, 4))
    naive_edge = np.zeros((L, 5, 4))
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

                def node(v):
                    return joint.sum(axis=tuple(a for a in range(I) if a != v - T))

                naive_edge[j, b] += wgt * node(root)
                for s in range(1, n):
                    hi, lo = path[s] - T, path[s - 1] - T
                    pair = joint.sum(axis=tuple(a for a in range(I) if a not in (hi, lo)))
                    edge[s, j] += wgt * (pair if hi < lo else pair.T)
                p0, st = node(path[0]), msa[seed_tip - 1, j]
                if st < 4:
                    edge[0, j, :, st] += wgt * p0
                else:
                    edge[0, j] += wgt * p0[:, None] * Pu[k]
    cc, load = reductions(edge, naive_edge)
    return dict(edge=edge, naive_edge=naive_edge, chain_counts=cc, edge_load=load, rate_post=rate_post)
