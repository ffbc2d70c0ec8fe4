"""CPU restatement (numpy) of the exact codon marginals of a node of a seed's lineage (K14) -- TEST INFRASTRUCTURE ONLY.

Given the naive base of a site the node's base there is independent of everything else, so for codon c over the sites
j1, j2, j3 = frame + 3 c ..
    T[c][x1 x2 x3] = sum_b Q[c][b1 b2 b3] G[j1][b1][x1] G[j2][b2][x2] G[j3][b3][x3]
with Q the naive codon posterior [n_codons][125] (tests/codon_oracle.py, entry 25 b1 + 5 b2 + b3 over A,C,G,T,N) and G
[L][5][4] = P(x_{node,j} = c | column j, naive_j = b) (tests/ancestral_probs_oracle.cond_tables).  The node triple is
indexed 16 x1 + 4 x2 + x3.  `change` folds the joint P(b, x) of a codon by linearham_amd.posterior.change_classes."""
import numpy as np

from linearham_amd import posterior as lp


def codon_G(G, frame, nc):
    """([nc][5][4],) * 3: G at the three sites of every codon."""
    G = np.asarray(G, dtype=np.float64)
    idx = frame + 3 * np.arange(nc)
    return G[idx], G[idx + 1], G[idx + 2]


def joint(Q, G, frame):
    """[nc][125][64]: P(naive triple b, node triple x) per codon."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 5, 5, 5)
    nc = Q.shape[0]
    g1, g2, g3 = codon_G(G, frame, nc)
    return np.einsum("cabd,cax,cby,cdz->cabdxyz", Q, g1, g2, g3).reshape(nc, 125, 64)


def contraction(Q, G, frame):
    """T [nc][64]."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 5, 5, 5)
    g1, g2, g3 = codon_G(G, frame, Q.shape[0])
    return np.einsum("cabd,cax,cby,cdz->cxyz", Q, g1, g2, g3).reshape(Q.shape[0], 64)


def change(Q, G, frame, classes=None):
    """[nc][4]: identical, synonymous, replacement, the naive triple holds an N."""
    cls = lp.change_classes() if classes is None else np.asarray(classes)
    J = joint(Q, G, frame)
    return np.stack([np.where(cls == k, J, 0.0).sum(axis=(1, 2)) for k in range(4)], axis=1)


def site_marginals(T):
    """[nc][3][4]: the three site marginals of every codon's table."""
    t = np.asarray(T).reshape(-1, 4, 4, 4)
    return np.stack([t.sum(axis=(2, 3)), t.sum(axis=(1, 3)), t.sum(axis=(1, 2))], axis=1)


def product_of_marginals(T):
    m = site_marginals(T)
    return np.einsum("cx,cy,cz->cxyz", m[:, 0], m[:, 1], m[:, 2]).reshape(-1, 64)


def triple_candidates(L, frame, c):
    """The 64 candidates constrained at the three sites of codon c (tests/ancestral_probs_oracle.constrained)."""
    from tests import ancestral_probs_oracle as apo
    s0 = frame + 3 * c
    return apo.constrained(L, [s0, s0 + 1, s0 + 2])


def from_sequences(seqs, G, frame):
    """T from codon_oracle.enumerated's (probability, naive sequence) list: each path's node triple distribution is the
    product of G's rows at the bases it writes."""
    G = np.asarray(G, dtype=np.float64)
    L = G.shape[0]
    nc = (L - frame) // 3 if L >= frame else 0
    T = np.zeros((nc, 64))
    for w, seq in seqs:
        b = [lp.BASES.index(ch) for ch in seq]
        for c in range(nc):
            s0 = frame + 3 * c
            T[c] += w * np.einsum("x,y,z->xyz", G[s0, b[s0]], G[s0 + 1, b[s0 + 1]], G[s0 + 2, b[s0 + 2]]).reshape(64)
    return T
