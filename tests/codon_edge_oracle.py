"""CPU restatement (numpy) of the exact amino-acid replacement posteriors along the edges of a seed's lineage (K15) -- TEST
INFRASTRUCTURE ONLY.

Given the naive base b of a site everything at that site is independent of the rest of the alignment, so with
    H[s][j][b][a][c] = P(x_{v_s,j} = a, x_{below,j} = c | column j, naive_j = b)
(tests/edge_oracle.edges for the one-hot naive distribution at b; path, seed tip and `below` as there) and the naive codon
posterior Q [n_codons][125] (tests/codon_oracle.py) the joint of codon c over the sites j1, j2, j3 = frame + 3 c .. at the
two ends of edge s is
    E[s][c][x][y] = sum_b Q[c][b1 b2 b3] H[s][j1][b1][x1][y1] H[s][j2][b2][x2][y2] H[s][j3][b3][x3][y3]
with x = 16 x1 + 4 x2 + x3.  The naive edge is K14's joint at the MRCA (tests/node_codon_oracle.joint with G = sum_c
H[len-1]).  The folds use linearham_amd.posterior.edge_classes / aa_symbols / change_classes."""
import functools

import numpy as np

from linearham_amd import posterior as lp
from tests import edge_oracle as eo
from tests import node_codon_oracle as nco

N_FREE = np.array([25 * (b // 16) + 5 * ((b // 4) % 4) + b % 4 for b in range(64)])  # entry of Q of an N-free triple


def cond_edges(children, root, brlen, T, msa, er, pi, rates, path, seed_tip, pre=None, enumerate_states=False):
    """H [len(path)][L][5][4][4]: five calls of edge_oracle.edges (or edges_by_enumeration), one per naive basis vector."""
    L = np.asarray(msa).shape[1]
    H = np.zeros((len(path), L, 5, 4, 4))
    for b in range(5):
        q = np.zeros((L, 5))
        q[:, b] = 1.0
        if enumerate_states:
            res = eo.edges_by_enumeration(children, root, brlen, T, msa, q, er, pi, rates, path, seed_tip)
        else:
            res = eo.edges(children, root, brlen, T, msa, q, er, pi, rates, path, seed_tip, pre=pre)
        H[:, :, b] = res["edge"]
    return H


def joint(Q, Hs, frame):
    """E_s [nc][64][64] from Q [nc][125] and one slot's H_s [L][5][4][4]."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 5, 5, 5)
    nc = Q.shape[0]
    h1, h2, h3 = nco.codon_G(Hs, frame, nc)  # [nc][5][4][4] each
    return np.einsum("cabd,caxu,cbyv,cdzw->cxyzuvw", Q, h1, h2, h3, optimize=True).reshape(nc, 64, 64)


def joint_from_sequences(seqs, Hs, frame):
    """E_s from codon_oracle.enumerated's (probability, naive sequence) list."""
    Hs = np.asarray(Hs, dtype=np.float64)
    L = Hs.shape[0]
    nc = (L - frame) // 3 if L >= frame else 0
    E = np.zeros((nc, 64, 64))
    for w, seq in seqs:
        b = [lp.BASES.index(ch) for ch in seq]
        for c in range(nc):
            s0 = frame + 3 * c
            E[c] += w * np.einsum("xu,yv,zw->xyzuvw", Hs[s0, b[s0]], Hs[s0 + 1, b[s0 + 1]],
                                  Hs[s0 + 2, b[s0 + 2]]).reshape(64, 64)
    return E


@functools.lru_cache(maxsize=None)
def fold_matrix():
    """[64][21] one-hot: triple -> symbol."""
    sym = lp.aa_symbols()
    F = np.zeros((64, 21))
    F[np.arange(64), sym] = 1.0
    return F


@functools.lru_cache(maxsize=None)
def _classes():
    return lp.edge_classes(), lp.change_classes()


def reduce_edges(E, Jn, P=None):
    """The five tables from E [len][nc][64][64] (inner edges and the seed edge, slot order) and the naive edge's joint Jn
    [nc][125][64]; P >= len pads edge_change and edge_load with zero slots."""
    n, nc = E.shape[:2]
    P = n if P is None else P
    cls, ncls = _classes()
    F = fold_matrix()
    edge_change = np.zeros((P + 1, nc, 3))
    for k in range(3):
        edge_change[:n, :, k] = np.where(cls == k, E, 0.0).sum(axis=(2, 3))
    nchange = np.stack([np.where(ncls == k, Jn, 0.0).sum(axis=(1, 2)) for k in range(4)], axis=1)
    edge_change[P] = nchange[:, :3]
    codon_counts = np.concatenate([edge_change.sum(axis=0), nchange[:, 3:]], axis=1)
    aa = np.einsum("xa,cxy,yb->cab", F, E.sum(axis=0), F, optimize=True) + \
        np.einsum("xa,cxy,yb->cab", F, Jn[:, N_FREE, :], F, optimize=True)
    return dict(codon_counts=codon_counts, aa_counts=aa, seed_change=edge_change[0].copy(), edge_change=edge_change,
                edge_load=edge_change[:, :, 1:].sum(axis=1))


def tables(Q, H, frame, P=None):
    """The five tables of one row from Q [nc][125] and H [len][L][5][4][4]."""
    E = np.stack([joint(Q, H[s], frame) for s in range(H.shape[0])])
    Jn = nco.joint(Q, H[-1].sum(axis=-1), frame)
    return reduce_edges(E, Jn, P)
