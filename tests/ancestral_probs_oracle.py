"""CPU restatement (numpy) of the exact posterior probabilities of candidate ancestral sequences (K13) -- TEST
INFRASTRUCTURE ONLY.

For a tree sample t, a node v of the seed's lineage path and a candidate x of L bytes (0..3 = A, C, G, T; 4 = the site is
left open)
    P(X_v = x | data, t) = sum_paths prior(path) prod_j E_t[b_j, j] G_t[j][b_j][x_j] / P(data | t)
with b_j the naive base the path writes on site j, E_t the xMSA emission and
    G_t[j][b][c] = P(x_{v,j} = c | column j, naive_j = b),
tests/ancestral_marginal_oracle.marginals for the one-hot naive distribution at b.  The sum over paths is the oracle's own
forward sweep (oracle/linearham_oracle.PhyloHMM) over xmsa_emission multiplied column by column through xmsa_ids.
"""
import numpy as np

from tests import ancestral_marginal_oracle as amo

OPEN = 4
PARENT, MRCA = 0, 1          # the C ABI's `node`: slot 0 and the last slot of the path


def slot_of(node, path):
    return 0 if node == PARENT else len(path) - 1


def cond_tables(children, root, brlen, T, msa, er, pi, rates, path, node, pre=None):
    """G [L][5][4] at the node: five calls of amo.marginals, one per naive basis vector."""
    L = np.asarray(msa).shape[1]
    if pre is None:
        pre = amo.prepare(children, root, brlen, T, msa, er, pi, rates)
    G = np.zeros((L, 5, 4))
    for b in range(5):
        q = np.zeros((L, 5))
        q[:, b] = 1.0
        marg, _ = amo.marginals(children, root, brlen, T, msa, q, er, pi, rates, path, pre=pre)
        G[:, b] = marg[slot_of(node, path)]
    return G


def _sweep(o, em):
    o.xmsa_emission = em
    o.vgerm_scaler_count = o.dgerm_scaler_count = o.jgerm_scaler_count = 0
    o._initialize_emission()
    o.cache_forward = True
    return o.log_likelihood()


def modified_emission(o, base, G, x):
    em = base.copy()
    for (b, site), xi in o.xmsa_ids.items():
        if x[site] != OPEN:
            em[xi] *= G[site, b, x[site]]
    return em


def log_candidates(o, G, cands):
    """log P(X_v = x_k | data, t) [K] for an oracle PhyloHMM `o` whose phylogenetic parameters and emissions are set
    (initialize_phylo_parameters, initialize_phylo_emission); its emissions are put back afterwards."""
    base = o.xmsa_emission.copy()
    ll0 = _sweep(o, base)
    out = np.array([_sweep(o, modified_emission(o, base, G, np.asarray(x))) - ll0 for x in cands])
    _sweep(o, base)
    return out


def one_site(L, site):
    """The four candidates constrained at `site` alone."""
    c = np.full((4, L), OPEN, dtype=np.uint8)
    c[np.arange(4), site] = np.arange(4)
    return c


def constrained(L, sites):
    """The 4^len(sites) candidates constrained at `sites`, the first site the slowest index."""
    k = len(sites)
    c = np.full((4 ** k, L), OPEN, dtype=np.uint8)
    for i in range(4 ** k):
        for s, site in enumerate(sites):
            c[i, site] = (i // 4 ** (k - 1 - s)) % 4
    return c
