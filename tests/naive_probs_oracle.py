"""Test-side restatement of K6 (posterior probabilities of whole naive sequences) on the oracle HMM's dense matrices.

Two forms of P(s | data, t) for a naive sequence s, both from oracle.linearham_oracle.HMM's members (the oracle itself
is imported, not changed):
  by_enumeration  every non-zero-probability state path (tests/posterior_oracle.py's chain), grouped by the naive
                  sequence it writes;
  factorised      P_HMM(s) * prod_i E[s_i, i] / L, with P_HMM(s) the forward sweep over the same chain with every
                  emission replaced by the indicator that the state's naive base is s's base at the state's site
                  (constrained_log_prior) -- what K6a computes on the device."""
import math

import numpy as np

from tests import posterior_oracle as po


def _germ_writes(h, region, padding):
    """Per gene of a germline region (state order), the (site, base) pairs its state writes, padding included."""
    R = getattr(h, region)
    P = getattr(h, padding) if padding else None
    out = []
    for name in (sorted(R.ggene_ranges) if region == "vgerm" else R.state_strs):  # posterior_oracle._chain's orders
        w = []
        for Q in ([R] + ([P] if P is not None else [])):
            if name not in Q.ggene_ranges:
                continue
            rs, re_ = Q.ggene_ranges[name]
            w += [(Q.site_inds[k], Q.naive_bases[k]) for k in range(rs, re_)]
        out.append(w)
    return out


def _junction_site0(h, name):
    return h.flexbounds["v_r"][0] if name == "vd_junction" else h.flexbounds["d_r"][0]


def row_writes(h):
    """For every row of posterior_oracle's chain, per state, the (site, base) pairs it writes (a junction state writes
    its base on the row's site)."""
    rows = po._rows(*po._chain(h))
    germ = {"vgerm": _germ_writes(h, "vgerm", "vpadding"), "jgerm": _germ_writes(h, "jgerm", "jpadding")}
    if h.locus == "igh":
        germ["dgerm"] = _germ_writes(h, "dgerm", None)
    out = []
    for name, i, e, _ in rows:
        if i is None:
            out.append(germ[name])
        else:
            J = getattr(h, name)
            site = _junction_site0(h, name) + i
            out.append([[(site, J.naive_bases[k])] for k in range(len(e))])
    return rows, out


def by_enumeration(h):
    """{naive sequence (tuple of 0..4): P(s | data, t)} from every state path; sites no state writes stay N."""
    rows, writes = row_writes(h)
    L = h.msa.shape[1]
    n = len(rows)
    acc = {}

    def rec(t, k, w, seq):
        seq = list(seq)
        for site, b in writes[t][k]:
            seq[site] = b
        if t == n - 1:
            key = tuple(seq)
            acc[key] = acc.get(key, 0.0) + w
            return
        _, _, e1, T1 = rows[t + 1]
        for k2 in np.nonzero(T1[k] * e1)[0]:
            rec(t + 1, k2, w * T1[k, k2] * e1[k2], seq)

    e0 = rows[0][2]
    for k in np.nonzero(e0)[0]:
        rec(0, k, e0[k], [4] * L)
    total = sum(acc.values())
    return {s: w / total for s, w in acc.items()}


def _indicator_chain(h, s):
    """posterior_oracle's chain with every emission replaced by the indicator of s (plain values, no scaling); s = None:
    every indicator 1, the prior chain over all state paths."""
    s = None if s is None else np.asarray(s)
    rows, writes = row_writes(h)

    def ind(ws):
        return 1.0 if s is None else float(all(s[site] == b for site, b in ws))

    igh = h.locus == "igh"
    nv = len(h.vgerm.state_strs)
    v0 = np.zeros(nv)
    for i, gname in enumerate(sorted(h.vgerm.ggene_ranges)):
        rs, re_ = h.vgerm.ggene_ranges[gname]
        gg = h.ggenes[gname]
        gis = h.vgerm.germ_inds[rs]
        v0[i] = gg.gene_prob * h.vpadding_transition[i] * np.prod(gg.transition[gis:gis + (re_ - rs - 1)])
    out = []
    for t, (name, i, e, T) in enumerate(rows):
        w = np.array([ind(x) for x in writes[t]])
        if name == "vgerm":
            v = v0 * w
        elif name == "jgerm":
            v = h.jpadding_transition * w
        elif i is None:
            v = w
        else:
            v = w * (getattr(h, name + "_xmsa_inds")[i] >= 0)  # the state exists on this row
        out.append((v, T))
    assert igh or len(out) == len(rows)
    return out


def constrained_log_prior(h, s):
    """log P_HMM(s): the forward sweep over the chain with indicator emissions (-inf: no path writes s)."""
    chain = _indicator_chain(h, s)
    a = None
    c = 0.0
    for v, T in chain:
        a = v.copy() if T is None else (a @ T) * v
        z = a.sum()
        if z == 0.0:
            return -math.inf
        c += math.log(z)
        a = a / z
    return c


def log_prior_mass(h):
    """log of the total probability of every state path (the prior chain's forward sweep): the normaliser of
    prior_draws' frequencies, P(draw = s) = exp(constrained_log_prior(s) - log_prior_mass)."""
    c = 0.0
    a = None
    for v, T in _indicator_chain(h, None):
        a = v.copy() if T is None else (a @ T) * v
        z = a.sum()
        c += math.log(z)
        a = a / z
    return c


def prior_draws(h, n, rng):
    """n naive sequences [n][L] (uint8, A,C,G,T,N = 0..4) drawn from the HMM's prior over state paths: forward filtering
    and backward sampling on _indicator_chain's chain with every indicator 1, then the path's writes (sites no state
    writes stay N).  Every draw is written by a path of non-zero probability, so its constrained_log_prior is finite."""
    chain = _indicator_chain(h, None)
    _, writes = row_writes(h)
    alphas = []
    a = None
    for v, T in chain:
        a = v.copy() if T is None else (a @ T) * v
        a = a / a.sum()
        alphas.append(a)

    def draw(p):  # one state per column of p [S][n] (columns unnormalised), by inverse CDF
        cum = np.cumsum(p, axis=0)
        u = rng.random(p.shape[1]) * cum[-1]
        return np.minimum((cum <= u[None, :]).sum(axis=0), p.shape[0] - 1)

    path = [None] * len(chain)
    path[-1] = draw(np.repeat(alphas[-1][:, None], n, axis=1))
    for t in range(len(chain) - 2, -1, -1):
        T = chain[t + 1][1]
        path[t] = draw(alphas[t][:, None] * T[:, path[t + 1]])
    L = h.msa.shape[1]
    out = np.full((n, L), 4, dtype=np.uint8)
    for t, ks in enumerate(path):
        for k in np.unique(ks):
            w = writes[t][k]
            if w:
                sites, bases = zip(*w)
                out[np.ix_(ks == k, np.asarray(sites))] = np.asarray(bases, dtype=np.uint8)
    return out


def candidate_layout(msa, seqs):
    """Host restatement of K6b's tables (lh_candidates_layout): (V, n_lem, n_vlem) for candidates seqs [K][L] on an
    alignment msa [N][L].  A (site, base) pair's u-column is its (alignment column pattern, base) pair -- two sites
    with identical columns share it (lh_family_create) -- so V = the sites where the candidates do not all agree,
    n_vlem = the distinct (pattern, base) pairs over the variable sites and every candidate, n_lem = those and the
    agreeing sites' (pattern, base) pairs together."""
    msa, seqs = np.asarray(msa), np.asarray(seqs)
    pats = {}
    pat = np.array([pats.setdefault(msa[:, i].tobytes(), len(pats)) for i in range(msa.shape[1])])
    var = np.nonzero((seqs != seqs[:1]).any(axis=0))[0]
    vpairs = {(int(pat[i]), int(b)) for i in var for b in np.unique(seqs[:, i])}
    agree = np.setdiff1d(np.arange(msa.shape[1]), var)
    apairs = {(int(pat[i]), int(seqs[0, i])) for i in agree}
    return len(var), len(vpairs | apairs), len(vpairs)


def gather_slots(msa, seqs):
    """lh_family_set_candidates' gather table, restated: (slots, idx) with slots the variable sites' (pattern, base)
    pairs in the order K6b's LDS row holds them (variable sites in site order, candidates in order, first appearance)
    and idx [V][K] each (variable site, candidate)'s slot."""
    msa, seqs = np.asarray(msa), np.asarray(seqs)
    pats = {}
    pat = np.array([pats.setdefault(msa[:, i].tobytes(), len(pats)) for i in range(msa.shape[1])])
    var = np.nonzero((seqs != seqs[:1]).any(axis=0))[0]
    pos, slots = {}, []
    idx = np.zeros((len(var), len(seqs)), dtype=np.int64)
    for v, i in enumerate(var):
        for k in range(len(seqs)):
            key = (int(pat[i]), int(seqs[k, i]))
            if key not in pos:
                pos[key] = len(slots)
                slots.append((int(i), int(seqs[k, i])))  # (a site with that pattern, base)
            idx[v, k] = pos[key]
    return var, slots, idx


def log_emission_sums(h, seqs):
    """log_emission_sum for every row of seqs [K][L] at once."""
    seqs = np.asarray(seqs)
    L = seqs.shape[1]
    with np.errstate(divide="ignore"):
        le = np.append(np.log(h.xmsa_emission), -math.inf)
    ids = np.full((5, L), len(le) - 1)
    for (b, i), x in h.xmsa_ids.items():
        ids[b, i] = x
    return le[ids[seqs, np.arange(L)[None, :]]].sum(axis=1)


def log_emission_sum(h, s):
    """sum_i log E[s_i, i] over the alignment's sites, from the oracle's xMSA emissions (-inf: no such column)."""
    tot = 0.0
    for i, b in enumerate(s):
        x = h.xmsa_ids.get((int(b), i))
        if x is None or h.xmsa_emission[x] == 0.0:
            return -math.inf
        tot += math.log(h.xmsa_emission[x])
    return tot


def log_cand(h, s, loglik=None):
    """log P(s | data, t), factorised."""
    ll = h.log_likelihood() if loglik is None else loglik
    lp = constrained_log_prior(h, s)
    if lp == -math.inf:
        return -math.inf
    return lp + log_emission_sum(h, s) - ll


def site_marginals(probs, L):
    """[L][5] per-site distribution of the naive base under {sequence: probability}."""
    sb = np.zeros((L, 5))
    for s, p in probs.items():
        sb[np.arange(L), np.asarray(s)] += p
    return sb
