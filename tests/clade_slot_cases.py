"""What tests/test_gpu_clade_slot.py's worker process (tests/clade_slot_worker.py) and the CPU tests share: K13 and K14 at a
slot per row (the `_at` entry points) on a family as node_codons_cases.NodeCodonsCase holds it, the oracle's tables at every
slot of a path, and a brute-force clade slot from descendant sets."""
import numpy as np

from linearham_amd import capi
from tests import ancestral_marginal_oracle as amo
from tests.node_codons_cases import NodeCodonsCase

LOG_CAND_BOUND = 2.5e-11   # tests/test_gpu_ancestral_probs.py's bound for log_cand at the two fixed nodes


def descendants(children, T):
    """tips below every node, {node: frozenset}, from `children` [(T-2)*2] alone."""
    children = np.asarray(children).reshape(-1, 2)
    below = {t: frozenset([t]) for t in range(T)}

    def fill(v):
        if v not in below:
            below[v] = fill(int(children[v - T, 0])) | fill(int(children[v - T, 1]))
        return below[v]
    for v in range(T, 2 * T - 2):
        fill(v)
    return below


def brute_clade_slot(children, root, T, seed_tip, with_tips):
    """(path, slot): the seed's ancestors up to the root found by descendant sets, smallest clade first, and the first of
    them that holds every tip of with_tips."""
    below = descendants(children, T)
    onpath = sorted((v for v in range(T, 2 * T - 2) if seed_tip in below[v] and below[v] <= below[root]),
                    key=lambda v: len(below[v]))
    assert onpath and onpath[-1] == root
    slot = next(s for s, v in enumerate(onpath) if all(t in below[v] for t in with_tips))
    return onpath, slot


def random_tree(rng, T):
    """A random binary tree on the tips 1 .. T-1 in lh_schedule_tree's numbering (children [(T-2)*2], root); tip 0, naive,
    hangs above the root and is nobody's child."""
    live, children, nxt = list(range(1, T)), np.zeros((T - 2, 2), dtype=np.int32), T
    while len(live) > 1:
        a, b = rng.choice(len(live), size=2, replace=False)
        children[nxt - T] = (live[a], live[b])
        live = [v for k, v in enumerate(live) if k not in (a, b)] + [nxt]
        nxt += 1
    return children.ravel(), live[0]


class AtCase(NodeCodonsCase):
    def partners(self, row, tip):
        """{partner tip: slot of its common ancestor with `tip` on tip's path} under the row's tree."""
        children, root, _ = self.trees[row]
        return {u: capi.clade_slot(self.T, children, root, tip, [u])[1] for u in range(1, self.T) if u != tip}

    def pick(self, row, tip, kind):
        """A slot of the kind 'first' (0), 'last' (the root) or 'interior' that some partner tip gives; None if none does."""
        n = len(self.path(row, tip))
        ok = {"first": lambda s: s == 0, "last": lambda s: s == n - 1, "interior": lambda s: 0 < s < n - 1}[kind]
        hits = sorted(s for s in self.partners(row, tip).values() if ok(s))
        return hits[len(hits) // 2] if hits else None

    def interior_pairs(self, rows):
        """One (row, tip) with an interior slot per row, the tips spread over the family; ([(row, tip)], [slot])."""
        pairs, slots = [], []
        for i in rows:
            for t in [1 + (3 * i + k) % (self.T - 1) for k in range(self.T - 1)]:
                s = self.pick(i, t, "interior")
                if s is not None:
                    pairs.append((i, t))
                    slots.append(s)
                    break
        return pairs, slots

    def probs_at(self, pairs, slots, cands=None, log_offset=None, want=("loglik", "cond", "log_cand")):
        if cands is not None:
            self.hip.set_ancestral_candidates(self.family, cands)
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        res = self.hip.eval_ancestral_candidates_at_batch(self.family, *self.args(rows), capi.pad_paths(paths), slots,
                                                          log_offset=log_offset, want=want)
        return res, paths

    def node_codons_at(self, pairs, slots, log_offset=None, want=("loglik", "codons", "change")):
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        res = self.hip.eval_node_codons_at_batch(self.family, *self.args(rows), capi.pad_paths(paths), slots,
                                                 log_offset=log_offset, want=want)
        return res, paths

    def given_at(self, pairs, slots, Q, want=("codons", "change")):
        rows = [p[0] for p in pairs]
        a = self.args(rows)
        fam = capi.Family.borrow(self.family, self.hip)
        _, ev = fam.eval_batch(*a, want=("rates",))
        return fam.asr_node_codons_at_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], Q,
                                            capi.pad_paths([self.path(*p) for p in pairs]), slots, want=want)

    def tables_at(self, row, path):
        """The oracle's G at every slot of the path, [P][L][5][4]: ancestral_probs_oracle.cond_tables without its choice
        of the slot."""
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        er, pi, rates = r["er"], np.asarray(r["pi"], dtype=float), self.rates(row)
        pre = amo.prepare(children, root, brlen, self.T, self.o.msa, er, pi, rates)
        G = np.zeros((len(path), self.L, 5, 4))
        for b in range(5):
            q = np.zeros((self.L, 5))
            q[:, b] = 1.0
            marg, _ = amo.marginals(children, root, brlen, self.T, self.o.msa, q, er, pi, rates, path, pre=pre)
            G[:, :, b] = marg[:len(path)]
        return G


def synth(hip, tmp_path, **kw):
    from tests import node_codons_cases as ncc
    c = ncc.synth(hip, tmp_path, **kw)
    c.__class__ = AtCase
    return c


def toy_case(hip, data_dir, tmp_path, R=4):
    from tests import node_codons_cases as ncc
    c = ncc.toy_case(hip, data_dir, tmp_path, R)
    c.__class__ = AtCase
    return c
