"""What tests/test_gpu_codon_edges.py and its worker process (tests/codon_edges_worker.py) share: a family as
lh_eval_codon_edges_batch takes it (node_codons_cases.NodeCodonsCase) with the oracle of K15 beside it."""
import numpy as np

from linearham_amd import capi
from tests import ancestral_marginal_oracle as amo
from tests import codon_edge_oracle as ceo
from tests.ancestral_cases import BOUND
from tests.node_codons_cases import NodeCodonsCase

TABLES = ("codon_counts", "aa_counts", "seed_change", "edge_change", "edge_load")


class CodonEdgesCase(NodeCodonsCase):
    def codon_edges(self, pairs, tip, log_offset=None, want=("loglik",) + TABLES, pad=0):
        """lh_eval_codon_edges_batch over (row, seed tip) pairs that share the seed tip; pad: padding slots added to the
        paths' common length."""
        assert all(p[1] == tip for p in pairs)
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        padded = capi.pad_paths(paths)
        if pad:
            padded = np.concatenate([padded, np.full((len(paths), pad), -1, dtype=padded.dtype)], axis=1)
        res = self.hip.eval_codon_edges_batch(self.family, *self.args(rows), padded, tip, log_offset=log_offset, want=want)
        return res, paths

    def given_edges(self, pairs, tip, Q, want=TABLES):
        """lh_asr_codon_edges_batch on the rates of the evaluation."""
        rows = [p[0] for p in pairs]
        a = self.args(rows)
        fam = capi.Family.borrow(self.family, self.hip)
        _, ev = fam.eval_batch(*a, want=("rates",))
        return fam.asr_codon_edges_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], Q,
                                         capi.pad_paths([self.path(*p) for p in pairs]), tip, want=want, n_sites=self.L)

    def oracle_H(self, row, path, tip):
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        pi = np.asarray(r["pi"], dtype=float)
        rates = self.rates(row)
        pre = amo.prepare(children, root, brlen, self.T, self.o.msa, r["er"], pi, rates)
        return ceo.cond_edges(children, root, brlen, self.T, self.o.msa, r["er"], pi, rates, path, tip, pre=pre)


def dirichlet_codons(rng, shape):
    """Naive codon posteriors [shape][125] for the given-rates forms: sparse Dirichlet rows, entries below 1e-3 set to 0."""
    dq = rng.dirichlet(np.ones(125) * 0.05, size=shape)
    dq[dq < 1e-3] = 0.0
    return dq / dq.sum(axis=-1, keepdims=True)


def compare(got, i, want):
    """The largest difference of row i of the device's five tables from the oracle's dict."""
    return max(np.abs(got[k][i] - want[k]).max() for k in TABLES)


def rules(res, paths):
    """What holds whatever the oracle says."""
    for i, p in enumerate(paths):
        n = len(p)
        cc, aa, ec, el = res["codon_counts"][i], res["aa_counts"][i], res["edge_change"][i], res["edge_load"][i]
        P = ec.shape[0] - 1
        assert np.abs(cc.sum(axis=1) - (n + 1)).max() < 1e-11
        assert np.abs(ec[:n].sum(axis=-1) - 1).max() < 1e-12
        assert not ec[n:P].any() and not el[n:P].any()
        assert np.abs(np.trace(aa, axis1=1, axis2=2) - (cc[:, 0] + cc[:, 1])).max() < 1e-11
        assert np.abs(aa.sum(axis=(1, 2)) - aa.trace(axis1=1, axis2=2) - cc[:, 2]).max() < 1e-11
        assert np.array_equal(res["seed_change"][i], ec[0])
        assert np.abs(el - ec[:, :, 1:].sum(axis=1)).max() < 1e-12
        assert np.abs(cc[:, :3] - (ec[:n].sum(axis=0) + ec[P])).max() < 1e-12


def check(c, pairs_by_tip, frames=(0, 1, 2), pad=0):
    """All five tables of every (row, tip) against the oracle, in every frame, one batch per seed tip; the sum rules.
    pairs_by_tip: {tip: [rows]}.  Returns the paths seen."""
    worst = 0.0
    seen = []
    H = {}
    for frame in frames:
        c.set_frame(frame)
        Q = {row: c.naive_codons(row) for row in sorted({r for rows in pairs_by_tip.values() for r in rows})}
        for tip, rows in pairs_by_tip.items():
            pairs = [(r, tip) for r in rows]
            res, paths = c.codon_edges(pairs, tip, pad=pad)
            rules(res, paths)
            P = res["edge_change"].shape[1] - 1
            for i, (row, _) in enumerate(pairs):
                if (row, tip) not in H:
                    H[row, tip] = c.oracle_H(row, paths[i], tip)
                want = ceo.tables(Q[row], H[row, tip], frame, P=P)
                worst = max(worst, compare(res, i, want))
            seen += paths
    print("the five tables: worst difference from the oracle %.3g" % worst)
    assert worst < BOUND, worst
    return seen


def _as_codon_edges(c):
    c.__class__ = CodonEdgesCase
    return c


def synth(hip, tmp_path, **kw):
    from tests import ancestral_probs_cases as apc
    return _as_codon_edges(apc.synth(hip, tmp_path, **kw))


def toy_case(hip, data_dir, tmp_path, R=4):
    from tests import ancestral_probs_cases as apc
    return _as_codon_edges(apc.toy_case(hip, data_dir, tmp_path, R))
