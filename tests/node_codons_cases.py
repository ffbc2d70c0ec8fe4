"""What tests/test_gpu_node_codons.py and its worker process (tests/node_codons_worker.py) share: a family as
lh_eval_node_codons_batch takes it (ancestral_probs_cases.ProbsCase) with the oracle of K14 beside it."""
import numpy as np

from linearham_amd import capi
from tests import codon_oracle as co
from tests import node_codon_oracle as nco
from tests.ancestral_cases import BOUND
from tests.ancestral_probs_cases import MRCA, PARENT, ProbsCase

NODES = (PARENT, MRCA)
HAS_N = np.array([4 in (i // 25, (i // 5) % 5, i % 5) for i in range(125)])


class NodeCodonsCase(ProbsCase):
    frame = None

    def set_frame(self, frame):
        self.lay = self.hip.set_codons(self.family, frame)
        self.frame = frame
        return self.lay

    def node_codons(self, pairs, node, log_offset=None, want=("loglik", "codons", "change")):
        """lh_eval_node_codons_batch over (row, seed tip) pairs."""
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        res = self.hip.eval_node_codons_batch(self.family, *self.args(rows), capi.pad_paths(paths), node,
                                              log_offset=log_offset, want=want)
        return res, paths

    def given(self, pairs, node, Q, want=("codons", "change")):
        """lh_asr_node_codons_batch on the rates of the evaluation."""
        rows = [p[0] for p in pairs]
        a = self.args(rows)
        fam = capi.Family.borrow(self.family, self.hip)
        _, ev = fam.eval_batch(*a, want=("rates",))
        return fam.asr_node_codons_batch(a[0], a[1], a[2], a[3], a[4], a[5], ev["rates"], Q,
                                         capi.pad_paths([self.path(*p) for p in pairs]), node, want=want)

    def naive_codons(self, row):
        """The oracle's Q of a row in the frame set (the row's parameters are left set on the oracle object)."""
        self.set_row(row)
        return co.dense(self.o, self.frame)[0]

    def oracle_node(self, Q, row, path, node):
        G = self.oracle_tables(row, path, node)
        return nco.contraction(Q, G, self.frame), nco.change(Q, G, self.frame)


def check(c, pairs, frames=(0, 1, 2)):
    """codons and change of both nodes against the oracle, in every frame; the sum rules; rows whose chain has one node give
    the same bits at both nodes.  Returns the paths."""
    worst = 0.0
    for frame in frames:
        c.set_frame(frame)
        Q = {row: c.naive_codons(row) for row in sorted({p[0] for p in pairs})}
        got = {}
        for node in NODES:
            res, paths = c.node_codons(pairs, node)
            got[node] = res
            assert np.abs(res["codons"].sum(axis=-1) - 1).max() < 1e-12
            assert np.abs(res["change"].sum(axis=-1) - 1).max() < 1e-12
            for i, (row, _) in enumerate(pairs):
                T, ch = c.oracle_node(Q[row], row, paths[i], node)
                worst = max(worst, np.abs(res["codons"][i] - T).max(), np.abs(res["change"][i] - ch).max())
        for i, p in enumerate(paths):
            if len(p) == 1:
                for k in ("codons", "change"):
                    assert np.array_equal(got[PARENT][k][i], got[MRCA][k][i])
    print("codons, change: worst difference from the oracle %.3g" % worst)
    assert worst < BOUND, worst
    return paths


def _as_node_codons(c):
    c.__class__ = NodeCodonsCase  # (ProbsCase with K14's calls and oracle beside K13's)
    return c


def synth(hip, tmp_path, **kw):
    from tests import ancestral_probs_cases as apc
    return _as_node_codons(apc.synth(hip, tmp_path, **kw))


def toy_case(hip, data_dir, tmp_path, R=4):
    from tests import ancestral_probs_cases as apc
    return _as_node_codons(apc.toy_case(hip, data_dir, tmp_path, R))
