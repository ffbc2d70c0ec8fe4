"""What tests/test_gpu_edges.py and its worker process (tests/edges_worker.py) share: tests/ancestral_cases.py's families
with K12's calls and oracle on top.  lh_asr_edges_batch takes one seed tip per call, so a list of (row, seed tip) pairs runs
as one call per tip, every row with that tip in one batch."""
import numpy as np

from linearham_amd import capi
from tests import edge_oracle as eo
from tests.ancestral_cases import BOUND, Case, EvalCase

TABLES = ("edge", "naive_edge", "chain_counts", "edge_load", "rate_post")


def by_tip(pairs):
    """{tip: positions in `pairs`} in the order the tips first appear."""
    groups = {}
    for i, (_, tip) in enumerate(pairs):
        groups.setdefault(tip, []).append(i)
    return groups


class EdgeCase(Case):
    def call(self, rows, tip, q, want=TABLES):
        """One lh_asr_edges_batch call: `rows` with seed tip `tip`.  Returns (dict of want, paths)."""
        paths = [self.path(r, tip) for r in rows]
        res = self.fam.asr_edges_batch(
            self.T, self.depth, np.stack([self.ops[i] for i in rows]), np.stack([self.trees[i][2] for i in rows]),
            [self.rows[i]["er"] for i in rows], [self.rows[i]["pi"] for i in rows], self.rates[rows],
            np.stack([q[i] for i in rows]), capi.pad_paths(paths), tip, want=want)
        return res, paths

    def edge_oracle(self, row, q, path, tip):
        from tests import ancestral_marginal_oracle as amo
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        if row not in self._pre:
            self._pre[row] = amo.prepare(children, root, brlen, self.T, self.h.msa, r["er"], r["pi"], self.rates[row])
        return eo.edges(children, root, brlen, self.T, self.h.msa, q, r["er"], np.asarray(r["pi"]), self.rates[row], path, tip,
                        pre=self._pre[row])

    def check_edges(self, pairs, q):
        """Every pair against the oracle; chain_counts' sum rule; zeros in the padding slots.  Returns per pair
        (dict of the pair's tables, path)."""
        out = [None] * len(pairs)
        worst = 0.0
        for tip, where in by_tip(pairs).items():
            rows = [pairs[i][0] for i in where]
            res, paths = self.call(rows, tip, q)
            for k, i in enumerate(where):
                n = len(paths[k])
                want = self.edge_oracle(rows[k], q[rows[k]], paths[k], tip)
                got = {key: res[key][k] for key in TABLES}
                worst = max(worst, np.abs(got["edge"][:n] - want["edge"]).max(),
                            np.abs(got["naive_edge"] - want["naive_edge"]).max(),
                            np.abs(got["chain_counts"] - want["chain_counts"]).max(),
                            np.abs(got["rate_post"] - want["rate_post"]).max())
                load = np.concatenate([got["edge_load"][:n], got["edge_load"][-1:]])
                worst = max(worst, np.abs(load - want["edge_load"]).max())
                assert not got["edge"][n:].any() and not got["edge_load"][n:-1].any(), pairs[i]
                cells = got["chain_counts"].sum(axis=(-1, -2))
                assert np.abs(cells - (n + 1 - q[rows[k]][:, 4])).max() < 1e-12, pairs[i]
                out[i] = (got, paths[k])
        print("worst difference from the oracle: %.3g" % worst)
        assert worst < BOUND, worst
        return out


class EdgeEvalCase(EvalCase):
    def run_edges(self, rows, tip, log_offset=None, want=("loglik", "site_base") + TABLES):
        paths = [self.path(r, tip) for r in rows]
        res = self.hip.eval_edges_batch(self.family, *self.args(rows), capi.pad_paths(paths), tip, log_offset=log_offset,
                                        want=want)
        return res, paths

    def edge_oracle(self, row, path, tip, q):
        from oracle import linearham_oracle as orc
        r = self.rows[row]
        children, root, brlen = self.trees[row]
        return eo.edges(children, root, brlen, self.T, self.o.msa, q, r["er"], np.asarray(r["pi"]),
                        orc.gamma_rates_mean(r["alpha"], self.R), path, tip)
