"""What tests/test_gpu_ancestral.py and its worker process (tests/ancestral_worker.py) share: a family with its tree samples
as lh_asr_marginals_batch takes them (Case) and as lh_eval_ancestral_batch does (EvalCase), each with its oracle."""
import os

import numpy as np

from linearham_amd import capi
from oracle import linearham_oracle as orc
from tests import ancestral_marginal_oracle as amo
from tests import desc_builder as db

BOUND = 1e-10


class Case:
    """A family (the oracle's view `h`), its tree samples and their rates; a batch is a list of (row, seed tip)."""

    def __init__(self, hip, h, rows, R):
        import linearham_amd
        self.hip, self.h, self.rows, self.R = hip, h, rows, R
        self.T, self.L = h.msa.shape[0] + 1, h.msa.shape[1]
        self.trees, self.ops, self.depth = [], [], 0
        for r in rows:
            children, root, brlen = db.tree_arrays(orc.parse_newick(r["tree"]), h.xmsa_labels)
            o, d = hip.schedule_tree(self.T, children, root)
            self.trees.append((children, root, brlen))
            self.ops.append(o)
            self.depth = max(self.depth, d)
        self.rates = np.stack([orc.gamma_rates_mean(r["alpha"], R) for r in rows])
        self.fam = linearham_amd.Family(db.build_family_desc(h), hip)
        self._pre = {}

    def path(self, row, tip):
        children, root, _ = self.trees[row]
        return capi.seed_path(self.T, children, root, tip)

    def sibling(self, row, tip):
        children, _, _ = self.trees[row]
        i = list(children).index(tip)
        return int(children[i ^ 1])

    def batch(self, pairs, q, want=("marg", "rate_post")):
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        marg, rp = self.fam.asr_marginals_batch(
            self.T, self.depth, np.stack([self.ops[i] for i in rows]), np.stack([self.trees[i][2] for i in rows]),
            [self.rows[i]["er"] for i in rows], [self.rows[i]["pi"] for i in rows], self.rates[rows],
            np.stack([q[i] for i in rows]), capi.pad_paths(paths), want=want)
        return marg, rp, paths

    def oracle(self, row, q, path):
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        if row not in self._pre:
            self._pre[row] = amo.prepare(children, root, brlen, self.T, self.h.msa, r["er"], r["pi"], self.rates[row])
        return amo.marginals(children, root, brlen, self.T, self.h.msa, q, r["er"], np.asarray(r["pi"]), self.rates[row],
                             path, pre=self._pre[row])

    def check(self, pairs, q):
        """The batch against the oracle, the sum rule, zeros in the padding slots.  Returns (marg, rate_post, paths)."""
        marg, rp, paths = self.batch(pairs, q)
        worst = 0.0
        for i, (row, _) in enumerate(pairs):
            P = len(paths[i])
            want, want_rp = self.oracle(row, q[row], paths[i])
            worst = max(worst, np.abs(marg[i, :P] - want).max(), np.abs(rp[i] - want_rp).max())
            assert np.abs(marg[i, :P].sum(axis=-1) - 1).max() < 1e-12, pairs[i]
            assert np.abs(rp[i].sum(axis=-1) - 1).max() < 1e-12, pairs[i]
            assert not marg[i, P:].any()
        print("worst difference from the oracle: %.3g" % worst)
        assert worst < BOUND, worst
        return marg, rp, paths


def naive_dist(rng, n, L):
    """Rows of a distribution over A, C, G, T, N with exact zeros, mass on N, and one-hot rows among them."""
    q = rng.dirichlet(np.ones(5) * 0.5, size=(n, L))
    q[rng.random((n, L, 5)) < 0.2] = 0.0
    q[..., 4] += (q.sum(axis=-1) == 0)
    q /= q.sum(axis=-1, keepdims=True)
    hot = rng.random((n, L)) < 0.1
    q[hot] = np.eye(5)[rng.integers(0, 5, size=int(hot.sum()))]
    return q


def toy(data_dir):
    h = orc.PhyloHMM(os.path.join(data_dir, "phylo_hmm_input.yaml"), 0, os.path.join(data_dir, "hmm_params"), 0)
    tree = open(os.path.join(data_dir, "newton.tree")).read()
    rows = [dict(tree=tree, er=[1.0] * 6, pi=[0.17, 0.19, 0.25, 0.39], alpha=1.0),
            dict(tree=tree, er=[1.3, 0.4, 2.0, 0.7, 1.1, 1.0], pi=[0.3, 0.2, 0.1, 0.4], alpha=0.4)]
    return h, rows


def write_table(path, rows, log_offset=None):
    cols = ["Iteration", "Posterior", "Likelihood", "Prior", "alpha"] + ["er[%d]" % i for i in range(1, 7)] + \
        ["pi[%d]" % i for i in range(1, 5)] + ["tree"]
    with open(path, "w") as f:
        f.write("\t".join(cols) + "\n")
        for i, r in enumerate(rows):
            lik = -1000.0 if log_offset is None else log_offset[i]
            f.write("\t".join([str(10 * i), "%.4f" % (lik - 50), repr(float(lik)), "-50.0", repr(float(r["alpha"]))] +
                              [repr(float(x)) for x in r["er"]] + [repr(float(x)) for x in r["pi"]] + [r["tree"]]) + "\n")


class EvalCase:
    """A family through the host library (its handle has sampler tables) and the oracle; rows of a table."""

    def __init__(self, hip, yaml_path, pdir, rows, R, tmp_path):
        from linearham_amd import host
        self.hip, self.rows, self.R = hip, rows, R
        self.hh = host.PhyloHMM(yaml_path, 0, pdir, 0)
        self.o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
        tsv = str(tmp_path / "rows.tsv")
        write_table(tsv, rows[:1])
        self.family = self.hh.flatten_tsv(tsv, 1)["family"]
        labels = list(self.o.xmsa_labels)
        self.T, self.L = len(labels), self.o.msa.shape[1]
        self.trees = [host.newick_arrays(r["tree"], labels) for r in rows]
        self.ops, self.depth = [], 0
        for children, root, _ in self.trees:
            o, d = hip.schedule_tree(self.T, children, root)
            self.ops.append(o)
            self.depth = max(self.depth, d)
        self.state_space = self.hh.dump(1)

    def path(self, row, tip):
        children, root, _ = self.trees[row]
        return capi.seed_path(self.T, children, root, tip)

    def args(self, rows):
        return (self.T, self.depth, np.stack([self.ops[i] for i in rows]), np.stack([self.trees[i][2] for i in rows]),
                np.array([self.rows[i]["er"] for i in rows]), np.array([self.rows[i]["pi"] for i in rows]),
                np.array([self.rows[i]["alpha"] for i in rows]), self.R)

    def run(self, pairs, log_offset=None, want=("loglik", "site_base", "marg", "rate_post")):
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        res = self.hip.eval_ancestral_batch(self.family, *self.args(rows), capi.pad_paths(paths), log_offset=log_offset,
                                            want=want)
        return res, paths

    def oracle(self, row, path, q=None):
        """(marg, rate_post, site_base, loglik) of a row; q: the naive-base distribution to use instead of the oracle's."""
        from tests import posterior_oracle as po
        r = self.rows[row]
        ll = None
        if q is None:
            self.o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], self.R, is_path=False)
            self.o.initialize_phylo_emission()
            ll = self.o.log_likelihood()
            q = po.site_base(self.o, po.smoothing(self.o))
        children, root, brlen = self.trees[row]
        marg, rp = amo.marginals(children, root, brlen, self.T, self.o.msa, q, r["er"], np.asarray(r["pi"]),
                                 orc.gamma_rates_mean(r["alpha"], self.R), path)
        return marg, rp, q, ll
