"""What tests/test_gpu_ancestral_probs.py and its worker process (tests/ancestral_probs_worker.py) share: a family as
lh_eval_ancestral_candidates_batch takes it (ancestral_cases.EvalCase) with the oracle of K13 beside it."""
import os

import numpy as np

from linearham_amd import capi
from oracle import asr_oracle as ao
from oracle import linearham_oracle as orc
from tests import ancestral_probs_oracle as apo
from tests.ancestral_cases import EvalCase

PARENT, MRCA = capi.NODE_PARENT, capi.NODE_MRCA


class ProbsCase(EvalCase):
    def probs(self, pairs, node, cands=None, log_offset=None, want=("loglik", "cond", "log_cand")):
        """lh_eval_ancestral_candidates_batch over (row, seed tip) pairs; cands: registered first."""
        if cands is not None:
            self.hip.set_ancestral_candidates(self.family, cands)
        rows = [p[0] for p in pairs]
        paths = [self.path(*p) for p in pairs]
        res = self.hip.eval_ancestral_candidates_batch(self.family, *self.args(rows), capi.pad_paths(paths), node,
                                                       log_offset=log_offset, want=want)
        return res, paths

    def rates(self, row):
        return orc.gamma_rates_mean(self.rows[row]["alpha"], self.R)

    def oracle_tables(self, row, path, node):
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        return apo.cond_tables(children, root, brlen, self.T, self.o.msa, r["er"], np.asarray(r["pi"], dtype=float),
                               self.rates(row), path, node)

    def set_row(self, row):
        """The oracle object on a row's tree; returns its log-likelihood."""
        r = self.rows[row]
        self.o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], self.R, is_path=False)
        self.o.initialize_phylo_emission()
        return self.o.log_likelihood()

    def oracle_log_cand(self, row, G, cands):
        self.set_row(row)
        return apo.log_candidates(self.o, G, cands)

    def oracle_draws(self, row, path, node, n, seed):
        """n ancestral sequences at the node drawn by the oracle: naive sequences from the HMM's posterior, the inner
        nodes under each by asr_oracle.asr_sample."""
        self.set_row(row)
        children, root, brlen = self.trees[row]
        r = self.rows[row]
        code = {c: i for i, c in enumerate(self.o.alphabet)}
        v = path[apo.slot_of(node, path)]
        out = []
        for i in range(n):
            naive = np.array([code[c] for c in self.o.sample_naive_sequence()], dtype=np.uint8)
            _, anc, _ = ao.asr_sample(children, root, brlen, self.T, self.o.msa, naive, r["er"],
                                      np.asarray(r["pi"], dtype=float), self.rates(row), seed, i)
            out.append(anc[v - self.T])
        return np.array(out, dtype=np.uint8)


def synth(hip, tmp_path, R=4, rows=None, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(**kw), out)
    table = sf.read_trees_tsv(os.path.join(out, "trees.tsv"))
    return ProbsCase(hip, os.path.join(out, "cluster.yaml"), os.path.join(out, "hmm_params"), rows(table) if rows else table, R,
                     tmp_path)


def toy_case(hip, data_dir, tmp_path, R=4):
    from tests.ancestral_cases import toy
    _, rows = toy(data_dir)
    return ProbsCase(hip, os.path.join(data_dir, "phylo_hmm_input.yaml"), os.path.join(data_dir, "hmm_params"), rows, R,
                     tmp_path)
