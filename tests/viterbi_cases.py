"""TEST INFRASTRUCTURE shared by tests/test_gpu_viterbi.py and its worker: families as (oracle object, device handle with
sampler tables, per-row inputs) and the oracle's most probable path of every row (tests/viterbi_oracle.py)."""
import json
import os

import numpy as np

from oracle import linearham_oracle as orc
from tests import desc_builder as db
from tests import posterior_oracle as po
from tests import viterbi_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "golden", "data")
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_goldens.json")))


def golden_rows(case):
    """(oracle object, [row parameters]) of a golden family: its one pinned tree."""
    meta = GOLD["PhyloHMM:" + case]["meta"]
    o = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    return o, [dict(tree=os.path.join(D, "newton.tree"), er=meta["er"], pi=meta["pi"], alpha=meta["alpha"],
                    R=meta["num_rates"], is_path=True)]


def synthetic_rows(workdir, n_rows, **kw):
    """(oracle object, [row parameters], (yaml, hmm_params, trees.tsv)) of a tools/synth_family.Spec.small family."""
    from tools import synth_family as sf
    out = os.path.join(str(workdir), "fam")
    sf.generate(sf.Spec.small(n_samples=n_rows, **kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    rows = [dict(tree=r["tree"], er=r["er"], pi=r["pi"], alpha=r["alpha"], R=4, is_path=False, likelihood=r["likelihood"])
            for r in sf.read_trees_tsv(tsv)]
    return o, rows, (yaml_path, pdir, tsv)


def set_row(o, r):
    """Puts row r on the oracle object; returns the germline emission count `ec` (read before any forward pass)."""
    o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], r["R"], is_path=r["is_path"])
    o.initialize_phylo_emission()
    return po.emission_count(o)


def oracle_row(o, r, keep_rows=False):
    """dict(path, states, log_path, margin, loglik[, rows]) of row r."""
    ec = set_row(o, r)
    v = vo.viterbi(o, ec)
    v["states"] = vo.to_states(o, v["path"])
    v["ec"] = ec
    if keep_rows:
        v["rows"] = [(a, b, np.array(e, dtype=float), T) for a, b, e, T in vo.chain_rows(o)]
    v["loglik"] = o.log_likelihood()
    return v


def device_family(hip, o):
    """A device handle of the oracle object's family with its sampler tables (K8 writes paths in K4's layout)."""
    import linearham_amd
    fam = linearham_amd.Family(db.build_family_desc(o), hip)
    fam.set_sampler(*vo.sampler_tables(o))
    return fam


def device_inputs(hip, o, rows):
    """dict(n_tips, max_depth, ops, brlen, er, pi, alpha, R) of the rows, as the batched entry points take them."""
    T = o.msa.shape[0] + 1
    ops, brlen, depth = [], [], 0
    for r in rows:
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], r["R"], is_path=r["is_path"])
        children, root, bl = db.tree_arrays(o.tree, o.xmsa_labels)
        op, d = hip.schedule_tree(T, children, root)
        ops.append(op)
        brlen.append(bl)
        depth = max(depth, d)
    return dict(n_tips=T, max_depth=depth, ops=np.stack(ops), brlen=np.stack(brlen),
                er=np.array([r["er"] for r in rows], dtype=float), pi=np.array([r["pi"] for r in rows], dtype=float),
                alpha=np.array([r["alpha"] for r in rows], dtype=float), R=rows[0]["R"])


def run_viterbi(hip, fam, inp, sl=slice(None), **kw):
    return hip.eval_viterbi_batch(fam, inp["n_tips"], inp["max_depth"], inp["ops"][sl], inp["brlen"][sl], inp["er"][sl],
                                  inp["pi"][sl], inp["alpha"][sl], inp["R"], **kw)


def tied_desc(o):
    """The family descriptor of `o` changed so that, with equal emissions, the four NTI states of a gene carry the same value
    on every junction row (every NTI table constant over the bases) and the best path runs through them (landing in a
    gene's germline states straight from the left gene costs 2^-12): exact ties at every NTI step."""
    desc = db.build_family_desc(o)
    for J in (desc.vd, desc.dj):
        if J is None:
            continue
        W, nR = J.n_rows, J.n_right
        J.right_ntt[:] = 0.25
        for a, shape, axis in ((J.right_gp_nli, (nR, 4), 1), (J.right_nlo, (W, nR, 4), 2), (J.exit_nlo, (nR, 4), 1)):
            v = a.reshape(shape)
            v[:] = v.max(axis=axis, keepdims=True)
        J.right_gp_li *= 2.0 ** -12
        J.exit_gp_li *= 2.0 ** -12
    return desc
