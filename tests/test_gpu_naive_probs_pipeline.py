"""Exact naive-sequence probability tables end to end: K6c (naive sequences and hashes of K4's states) against the host's
HMM::ApplySampledStates, PhyloHMM::RunNaiveProbsPipeline against `linearham --pipeline` and the numpy oracles, its
invariances (hash width, host sampling, batch size, repeated runs), its edges, and the `--naive-probs[-pipeline]` CLI."""
import collections
import json
import math
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import host
from oracle import linearham_oracle as orc
from tests import naive_probs_oracle as npo
from tests import posterior_oracle as po

pytestmark = pytest.mark.gpu

D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_goldens.json")))
BASES = "ACGTN"
FILES = (".naive.tsv", ".aa.fasta", ".dnamap", ".summary.tsv")


def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _synthetic(tmp_path, name="fam", seed=0, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / name)
    sf.generate(sf.Spec.small(**kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    return yaml_path, pdir, tsv, sf.read_trees_tsv(tsv)


def _check_assembly(h, n_draws=24, seed=1):
    rng = np.random.default_rng(seed)
    states = np.array([h.sample_states_with_words(rng.integers(0, 2 ** 32, 624, dtype=np.uint64).astype(np.uint32))[0]
                       for _ in range(n_draws)])
    seqs, hsh, want = h.naive_sequences(states)
    got = ["".join(BASES[b] for b in row) for row in seqs]
    assert got == want
    by = {}
    for s, x in zip(got, hsh):
        assert by.setdefault(s, int(x)) == int(x)  # equal sequences, equal hashes
    assert len(set(by.values())) == len(by)  # (64-bit hashes of distinct sequences: no collision expected)
    return got


@pytest.mark.parametrize("case", ["phylo_hmm_input", "phylo_hmm_input_extra"])
def test_assembly_golden(case):
    meta = GOLD["PhyloHMM:" + case]["meta"]
    h = host.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    _check_assembly(h)


@pytest.mark.parametrize("locus,kw", [("igh", {}), ("igk", {}), ("igl", {}), ("igh", dict(ragged=4, ambiguous=0.02)),
                                      ("igk", dict(n_v=150, n_j=70))])
def test_assembly_synthetic(tmp_path, locus, kw):
    yaml_path, pdir, tsv, rows = _synthetic(tmp_path, locus=locus, n_samples=2, **kw)
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    r = rows[0]
    h.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
    got = _check_assembly(h, n_draws=40)
    assert len(set(got)) > 1


def _pipeline_cli(yaml_path, pdir, tsv, prefix, env=None, extra=(), seed=0):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([_exe(), "--naive-probs-pipeline", "--yaml-path", yaml_path, "--cluster-ind", "0",
                        "--hmm-param-dir", pdir, "--input-path", tsv, "--output-path", prefix, "--num-rates", "4",
                        "--seed", str(seed)] + list(extra), capture_output=True, text=True, timeout=600, env=e)
    return r


def _bytes(prefix):
    return [open(prefix + f, "rb").read() for f in FILES]


def test_pipeline_candidates_are_the_pipeline_draws(tmp_path):
    """At burn-in 0 with seed s the candidates are the distinct NaiveSequence values of RunPipeline with seed s, with
    their counts; every row is used; the probabilities are sorted and cover at most the whole mass."""
    yaml_path, pdir, tsv, rows = _synthetic(tmp_path, locus="igh", n_samples=300)
    res = str(tmp_path / "lh.tsv")
    host.PhyloHMM(yaml_path, 0, pdir, 5).run_pipeline(tsv, res, 4)
    lines = [ln.rstrip("\n").split("\t") for ln in open(res)]
    c = lines[0].index("NaiveSequence")
    counts = collections.Counter(ln[c] for ln in lines[1:])
    t = host.PhyloHMM(yaml_path, 0, pdir, 5).run_naive_probs_pipeline(tsv, str(tmp_path / "np"), 4)
    got = {r["seq"]: r["sampled_count"] for r in t["naive"]}
    assert got == dict(counts)
    s = t["summary"]
    assert s["rows_used"] == 300 and s["rows_skipped_nonfinite"] == 0
    assert s["draws_distinct"] == len(counts) == s["candidates"] and s["candidates_dropped"] == 0
    p = [r["probability"] for r in t["naive"]]
    assert p == sorted(p, reverse=True)
    assert 0 < s["covered_mass"] <= 1 + 1e-12 and abs(s["covered_mass"] - sum(p)) < 1e-12
    assert abs(sum(r["sampled_frequency"] for r in t["naive"]) - 1.0) < 1e-12
    # the amino-acid table: group sums of the DNA table, exact in the header
    total = sum(pp for _, pp, _ in t["aa"])
    assert abs(total - s["covered_mass"]) < 1e-12
    for name, pp, _ in t["aa"]:
        assert abs(sum(x for x, _ in t["dnamap"][name]) - pp) < 1e-15 + 1e-12 * pp


@pytest.mark.parametrize("burnin", [0.0, 0.25])
def test_pipeline_probabilities_against_the_oracle(tmp_path, burnin):
    yaml_path, pdir, tsv, rows = _synthetic(tmp_path, locus="igh", n_samples=16)
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    t = h.run_naive_probs_pipeline(tsv, str(tmp_path / "np"), 4, burnin_frac=burnin)
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    seqs = [r["seq"] for r in t["naive"]]
    lls, per_row = [], []
    for r in rows:
        o.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
        o.initialize_phylo_emission()
        ll = o.log_likelihood()
        lls.append(ll)
        per_row.append([math.exp(npo.log_cand(o, [BASES.index(ch) for ch in s], ll)) for s in seqs])
    rb = np.array([r["likelihood"] for r in rows])
    want, ess = po.weighted_marginals(lls, rb, np.array(per_row), burnin)
    got = np.array([r["probability"] for r in t["naive"]])
    assert np.max(np.abs(got - want)) < 1e-10 + 1e-13 * max(abs(x) for x in lls)
    s = t["summary"]
    assert s["rows_used"] == len(rows) - int(math.floor(burnin * len(rows)))
    assert abs(s["kish_ess"] - ess) < 1e-9 * ess


def test_invariances(tmp_path):
    """Byte-identical files across hash widths (collisions resolved exactly), the host sampler and two runs.  Batch
    sizes that split the table unevenly give the same candidates, counts and sampled frequencies bit for bit; the exact
    probabilities are combined batch by batch (RunMarginalsPipeline's rule), so they agree to rounding."""
    yaml_path, pdir, tsv, rows = _synthetic(tmp_path, locus="igh", n_samples=1000)
    base = str(tmp_path / "base")
    r = _pipeline_cli(yaml_path, pdir, tsv, base, extra=["--burnin-frac", "0.1"])
    assert r.returncode == 0, r.stderr
    want = _bytes(base)
    ref = host.read_naive_probs(base)
    assert ref["summary"]["candidates"] > 8
    for k, env in enumerate([{}, {"LH_COLLECT_HASH_BITS": "4"}, {"LH_COLLECT_HASH_BITS": "1"}, {"LH_HOST_SAMPLING": "1"},
                             {"LH_HOST_SAMPLING": "1", "LH_COLLECT_HASH_BITS": "4"}]):
        prefix = str(tmp_path / ("v%d" % k))
        r = _pipeline_cli(yaml_path, pdir, tsv, prefix, env=env, extra=["--burnin-frac", "0.1"])
        assert r.returncode == 0, (env, r.stderr)
        assert _bytes(prefix) == want, env
    for k, env in enumerate([{"LH_PIPELINE_BATCH": "1"}, {"LH_PIPELINE_BATCH": "257"},
                             {"LH_PIPELINE_BATCH": "1000", "LH_COLLECT_HASH_BITS": "4"}]):
        prefix = str(tmp_path / ("b%d" % k))
        r = _pipeline_cli(yaml_path, pdir, tsv, prefix, env=env, extra=["--burnin-frac", "0.1"])
        assert r.returncode == 0, (env, r.stderr)
        got = host.read_naive_probs(prefix)
        key = lambda t: {x["seq"]: (x["sampled_count"], x["sampled_frequency"], x["log_prior"]) for x in t["naive"]}  # noqa
        assert key(got) == key(ref), env
        pr = {x["seq"]: x["probability"] for x in ref["naive"]}
        for x in got["naive"]:
            assert abs(x["probability"] - pr[x["seq"]]) <= 1e-13 * pr[x["seq"]] + 1e-300, env
        for name in ("rows_used", "rows_skipped_nonfinite", "draws_distinct", "candidates", "candidates_dropped"):
            assert got["summary"][name] == ref["summary"][name], (env, name)
        assert abs(got["summary"]["kish_ess"] - ref["summary"]["kish_ess"]) < 1e-12 * ref["summary"]["kish_ess"]


def _golden_table(path, n=12, seed=4):
    """A RevBayes table for the golden family: its tree with scaled branch lengths, varied substitution parameters and
    RevBayes log-likelihoods, so that the rows' weights differ."""
    import re
    rng = np.random.default_rng(seed)
    newick = open(os.path.join(D, "newton.tree")).read().strip()
    head = ["Iteration", "Likelihood", "Prior", "alpha"] + ["er[%d]" % i for i in range(1, 7)] + \
        ["pi[%d]" % i for i in range(1, 5)] + ["tree"]
    lines = ["\t".join(head)]
    for i in range(n):
        scale = rng.uniform(0.5, 2.0)
        tree = re.sub(r":([0-9.]+)", lambda m: ":%.6f" % (float(m.group(1)) * scale), newick)
        er = rng.uniform(0.5, 2.0, 6)
        pi = rng.dirichlet([8.0] * 4)
        vals = [str(i), repr(float(rng.uniform(-90.0, -70.0))), "-10.0", repr(float(rng.uniform(0.3, 3.0)))]
        vals += [repr(float(x)) for x in er] + [repr(float(x)) for x in pi] + [tree]
        lines.append("\t".join(vals))
    open(path, "w").write("\n".join(lines) + "\n")


@pytest.mark.parametrize("burnin", [0.0, 0.25])
def test_complete_candidate_set(tmp_path, burnin):
    """Every sequence with a non-zero prior (naive_probs_oracle.by_enumeration) as the candidate file: the candidates
    hold all the posterior mass, and their per-site marginals sum_k p_k [s_k[site] = b] are K5's (--marginals-pipeline's
    .sites.tsv on the same table)."""
    case = "phylo_hmm_input"
    meta = GOLD["PhyloHMM:" + case]["meta"]
    yaml_path, pdir = os.path.join(D, case + ".yaml"), os.path.join(D, "hmm_params")
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    o.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    o.initialize_phylo_emission()
    o.log_likelihood()
    seqs = ["".join(BASES[b] for b in s) for s in npo.by_enumeration(o)]  # (the support does not depend on the tree)
    assert len(seqs) > 10
    cf = tmp_path / "all.txt"
    cf.write_text("\n".join(seqs) + "\n")
    tsv = str(tmp_path / "trees.tsv")
    _golden_table(tsv)
    t = host.PhyloHMM(yaml_path, 0, pdir, 0).run_naive_probs_pipeline(tsv, str(tmp_path / "np"), 4, burnin_frac=burnin,
                                                                      candidates_path=str(cf))
    s = t["summary"]
    assert s["candidates"] == len(seqs) and s["rows_used"] == 12 - int(math.floor(burnin * 12))
    assert abs(s["covered_mass"] - 1.0) < 1e-12
    assert all(np.isfinite(x["log_prior"]) for x in t["naive"])
    sb, _, ms = host.PhyloHMM(yaml_path, 0, pdir, 0).run_marginals_pipeline(tsv, str(tmp_path / "m"), 4,
                                                                            burnin_frac=burnin)
    L = o.msa.shape[1]
    k6 = np.zeros((L, 5))
    for x in t["naive"]:
        for j, ch in enumerate(x["seq"]):
            k6[j, BASES.index(ch)] += x["probability"]
    assert np.max(np.abs(k6 - sb)) < 1e-11  # (two reductions of the same weights in different orders)
    assert ms["rows_used"] == s["rows_used"] and abs(ms["kish_ess"] - s["kish_ess"]) < 1e-12 * s["kish_ess"]


def test_edges(tmp_path):
    yaml_path, pdir, tsv, rows = _synthetic(tmp_path, locus="igk", n_samples=200)
    full = host.PhyloHMM(yaml_path, 0, pdir, 0).run_naive_probs_pipeline(tsv, str(tmp_path / "full"), 4)
    n = full["summary"]["draws_distinct"]
    assert n >= 3
    # --max-candidates: the most drawn (ties: first appearance) and the number dropped
    k = n // 2
    r = _pipeline_cli(yaml_path, pdir, tsv, str(tmp_path / "cut"), extra=["--max-candidates", str(k)])
    assert r.returncode == 0, r.stderr
    cut = host.read_naive_probs(str(tmp_path / "cut"))
    assert cut["summary"]["candidates"] == k and cut["summary"]["candidates_dropped"] == n - k
    counts = {x["seq"]: x["sampled_count"] for x in full["naive"]}
    kept = {x["seq"] for x in cut["naive"]}
    assert min(counts[s] for s in kept) >= max([counts[s] for s in counts if s not in kept] + [0])
    for x in cut["naive"]:
        assert x["sampled_count"] == counts[x["seq"]]
    # candidates from a file, one of them impossible: probability 0, log_prior -inf, NA in the sampled columns
    seqs = [x["seq"] for x in full["naive"][:3]]
    o = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    L = o.msa.shape[1]
    i, b = next((i, b) for i in range(L) for b in range(5) if (b, i) not in o.xmsa_ids)
    bad = seqs[0][:i] + BASES[b] + seqs[0][i + 1:]
    cf = tmp_path / "cands.fa"
    cf.write_text("".join(">c%d\n%s\n" % (j, s) for j, s in enumerate(seqs + [bad])))
    t = host.PhyloHMM(yaml_path, 0, pdir, 0).run_naive_probs_pipeline(tsv, str(tmp_path / "file"), 4,
                                                                      candidates_path=str(cf))
    by = {x["seq"]: x for x in t["naive"]}
    assert by[bad]["probability"] == 0.0 and by[bad]["log_prior"] == -math.inf
    assert all(x["sampled_count"] is None for x in t["naive"])
    assert t["summary"]["draws_distinct"] is None
    for s in seqs:
        assert abs(by[s]["probability"] - {x["seq"]: x["probability"] for x in full["naive"]}[s]) < 1e-14
    # a malformed candidate file is refused with its line
    cf.write_text("ACGT\n")
    r = _pipeline_cli(yaml_path, pdir, tsv, str(tmp_path / "x"), extra=["--candidates-path", str(cf)])
    assert r.returncode != 0 and "line 1" in r.stderr
    # more than one device
    r = _pipeline_cli(yaml_path, pdir, tsv, str(tmp_path / "x"), extra=["--devices", "0,1"])
    assert r.returncode != 0 and "one device" in r.stderr


def test_extended_range_overflow_row(tmp_path):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec(n_leaves=500, n_sites=600, n_samples=64), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    d = _pipeline_cli(yaml_path, pdir, tsv, str(tmp_path / "d"))
    assert d.returncode == 0, d.stderr
    e = _pipeline_cli(yaml_path, pdir, tsv, str(tmp_path / "e"), extra=["--extended-range", "1"])
    assert e.returncode == 0, e.stderr
    sd, se = host.read_naive_probs(str(tmp_path / "d"))["summary"], host.read_naive_probs(str(tmp_path / "e"))["summary"]
    assert sd["rows_skipped_nonfinite"] > 0
    assert se["rows_skipped_nonfinite"] == 0 and se["rows_used"] == 64
    assert sd["rows_used"] == 64 - sd["rows_skipped_nonfinite"]


def test_cli_naive_probs_golden(tmp_path):
    case = "phylo_hmm_input"
    meta = GOLD["PhyloHMM:" + case]["meta"]
    o = orc.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    o.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    o.initialize_phylo_emission()
    ll = o.log_likelihood()
    bf = npo.by_enumeration(o)
    seqs = ["".join(BASES[b] for b in s) for s in list(bf)[:20]]
    cf = tmp_path / "c.txt"
    cf.write_text("\n".join(seqs) + "\n")
    args = [_exe(), "--naive-probs", "--yaml-path", os.path.join(D, case + ".yaml"), "--cluster-ind", "0",
            "--hmm-param-dir", os.path.join(D, "hmm_params"), "--newick-path", os.path.join(D, "newton.tree"),
            "--num-rates", str(meta["num_rates"]), "--alpha", repr(meta["alpha"]), "--candidates-path", str(cf)]
    args += sum([["--er", repr(x)] for x in meta["er"]], []) + sum([["--pi", repr(x)] for x in meta["pi"]], [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[0] == "rank\tNaiveSequence\tprobability\tlog_prior"
    rows = host.parse_naive_table(r.stdout)
    h = host.PhyloHMM(os.path.join(D, case + ".yaml"), 0, os.path.join(D, "hmm_params"), 0)
    h.initialize_phylo_parameters(os.path.join(D, "newton.tree"), meta["er"], meta["pi"], meta["alpha"], meta["num_rates"])
    lc, hll, prior = h.candidate_posterior(seqs)
    assert abs(hll - ll) < 1e-9 * abs(ll)
    got = {x["seq"]: x for x in rows}
    for k, s in enumerate(seqs):
        assert got[s]["probability"] == math.exp(lc[k]) and got[s]["log_prior"] == prior[k]
        want = npo.log_cand(o, [BASES.index(ch) for ch in s], ll)
        assert abs(lc[k] - want) < 1e-10 + 1e-13 * abs(ll)
