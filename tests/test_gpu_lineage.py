"""The lineage of a seed sequence on the device: K7 (lh_lineage_batch) against numpy on lh_asr_batch's sampled states
for the same draws, the lineage store, and PhyloHMM::RunLineagePipeline / `linearham --lineage-pipeline` against
`--pipeline` -> `--asr` -> tests/lineage_oracle.py on the same table.  Integers and bytes only: no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from linearham_amd import capi, host
from oracle import linearham_oracle as orc
from tests import desc_builder as db
from tests import lineage_oracle as lo
from tests.test_lineage_cpu import FILES, _compare, something_to_count

pytestmark = pytest.mark.gpu

BASES = "ACGTN"


@pytest.fixture(scope="module")
def hip():
    import linearham_amd
    lib = linearham_amd.load_library()
    assert lib.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return lib


def _family(tmp_path, **kw):
    from tools import synth_family as sf
    out = str(tmp_path / "fam")
    sf.generate(sf.Spec.small(divergence=0.03, brlen_mean=0.003, **kw), out)
    yaml_path, pdir, tsv = (os.path.join(out, n) for n in ("cluster.yaml", "hmm_params", "trees.tsv"))
    return yaml_path, pdir, tsv, sf.read_trees_tsv(tsv)


def _chain(children, root, T, tip):
    """The inner nodes from `tip`'s parent up to `root`."""
    parent = {}
    for v in range(T, 2 * T - 2):
        for c in children[2 * (v - T):2 * (v - T) + 2]:
            parent[int(c)] = v
    out = [parent[tip]]
    while out[-1] != root:
        out.append(parent[out[-1]])
    return out


def _kernel_case(hip, yaml_path, pdir, rows, naive, tip=None, seed=20261016, first_sample=5):
    """asr_batch and lineage_batch on the same inputs and draws: (anc, path lists, P, nt_hash, aa_hash, family).  `tip`
    None: every path is the root alone (a seed next to the root, P = 1)."""
    import linearham_amd
    h = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    T = h.msa.shape[0] + 1
    ops, brl, chains, depth = [], [], [], 0
    for s in rows:
        children, root, brlen = db.tree_arrays(orc.parse_newick(s["tree"]), h.xmsa_labels)
        o, d = hip.schedule_tree(T, children, root)
        ops.append(o)
        brl.append(brlen)
        depth = max(depth, d)
        chains.append([root] if tip is None else _chain(np.asarray(children).ravel(), root, T, tip))
    P = max(len(c) for c in chains)
    path = np.full((len(rows), P), -1, dtype=np.int32)
    for i, c in enumerate(chains):
        path[i, :len(c)] = c
    rates = np.stack([orc.gamma_rates_mean(s["alpha"], 4) for s in rows])
    args = (T, depth, np.stack(ops), np.stack(brl), [s["er"] for s in rows], [s["pi"] for s in rows], rates, naive, seed)
    anc, _ = fam.asr_batch(*args, first_sample)
    nt, aa = fam.lineage_batch(*args, path, first_sample)
    return anc, chains, P, nt, aa, fam, T


def _slots(anc, chains, P, naive, T):
    """{(row, slot): bases as a string} of the valid slots."""
    out = {}
    for i, c in enumerate(chains):
        for s, v in enumerate(c):
            out[(i, s)] = "".join(BASES[b] for b in anc[i][v - T])
        out[(i, P)] = "".join(BASES[b] for b in naive[i])
    return out


def _check_hashes(anc, chains, P, nt, aa, naive, T):
    """Over all (row, slot) pairs of the batch two hashes are equal exactly when the sequences (the oracle's
    translations) are equal; padding slots hold the sentinel."""
    slots = _slots(anc, chains, P, naive, T)
    assert anc.max() <= 3
    by_nt, by_aa = {}, {}
    for (i, s), seq in slots.items():
        assert by_nt.setdefault(seq, int(nt[i, s])) == int(nt[i, s]), (i, s)
        t = lo.translate(seq)
        assert by_aa.setdefault(t, int(aa[i, s])) == int(aa[i, s]), (i, s)
    assert len(set(by_nt.values())) == len(by_nt) and len(set(by_aa.values())) == len(by_aa)
    for i, c in enumerate(chains):
        for s in range(len(c), P):
            assert int(nt[i, s]) == capi.LINEAGE_PAD_HASH and int(aa[i, s]) == capi.LINEAGE_PAD_HASH
    return slots, by_nt, by_aa


def _few_naive(rng, n, L, k=3):
    """n naive rows drawn from k random sequences with N (equal and unequal pairs both occur)."""
    pool = rng.integers(0, 5, size=(k, L)).astype(np.uint8)
    return pool[rng.integers(0, k, size=n)]


@pytest.mark.parametrize("n_sites", [62, 61])
def test_kernel_hashes_separate_exactly_the_distinct_sequences(hip, tmp_path, n_sites):
    """L = 62 and 61 (neither a multiple of 3 nor of 8), a stepwise tree whose paths differ in length over the batch."""
    yaml_path, pdir, tsv, rows = _family(tmp_path, n_leaves=8, n_samples=40, n_sites=n_sites)
    rng = np.random.default_rng(n_sites)
    naive = _few_naive(rng, len(rows), n_sites)
    anc, chains, P, nt, aa, fam, T = _kernel_case(hip, yaml_path, pdir, rows, naive, tip=_last_tip(yaml_path, pdir))
    assert len({len(c) for c in chains}) >= 2 and P >= 3   # paths of different lengths, padding in use
    slots, by_nt, by_aa = _check_hashes(anc, chains, P, nt, aa, naive, T)
    assert len(by_nt) < len(slots) and 1 < len(by_aa) <= len(by_nt)   # sequences repeat over the batch
    # the lineage store: ids by sequence, one new id per distinct sequence, nothing differs
    ids = np.full((len(rows), P + 1), -1, dtype=np.int32)
    order = {}
    for (i, s) in sorted(slots):
        ids[i, s] = order.setdefault(slots[(i, s)], len(order))
    assert len(fam.lineage_resolve(ids)) == 0
    store = fam.lineage_store_read()
    assert ["".join(BASES[b] for b in r) for r in store] == list(order)
    assert np.array_equal(fam.lineage_store_read(1, 2), store[1:3])
    # a wrong assignment is found and can be read back
    wrong = ids.copy()
    (i0, s0), (i1, s1) = [k for k in sorted(slots) if slots[k] != slots[(0, 0)]][0], (0, 0)
    wrong[i0, s0] = ids[i1, s1]
    bad = fam.lineage_resolve(wrong)
    assert bad.tolist() == [i0 * (P + 1) + s0]
    assert "".join(BASES[b] for b in fam.lineage_rows_read(bad)[0]) == slots[(i0, s0)]
    fam.lineage_reset()
    assert fam.lineage_store_read(n_sites=n_sites).shape[0] == 0
    fam.close()


def _last_tip(yaml_path, pdir):
    """The last tip of the family (node number T - 1)."""
    return orc.PhyloHMM(yaml_path, 0, pdir, 0).msa.shape[0]


def test_kernel_seed_next_to_the_root_and_balanced_tree(hip, tmp_path):
    """P = 1 (the path is the root alone), and a balanced 16-tip tree (every path has the same length)."""
    yaml_path, pdir, tsv, rows = _family(tmp_path, n_leaves=16, n_samples=12, tree_shape="balanced", n_nni=0, seed=49)
    L = 62
    rng = np.random.default_rng(1)
    naive = _few_naive(rng, len(rows), L)
    anc, chains, P, nt, aa, fam, T = _kernel_case(hip, yaml_path, pdir, rows, naive, tip=None)
    assert P == 1 and nt.shape == (len(rows), 2)
    _check_hashes(anc, chains, P, nt, aa, naive, T)
    fam.close()
    anc, chains, P, nt, aa, fam, T = _kernel_case(hip, yaml_path, pdir, rows, naive, tip=T - 1)
    assert P >= 3 and {len(c) for c in chains} == {P}
    _check_hashes(anc, chains, P, nt, aa, naive, T)
    # hash bits do not depend on the batch or the slot: a sub-batch with other sample numbers' draws left aside,
    # the naive slots (the same bytes) hash as before
    fam.close()
    anc2, chains2, P2, nt2, aa2, fam, T = _kernel_case(hip, yaml_path, pdir, rows[3:7], naive[3:7], tip=T - 1,
                                                       first_sample=8)
    assert np.array_equal(nt2[:, P2], nt[3:7, P]) and np.array_equal(aa2[:, P2], aa[3:7, P])
    assert np.array_equal(nt2, nt[3:7]) and np.array_equal(aa2, aa[3:7])   # first_sample + i: the same draws
    fam.close()


def test_kernel_naive_slot_hash_is_k6c_hash(hip, tmp_path):
    """A naive sequence hashed by K6c (lh_naive_sequences, from sampled states) and by K7 (the same bytes in the naive
    slot) agree bit for bit."""
    yaml_path, pdir, tsv, rows = _family(tmp_path, n_leaves=8, n_samples=24)
    h = host.PhyloHMM(yaml_path, 0, pdir, 0)
    r = rows[0]
    h.initialize_phylo_parameters(r["tree"], r["er"], r["pi"], r["alpha"], 4, is_path=False)
    rng = np.random.default_rng(2)
    states = np.array([h.sample_states_with_words(rng.integers(0, 2 ** 32, 624, dtype=np.uint64).astype(np.uint32))[0]
                       for _ in range(len(rows))])
    seqs, hsh, _ = h.naive_sequences(states)
    anc, chains, P, nt, aa, fam, T = _kernel_case(hip, yaml_path, pdir, rows, seqs, tip=1)
    assert np.array_equal(nt[:, P], hsh)
    fam.close()


def test_batch_too_large_is_refused_with_the_largest_n(hip, tmp_path):
    yaml_path, pdir, tsv, rows = _family(tmp_path, n_leaves=8, n_samples=2)
    import ctypes as C
    import linearham_amd
    h = orc.PhyloHMM(yaml_path, 0, pdir, 0)
    fam = linearham_amd.Family(db.build_family_desc(h), hip)
    T, L = h.msa.shape[0] + 1, h.msa.shape[1]
    most = (1 << 30) // ((T - 2) * L)
    n = most + 1
    z = C.c_void_p(8)   # never read: the call is refused on its sizes
    rc = hip.lib.lh_lineage_batch(fam.handle, n, T, 4, C.cast(z, C.POINTER(C.c_int32)), C.cast(z, C.POINTER(C.c_double)),
                                  C.cast(z, C.POINTER(C.c_double)), C.cast(z, C.POINTER(C.c_double)),
                                  C.cast(z, C.POINTER(C.c_double)), 4, C.cast(z, C.POINTER(C.c_uint8)), 1, 0,
                                  C.cast(z, C.POINTER(C.c_int32)), 1, C.cast(z, C.POINTER(C.c_uint64)),
                                  C.cast(z, C.POINTER(C.c_uint64)))
    assert rc != 0 and ("at most %d samples" % most) in hip.error()
    fam.close()


# ---- the pipeline ----

def _exe():
    return os.path.join(os.path.dirname(host.host_library_path()), "linearham")


def _tables(tmp_path, n_rows=120, **kw):
    """`--pipeline` (seed 3) and `--asr` (seed 77) on a synthetic family; the oracle's tables of the last tip."""
    yaml_path, pdir, tsv, rows = _family(tmp_path, n_samples=n_rows, **kw)
    h = host.PhyloHMM(yaml_path, 0, pdir, 3)
    res, asr = str(tmp_path / "lh.tsv"), str(tmp_path / "asr.trees")
    h.run_pipeline(tsv, res, 4)
    h.run_asr(res, asr, 77)
    lines = [ln.rstrip("\n") for ln in open(asr)]
    seed_name = list(orc.PhyloHMM(yaml_path, 0, pdir, 3).xmsa_labels)[-1]
    want = lo.tabulate_trees(lines, seed_name)
    lengths = [len(lo.seqs_of_tree(ln, seed_name)) - 3 for ln in lines]
    something_to_count(want, lengths)
    return dict(yaml=yaml_path, pdir=pdir, res=res, asr=asr, h=h, seed_name=seed_name, want=want, lengths=lengths)


def _cli(t, prefix, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([_exe(), "--lineage-pipeline", "--yaml-path", t["yaml"], "--cluster-ind", "0", "--hmm-param-dir",
                           t["pdir"], "--input-path", t["res"], "--output-path", prefix, "--seed-seq", t["seed_name"],
                           "--seed", "77"], capture_output=True, text=True, timeout=600, env=e)


def _same_files(a, b, files=FILES):
    for ext in files:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext


@pytest.mark.parametrize("kw", [dict(n_leaves=8), dict(n_leaves=12, locus="igk", seed=43),
                                dict(n_leaves=20, seed=42, ragged=6, ambiguous=0.02)], ids=["igh", "igk", "ragged_n"])
def test_pipeline_matches_asr_then_oracle(tmp_path, kw):
    """run_pipeline -> run_asr(77) -> oracle against run_lineage_pipeline(77) on the same table: .fasta and .dnamap are
    the oracle's bytes, .nodes.tsv and .edges.tsv its counters; and all four are what the host tabulator makes of
    run_asr's file."""
    t = _tables(tmp_path, **kw)
    if "ragged" in kw:
        msa = orc.PhyloHMM(t["yaml"], 0, t["pdir"], 3).msa
        n_n = (msa == 4).sum(axis=0)
        assert ((n_n > 0) & (n_n < msa.shape[0])).sum() > 5
    prefix = str(tmp_path / "lin")
    got = t["h"].run_lineage_pipeline(t["res"], t["seed_name"], prefix, 77)
    _compare(prefix, t["want"])
    assert got["summary"]["longest_path"] == max(t["lengths"])
    assert got["summary"]["hash_collisions_resolved"] == 0
    via_trees = str(tmp_path / "via_trees")
    host.tabulate_lineage_trees(t["asr"], t["seed_name"], via_trees)
    _same_files(prefix, via_trees)
    # another Philox seed gives other draws (the comparison above is not of constants)
    other = str(tmp_path / "other")
    t["h"].run_lineage_pipeline(t["res"], t["seed_name"], other, 78)
    assert open(other + ".dnamap", "rb").read() != open(prefix + ".dnamap", "rb").read()


def test_cli_batch_size_and_hash_width(tmp_path):
    """`linearham --lineage-pipeline` writes the library call's bytes; LH_LINEAGE_BATCH=7 (18 batches) and
    LH_COLLECT_HASH_BITS=6 (at most 64 hash values: most sequences collide and are resolved by their bases) change
    nothing but the summary's collision count.  Child processes: the switches are read once."""
    t = _tables(tmp_path, n_leaves=8)
    lib = str(tmp_path / "lib")
    t["h"].run_lineage_pipeline(t["res"], t["seed_name"], lib, 77)
    plain = str(tmp_path / "cli")
    r = _cli(t, plain)
    assert r.returncode == 0, r.stderr
    _same_files(plain, lib)
    small = str(tmp_path / "b7")
    r = _cli(t, small, {"LH_LINEAGE_BATCH": "7"})
    assert r.returncode == 0, r.stderr
    _same_files(small, lib)
    narrow = str(tmp_path / "h6")
    r = _cli(t, narrow, {"LH_COLLECT_HASH_BITS": "6"})
    assert r.returncode == 0, r.stderr
    _same_files(narrow, lib, FILES[:4])
    s = host.read_lineage(narrow)["summary"]
    assert s["hash_collisions_resolved"] > 0, s     # else this tests nothing
    assert dict(s, hash_collisions_resolved=0) == host.read_lineage(lib)["summary"]
    both = str(tmp_path / "h6b7")
    r = _cli(t, both, {"LH_COLLECT_HASH_BITS": "6", "LH_LINEAGE_BATCH": "7"})
    assert r.returncode == 0, r.stderr
    _same_files(both, lib, FILES[:4])
    assert host.read_lineage(both)["summary"]["hash_collisions_resolved"] > 0


def test_pipeline_errors(tmp_path):
    t = _tables(tmp_path, n_rows=120, n_leaves=8)
    r = subprocess.run([_exe(), "--lineage-pipeline", "--yaml-path", t["yaml"], "--cluster-ind", "0", "--hmm-param-dir",
                        t["pdir"], "--input-path", t["res"], "--output-path", str(tmp_path / "e"), "--seed-seq", "nobody"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "nobody" in r.stderr
    with pytest.raises(RuntimeError, match="naive"):
        t["h"].run_lineage_pipeline(t["res"], "naive", str(tmp_path / "e"), 77)


def test_collect_device_and_a_rejected_schedule():
    """lh_lineage_collect_device on device-resident arrays (torch tensors, a stream, no synchronisation in the call): the
    hashes are lh_lineage_batch's; a path entry outside the inner nodes is padding; and after lh_asr_batch_device met a
    malformed device-resident schedule, that sample's hashes are all-ones in every slot, lh_family_status reports it,
    and the other samples keep their hashes.  (Its own process: torch brings its own HIP runtime, which comes up first.)"""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "lineage_device_worker.py")], capture_output=True,
                       text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["clean_status"] == "" and res["clean_hashes_ok"] and res["host_call_equal"]
    assert res["wild_path_is_padding"]
    assert "malformed schedule" in res["bad_status"]
    assert res["victim_all_ones"] and res["others_unchanged"]
