"""ctypes binding of the C++ host library (liblinearham_host.so): linearham's HMM / SimpleHMM /
PhyloHMM class surface.  Used by tests/ and bench.py; no numerics live here."""
import ctypes as C
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def host_library_path():
    # LH_LIB_DIR: timing experiments load a variant build from its own directory (tools/build_variant.sh) instead of
    # overwriting the product library in place
    return os.path.join(os.environ.get("LH_LIB_DIR") or os.path.join(_HERE, "lib"), "liblinearham_host.so")


def load_host():
    global _LIB
    if _LIB is None:
        p = host_library_path()
        if not os.path.exists(p):
            raise RuntimeError("host library %s is missing: run __graft_entry__.build()" % p)
        lib = C.CDLL(p)
        lib.lhh_last_error.restype = C.c_char_p
        _LIB = lib
    return _LIB


def _check(rc):
    if rc != 0:
        raise RuntimeError(load_host().lhh_last_error().decode())


def germline_json(path, gtype):
    out = C.c_char_p()
    _check(load_host().lhh_germline_json(path.encode(), C.c_char(gtype.encode()), C.byref(out)))
    return json.loads(out.value.decode())


def newick_roundtrip(newick, labels):
    """Parse a Newick string as the host does and return the output table's tree column
    (PhyloHMM::WriteOutputLine, src/PhyloHMM.cpp:299-300).  No device needed."""
    out = C.c_char_p()
    _check(load_host().lhh_newick_roundtrip(newick.encode(), "\n".join(labels).encode(), C.byref(out), None, None,
                                            None))
    return out.value.decode()


def newick_arrays(newick, labels):
    """The host's rooted-at-naive arrays of a Newick string: (children [(T-2)*2], root, brlen [2T-2])."""
    import numpy as np
    T = len(labels)
    children = np.zeros(2 * (T - 2), dtype=np.int32)
    brlen = np.zeros(2 * T - 2)
    root = C.c_int32()
    out = C.c_char_p()
    _check(load_host().lhh_newick_roundtrip(newick.encode(), "\n".join(labels).encode(), C.byref(out),
                                            children.ctypes.data_as(C.POINTER(C.c_int32)),
                                            brlen.ctypes.data_as(C.POINTER(C.c_double)), C.byref(root)))
    return children, root.value, brlen


def seed_path(n_tips, children, root, seed_tip):
    """The `path` row of a tip under the tree (children [(T-2)*2], root) in lh_schedule_tree's numbering: the inner nodes
    from the tip's parent up to the root (naive's neighbour), each the child of the next -- linearham::SeedPath, the walk
    the lineage pipelines use.  No device needed."""
    import numpy as np
    children = np.ascontiguousarray(children, dtype=np.int32).ravel()
    T = int(n_tips)
    if children.size != 2 * (T - 2):
        raise ValueError("seed_path: children must hold 2 (n_tips - 2) entries")
    if not 1 <= seed_tip < T:
        raise ValueError("seed_path: the seed is one of the tips 1 .. n_tips - 1 (0 is naive)")
    path = np.zeros(max(T - 2, 1), dtype=np.int32)
    n = C.c_int()
    lib = load_host()
    lib.lhh_seed_path.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    _check(lib.lhh_seed_path(children.ctypes.data, T, int(root), int(seed_tip), path.ctypes.data, len(path), C.byref(n)))
    if n.value == 0:
        raise ValueError("seed_path: tip %d does not hang below the root" % seed_tip)
    return [int(v) for v in path[:n.value]]


def clade_slot(n_tips, children, root, seed_tip, with_tips):
    """(path, slot): the seed's `path` row (seed_path) and the index on it of the most recent common ancestor of the seed
    and the tips `with_tips` -- linearham::CladeSlot.  That node means the same in every tree sample though its slot
    differs; the `_at` entry points of K13 and K14 take the slot per row.  Raises ValueError, naming the offender, for an
    empty list, tip 0 (naive), a tip outside 1 .. n_tips - 1, the seed itself or a repeated tip.  No device needed."""
    import numpy as np
    children = np.ascontiguousarray(children, dtype=np.int32).ravel()
    T = int(n_tips)
    if children.size != 2 * (T - 2):
        raise ValueError("clade_slot: children must hold 2 (n_tips - 2) entries")
    tips = np.ascontiguousarray([int(t) for t in with_tips], dtype=np.int32)
    path = np.zeros(max(T - 2, 1), dtype=np.int32)
    n, slot = C.c_int(), C.c_int()
    lib = load_host()
    lib.lhh_clade_slot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if lib.lhh_clade_slot(children.ctypes.data, T, int(root), int(seed_tip), tips.ctypes.data, len(tips), path.ctypes.data,
                          len(path), C.byref(n), C.byref(slot)) != 0:
        raise ValueError(lib.lhh_last_error().decode())
    return [int(v) for v in path[:n.value]], slot.value


def read_ancestral_marginals(prefix):
    """The files of PhyloHMM::RunAncestralMarginalsPipeline: dict(parent [L][4], mrca [L][4], map_base {"parent", "mrca"},
    rates [L][R], rows [(row, weight, chain_length)], summary)."""
    import numpy as np

    def table(path, last_is_text):
        lines = open(path).read().strip().split("\n")
        cells = [ln.split("\t") for ln in lines[1:]]
        end = -1 if last_is_text else None
        return lines[0].split("\t"), np.array([[float(x) for x in c[1:end]] for c in cells]), [c[-1] for c in cells]
    out, maps = {}, {}
    for name in ("parent", "mrca"):
        header, out[name], maps[name] = table(prefix + "." + name + ".tsv", True)
        assert header == ["site", "A", "C", "G", "T", "map_base"]
    out["map_base"] = maps
    _, out["rates"], _ = table(prefix + ".rates.tsv", False)
    rows = [ln.split("\t") for ln in open(prefix + ".rows.tsv").read().strip().split("\n")]
    assert rows[0] == ["row", "weight", "chain_length"]
    out["rows"] = [(int(r[0]), float(r[1]), int(r[2])) for r in rows[1:]]
    out["summary"] = _parse_summary(open(prefix + ".summary.tsv").read())
    return out


def read_ancestral_probs(prefix):
    """The files of PhyloHMM::RunAncestralProbsPipeline: dict(names, seqs, prob [K] in the file's (ranked) order, rows [(row,
    weight, chain_length)], summary)."""
    import numpy as np
    lines = [ln.split("\t") for ln in open(prefix + ".probs.tsv").read().strip("\n").split("\n")]
    assert lines[0] == ["name", "sequence", "probability"], lines[0]
    return dict(names=[c[0] for c in lines[1:]], seqs=[c[1] for c in lines[1:]], prob=np.array([float(c[2]) for c in lines[1:]]),
                rows=_seed_rows(prefix),
                summary=_parse_summary(open(prefix + ".summary.tsv").read()))


def parse_node_codons(text):
    """dict(codons [n_codons][64], aa [per codon {amino acid: p}], change [n_codons][4]) from the three tables
    WriteNodeCodonTable, WriteNodeAminoAcidTable and WriteChangeTable print, separated by blank lines.  The changes table has
    a line per codon, so it gives the count."""
    import numpy as np
    cod, aa, chg = text.strip("\n").split("\n\n")
    lines = [ln.split("\t") for ln in chg.strip("\n").split("\n")]
    assert lines[0] == ["codon", "identical", "synonymous", "replacement", "undetermined"], lines[0]
    change = np.array([[float(x) for x in ln[1:]] for ln in lines[1:]]).reshape(-1, 4)
    assert [int(ln[0]) for ln in lines[1:]] == list(range(len(change)))
    rows = [ln.split("\t") for ln in cod.strip("\n").split("\n")]
    assert rows[0] == ["codon", "first_site", "bases", "probability"], rows[0]
    codons = np.zeros((len(change), 64))
    for c, _, bases, p in rows[1:]:
        i = ["ACGT".index(b) for b in bases]
        codons[int(c), 16 * i[0] + 4 * i[1] + i[2]] = float(p)
    assert aa.split("\n")[0].split("\t") == ["codon", "aa", "probability"]
    return dict(codons=codons, aa=_parse_aa_table(aa, len(change)), change=change)


def read_node_codons(prefix):
    """The files of PhyloHMM::RunNodeCodonsPipeline: parse_node_codons' dict plus rows [(row, weight, chain_length)] and
    summary."""
    res = parse_node_codons("\n".join(open(prefix + ext).read() for ext in (".codons.tsv", ".aa.tsv", ".changes.tsv")))
    res["rows"] = _seed_rows(prefix)
    summary = {}
    for ln in open(prefix + ".summary.tsv").read().strip().split("\n")[1:]:
        k, v = ln.split("\t")
        summary[k] = v if k == "node" else None if v == "NA" else \
            int(v) if k in ("rows_used", "rows_skipped_nonfinite", "frame", "slot_min", "slot_max") else float(v)
    res["summary"] = summary
    return res


def node_codons_write(codons, change, frame=0):
    """The host writers on caller tables codons [n_codons][64] and change [n_codons][4]: the three texts joined by blank
    lines (parse_node_codons reads them back)."""
    import numpy as np
    codons = np.ascontiguousarray(codons, dtype=np.float64)
    change = np.ascontiguousarray(change, dtype=np.float64)
    n = codons.shape[0]
    assert codons.shape == (n, 64) and change.shape == (n, 4)
    lib = load_host()
    lib.lhh_write_node_codons.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    out = C.c_char_p()
    _check(lib.lhh_write_node_codons(codons.ctypes.data, change.ctypes.data, n, frame, C.byref(out)))
    return out.value.decode()


def parse_lineage_replacements(text):
    """dict(aa_counts [n_codons][21][21] -- the off-diagonal cells, the diagonal is not written --, codon_counts
    [n_codons][4], seed_change [n_codons][3]) from the three tables WriteReplacementTable, WriteCodonChangeTable and
    WriteSeedChangeTable print, separated by blank lines.  Amino acids are indexed by posterior.AA_SYMBOLS."""
    import numpy as np
    from .posterior import AA_SYMBOLS
    rep, chg, seed = text.strip("\n").split("\n\n")[:3]
    lines = [ln.split("\t") for ln in chg.strip("\n").split("\n")]
    assert lines[0] == ["codon", "unchanged", "synonymous", "replacement", "undetermined"], lines[0]
    counts = np.array([[float(x) for x in ln[1:]] for ln in lines[1:]]).reshape(-1, 4)
    assert [int(ln[0]) for ln in lines[1:]] == list(range(len(counts)))
    lines = [ln.split("\t") for ln in seed.strip("\n").split("\n")]
    assert lines[0] == ["codon", "unchanged", "synonymous", "replacement"], lines[0]
    seed_change = np.array([[float(x) for x in ln[1:]] for ln in lines[1:]]).reshape(-1, 3)
    rows = [ln.split("\t") for ln in rep.strip("\n").split("\n")]
    assert rows[0] == ["codon", "first_site", "from", "to", "expected_edges"], rows[0]
    aa = np.zeros((len(counts), 21, 21))
    for c, _, x, y, v in rows[1:]:
        aa[int(c), AA_SYMBOLS.index(x), AA_SYMBOLS.index(y)] = float(v)
    return dict(aa_counts=aa, codon_counts=counts, seed_change=seed_change)


def read_lineage_replacements(prefix):
    """The files of PhyloHMM::RunLineageReplacementsPipeline: parse_lineage_replacements' dict plus rows [(row, weight,
    chain_length, expected_synonymous, expected_replacement)] and summary."""
    res = parse_lineage_replacements("\n".join(open(prefix + ext).read()
                                               for ext in (".replacements.tsv", ".codon_changes.tsv", ".seed_edge.tsv")))
    rows = [ln.split("\t") for ln in open(prefix + ".rows.tsv").read().strip().split("\n")]
    assert rows[0] == ["row", "weight", "chain_length", "expected_synonymous", "expected_replacement"]
    res["rows"] = [(int(r[0]), float(r[1]), int(r[2]), float(r[3]), float(r[4])) for r in rows[1:]]
    summary = {}
    for ln in open(prefix + ".summary.tsv").read().strip().split("\n")[1:]:
        k, v = ln.split("\t")
        summary[k] = int(v) if k in ("rows_used", "rows_skipped_nonfinite", "frame") else float(v)
    res["summary"] = summary
    return res


def lineage_replacements_write(codon_counts, aa_counts, seed_change, frame=0):
    """The host writers on caller tables codon_counts [n_codons][4], aa_counts [n_codons][21][21] and seed_change
    [n_codons][3]: the three texts joined by blank lines (parse_lineage_replacements reads them back)."""
    import numpy as np
    cc = np.ascontiguousarray(codon_counts, dtype=np.float64)
    aa = np.ascontiguousarray(aa_counts, dtype=np.float64)
    sc = np.ascontiguousarray(seed_change, dtype=np.float64)
    n = cc.shape[0]
    assert cc.shape == (n, 4) and aa.shape == (n, 21, 21) and sc.shape == (n, 3)
    lib = load_host()
    lib.lhh_write_lineage_replacements.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    out = C.c_char_p()
    _check(lib.lhh_write_lineage_replacements(cc.ctypes.data, aa.ctypes.data, sc.ctypes.data, n, frame, C.byref(out)))
    return out.value.decode()


def parse_lineage_node(name):
    """--node's values: "parent" -> 0 (the seed's parent), "mrca" -> 1, "mrca-with:<name>[,<name>...]" -> NODE_MRCA_WITH
    (linearham::ParseLineageNode; parse_lineage_node_text also gives the names)."""
    lib = load_host()
    lib.lhh_parse_lineage_node.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    node = C.c_int()
    _check(lib.lhh_parse_lineage_node(name.encode(), C.byref(node)))
    return node.value


def read_named_candidates(path, n_sites):
    """linearham::ReadNamedCandidateFile: [(name, sequence)] in file order."""
    lib = load_host()
    lib.lhh_read_named_candidates.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p)]
    out = C.c_char_p()
    _check(lib.lhh_read_named_candidates(path.encode(), n_sites, C.byref(out)))
    return [tuple(ln.split("\t")) for ln in out.value.decode().strip("\n").split("\n")]


NODE_MRCA_WITH = 2  # parse_lineage_node's value for "mrca-with:<name>[,<name>...]"


def parse_lineage_node_text(text):
    """(node, names) of --node's text (linearham::ParseLineageNodeText): (0, []) for "parent", (1, []) for "mrca" and
    (NODE_MRCA_WITH, names) for "mrca-with:<name>[,<name>...]", the most recent common ancestor of the seed and the named
    sequences."""
    lib = load_host()
    lib.lhh_parse_lineage_node_text.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    node, names = C.c_int(), C.c_char_p()
    _check(lib.lhh_parse_lineage_node_text(text.encode(), C.byref(node), C.byref(names)))
    return node.value, [n for n in names.value.decode().split("\n") if n]


def _node_arg(node):
    """How PhyloHMM's methods hand `node` on: (entry-point suffix, argument, its ctype).  "mrca-with:..." goes as text to
    the `_at` entry points; the two old words and integers take the integer ones, as before."""
    if isinstance(node, str) and node.startswith("mrca-with:"):
        return "_at", node.encode(), C.c_char_p
    if isinstance(node, str):
        node = parse_lineage_node(node)
    return "", node, C.c_int


def _seed_rows(prefix):
    """.rows.tsv of a pipeline over a seed's lineage: (row, weight, chain_length), and the slot where the node is a
    'mrca-with' one."""
    rows = [ln.split("\t") for ln in open(prefix + ".rows.tsv").read().strip().split("\n")]
    assert rows[0] in (["row", "weight", "chain_length"], ["row", "weight", "chain_length", "slot"]), rows[0]
    return [(int(r[0]), float(r[1])) + tuple(int(x) for x in r[2:]) for r in rows[1:]]


def read_lineage_substitutions(prefix):
    """The files of PhyloHMM::RunLineageSubstitutionsPipeline: dict(counts [L][4][4], substitutions [L] (the off-diagonal sum
    the file carries), seed_edge [L][4][4], naive_edge [L][5][4], rows [(row, weight, chain_length, expected_substitutions)],
    summary).  Tables are indexed [ancestor base][descendant base]."""
    import numpy as np

    def table(path, n_rows, with_sum):
        lines = open(path).read().strip().split("\n")
        want = ["site"] + [a + c for a in "ACGTN"[:n_rows] for c in "ACGT"] + (["substitutions"] if with_sum else [])
        assert lines[0].split("\t") == want, lines[0]
        return np.array([[float(x) for x in ln.split("\t")[1:]] for ln in lines[1:]])
    out = {}
    counts = table(prefix + ".substitutions.tsv", 4, True)
    out["counts"], out["substitutions"] = counts[:, :16].reshape(-1, 4, 4), counts[:, 16]
    out["seed_edge"] = table(prefix + ".seed_edge.tsv", 4, False).reshape(-1, 4, 4)
    out["naive_edge"] = table(prefix + ".naive_edge.tsv", 5, False).reshape(-1, 5, 4)
    rows = [ln.split("\t") for ln in open(prefix + ".rows.tsv").read().strip().split("\n")]
    assert rows[0] == ["row", "weight", "chain_length", "expected_substitutions"]
    out["rows"] = [(int(r[0]), float(r[1]), int(r[2]), float(r[3])) for r in rows[1:]]
    out["summary"] = _parse_summary(open(prefix + ".summary.tsv").read())
    return out


def _parse_gene_table(text):
    genes = {}
    for line in text.strip().split("\n")[1:]:
        reg, name, p = line.split("\t")
        genes.setdefault(reg, {})[name] = float(p)
    return genes


def read_marginals(prefix):
    """(site_base [L][5], {"V"|"D"|"J": {gene: p}}, summary dict) from the files RunMarginalsPipeline writes."""
    lines = open(prefix + ".sites.tsv").read().strip().split("\n")[1:]
    sb = np.array([[float(x) for x in ln.split("\t")[1:6]] for ln in lines])
    genes = _parse_gene_table(open(prefix + ".genes.tsv").read())
    summary = {}
    for ln in open(prefix + ".summary.tsv").read().strip().split("\n")[1:]:
        k, v = ln.split("\t")
        summary[k] = float(v) if k == "kish_ess" else int(v)
    return sb, genes, summary


def _parse_aa_table(text, n_codons):
    aa = [dict() for _ in range(n_codons)]
    for ln in text.strip("\n").split("\n")[1:]:
        c, a, p = ln.split("\t")
        aa[int(c)][a] = float(p)
    return aa


def parse_codon_tables(codon_text, aa_text):
    """(table [n_codons][125], [per codon {amino acid: p}]) from the texts WriteCodonTable / WriteAminoAcidTable print
    (every codon has an entry above 0, so the last line names the last codon)."""
    from . import posterior
    rows = [ln.split("\t") for ln in codon_text.strip("\n").split("\n")[1:]]
    n_codons = int(rows[-1][0]) + 1 if rows else 0
    table = np.zeros((n_codons, 125))
    for c, site, bases, p in rows:
        i = [posterior.BASES.index(b) for b in bases]
        table[int(c), 25 * i[0] + 5 * i[1] + i[2]] = float(p)
    return table, _parse_aa_table(aa_text, n_codons)


def read_codon_marginals(prefix):
    """(table [n_codons][125], [per codon {amino acid: p}], summary dict) from the files RunCodonMarginalsPipeline writes."""
    table, aa = parse_codon_tables(open(prefix + ".codons.tsv").read(), open(prefix + ".aa.tsv").read())
    summary = {}
    for ln in open(prefix + ".summary.tsv").read().strip().split("\n")[1:]:
        k, v = ln.split("\t")
        summary[k] = float(v) if k == "kish_ess" else int(v)
    return table, aa, summary


def parse_events(deletions_text, insertions_text, spans_text):
    """dict(deletions = {(column, gene, length): p}, insertions = {(column, length): p}, spans = {(junction, left rows,
    right first row): p}) from the texts WriteDeletionTable / WriteInsertionTable / WriteSpanTable print.  gene "*" names
    the gene-summed rows; an insertion's column is the annotation's (VDInsertion, DJInsertion, VJInsertion)."""
    def rows(text):
        return [ln.split("\t") for ln in text.strip("\n").split("\n")[1:] if ln]
    return dict(deletions={(c, g, int(k)): float(p) for c, g, k, p in rows(deletions_text)},
                insertions={(j + "Insertion", int(k)): float(p) for j, k, p in rows(insertions_text)},
                spans={(j, int(a), int(b)): float(p) for j, a, b, p in rows(spans_text)})


def read_events(prefix):
    """(parse_events' dict, summary dict) from the files RunEventsPipeline writes."""
    tables = parse_events(*[open(prefix + ext).read() for ext in (".deletions.tsv", ".insertions.tsv", ".spans.tsv")])
    summary = {}
    for ln in open(prefix + ".summary.tsv").read().strip().split("\n")[1:]:
        k, v = ln.split("\t")
        summary[k] = float(v) if k == "kish_ess" else int(v)
    return tables, summary


def read_naive_probs(prefix):
    """The files RunNaiveProbsPipeline writes: dict(naive = list of row dicts of <prefix>.naive.tsv in rank order
    (probability / log_prior floats, sampled_count int or None, sampled_frequency float or None), aa = [(name, p, aa)]
    of <prefix>.aa.fasta, dnamap = {name: [(p, dna)]} of <prefix>.dnamap, summary = dict of <prefix>.summary.tsv)."""
    return dict(naive=parse_naive_table(open(prefix + ".naive.tsv").read()), aa=_parse_aa(open(prefix + ".aa.fasta").read()),
                dnamap=_parse_dnamap(open(prefix + ".dnamap").read()), summary=_parse_summary(open(prefix + ".summary.tsv").read()))


def parse_naive_table(text):
    """Rows of a .naive.tsv table (or of `linearham --naive-probs`'s output, which has no sampled columns)."""
    lines = text.strip("\n").split("\n")
    head = lines[0].split("\t")
    rows = []
    for ln in lines[1:]:
        d = dict(zip(head, ln.split("\t")))
        r = dict(rank=int(d["rank"]), seq=d["NaiveSequence"], probability=float(d["probability"]),
                 log_prior=float(d["log_prior"]))
        if "sampled_count" in d:
            r["sampled_count"] = None if d["sampled_count"] == "NA" else int(d["sampled_count"])
            r["sampled_frequency"] = None if d["sampled_frequency"] == "NA" else float(d["sampled_frequency"])
        rows.append(r)
    return rows


def _parse_aa(text):
    lines = text.strip("\n").split("\n")
    return [(lines[i][1:], float(lines[i][1:].split("_")[2]), lines[i + 1]) for i in range(0, len(lines), 2)]


def _parse_dnamap(text):
    out, name = {}, None
    for ln in text.strip("\n").split("\n"):
        if ln.startswith(">"):
            name = ln[1:]
            out[name] = []
        else:
            p, dna = ln.split(",")
            out[name].append((float(p), dna))
    return out


def _parse_summary(text):
    out = {}
    for ln in text.strip().split("\n")[1:]:
        k, v = ln.split("\t")
        out[k] = None if v == "NA" else v if k == "node" else (float(v) if k in ("kish_ess", "covered_mass") else int(v))
    return out


def read_annotations(prefix):
    """The files RunAnnotationsPipeline writes: dict(annotations = list of row dicts of <prefix>.annotations.tsv in rank
    order (rank, map_rows ints; probability, log_probability, log_prior, map_weight_share floats; the annotation columns
    as strings), best = the one row of <prefix>.best.tsv, rows = [dict(row, lh_loglik, log_weight, log_path_posterior,
    annotation = rank or None)] of <prefix>.rows.tsv, summary = dict of <prefix>.summary.tsv)."""
    def table(path):
        lines = open(path).read().strip("\n").split("\n")
        head = lines[0].split("\t")
        return [dict(zip(head, ln.split("\t") + [""] * (len(head) - len(ln.split("\t"))))) for ln in lines[1:]]

    def annotation(d):
        d = dict(d)
        for k in ("rank", "map_rows"):
            d[k] = int(d[k])
        for k in ("probability", "log_probability", "log_prior", "map_weight_share"):
            d[k] = float(d[k])
        return d
    ann = [annotation(d) for d in table(prefix + ".annotations.tsv")]
    best = [annotation(d) for d in table(prefix + ".best.tsv")]
    rows = [dict(row=int(d["row"]), lh_loglik=float(d["lh_loglik"]), log_weight=float(d["log_weight"]),
                 log_path_posterior=float(d["log_path_posterior"]),
                 annotation=None if d["annotation"] == "NA" else int(d["annotation"])) for d in table(prefix + ".rows.tsv")]
    summary = {d["key"]: float(d["value"]) if d["key"] in ("kish_ess", "covered_mass") else int(d["value"])
               for d in table(prefix + ".summary.tsv")}
    return dict(annotations=ann, best=best[0] if best else None, rows=rows, summary=summary)


def read_lineage(prefix):
    """The files RunLineagePipeline / RunWeightedLineagePipeline / tabulate_lineage_trees write: dict(fasta = [(name, aa)]
    of <prefix>.fasta, dnamap = {name: [(fraction, dna)]} of <prefix>.dnamap, nodes = [dict(name, kind, count, fraction)]
    of <prefix>.nodes.tsv, edges = [dict(parent, child, count, fraction, parent_fraction, mutations = list)] of
    <prefix>.edges.tsv, summary = {key: int, kish_ess: float} of <prefix>.summary.tsv), all in file order.  Counts are
    ints, or floats in weighted tables.  With <prefix>.rows.tsv (the weighted pipeline) also rows = [dict(row, lh_loglik,
    log_weight, weight, naive_id, path_len)]."""
    fa = open(prefix + ".fasta").read().strip("\n").split("\n")
    fasta = [(fa[i][1:], fa[i + 1]) for i in range(0, len(fa) - 1, 2)]

    def table(path):
        lines = open(path).read().strip("\n").split("\n")
        head = lines[0].split("\t")
        return [dict(zip(head, ln.split("\t") + [""] * (len(head) - len(ln.split("\t"))))) for ln in lines[1:]]

    def count(text):
        return int(text) if text.lstrip("-").isdigit() else float(text)

    nodes = [dict(name=d["name"], kind=d["kind"], count=count(d["count"]), fraction=float(d["fraction"]))
             for d in table(prefix + ".nodes.tsv")]
    edges = [dict(parent=d["parent"], child=d["child"], count=count(d["count"]), fraction=float(d["fraction"]),
                  parent_fraction=float(d["parent_fraction"]), mutations=d["mutations"].split())
             for d in table(prefix + ".edges.tsv")]
    summary = {d["key"]: float(d["value"]) if d["key"] == "kish_ess" else int(d["value"])
               for d in table(prefix + ".summary.tsv")}
    out = dict(fasta=fasta, dnamap=_parse_dnamap(open(prefix + ".dnamap").read()), nodes=nodes, edges=edges,
               summary=summary)
    if os.path.exists(prefix + ".rows.tsv"):
        out["rows"] = [dict(row=int(d["row"]), lh_loglik=float(d["lh_loglik"]), log_weight=float(d["log_weight"]),
                            weight=float(d["weight"]), naive_id=int(d["naive_id"]), path_len=int(d["path_len"]))
                       for d in table(prefix + ".rows.tsv")]
    return out


def tabulate_lineage_trees(trees_path, seed_seq, output_prefix, weights_path=None):
    """Lineage.hpp TabulateLineageTrees (tabulate_lineage_probs.py on a file PhyloHMM.run_asr wrote; no family, no
    GPU); weights_path: one log-weight per tree line (tree k counts exp(lw_k - max lw)).  Returns
    read_lineage(output_prefix)."""
    lib = load_host()
    if weights_path is None:
        lib.lhh_lineage_tabulate_trees.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        _check(lib.lhh_lineage_tabulate_trees(trees_path.encode(), seed_seq.encode(), output_prefix.encode()))
    else:
        lib.lhh_lineage_tabulate_trees_weighted.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
        _check(lib.lhh_lineage_tabulate_trees_weighted(trees_path.encode(), seed_seq.encode(), output_prefix.encode(),
                                                       weights_path.encode()))
    return read_lineage(output_prefix)


def translate(dna):
    """The host's translation (NaiveProbs.hpp TranslateDna)."""
    out = C.c_char_p()
    _check(load_host().lhh_translate(dna.encode(), C.byref(out)))
    return out.value.decode()


def repr_double(v):
    """The host's repr(float) formatting (NaiveProbs.hpp ReprDouble)."""
    out = C.c_char_p()
    lib = load_host()
    lib.lhh_repr_double.argtypes = [C.c_double, C.POINTER(C.c_char_p)]
    _check(lib.lhh_repr_double(v, C.byref(out)))
    return out.value.decode()


def read_candidates(path, n_sites):
    """The host's candidate-file reader: the sequences (raises RuntimeError with its message on a refusal)."""
    out = C.c_char_p()
    _check(load_host().lhh_read_candidates(path.encode(), n_sites, C.byref(out)))
    return out.value.decode().split()


def naive_probs_write(seqs, prob, log_prior, count=None, freq=None):
    """The host writers on caller data: (.naive.tsv, .aa.fasta, .dnamap) texts."""
    K = len(seqs)
    lib = load_host()
    lib.lhh_naive_probs_write.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_char_p)]
    p, lp = np.ascontiguousarray(prob, dtype=np.float64), np.ascontiguousarray(log_prior, dtype=np.float64)
    c = None if count is None else np.ascontiguousarray(count, dtype=np.int64)
    f = None if freq is None else np.ascontiguousarray(freq, dtype=np.float64)
    out = C.c_char_p()
    _check(lib.lhh_naive_probs_write(K, "\n".join(seqs).encode(), p.ctypes.data, lp.ctypes.data,
                                     None if c is None else c.ctypes.data, None if f is None else f.ctypes.data,
                                     C.byref(out)))
    a, b, d = out.value.decode().split("\x1e\n")
    return a, b, d


class _HMM:
    def __init__(self, handle):
        self.h = handle
        self.lib = load_host()

    def close(self):
        if self.h:
            self.lib.lhh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dump(self, what):
        """what: bit 0 state space + transitions, bit 1 forward arrays, bit 2 sample, bit 3 xMSA."""
        out = C.c_char_p()
        _check(self.lib.lhh_dump_json(self.h, what, C.byref(out)))
        return json.loads(out.value.decode())

    def log_likelihood(self):
        v = C.c_double()
        _check(self.lib.lhh_loglikelihood(self.h, C.byref(v)))
        return v.value

    def sample_naive_sequence(self):
        out = C.c_char_p()
        _check(self.lib.lhh_sample(self.h, C.byref(out)))
        return out.value.decode()


class SimpleHMM(_HMM):
    def __init__(self, yaml_path, cluster_ind, hmm_param_dir, seed):
        h = C.c_void_p()
        _check(load_host().lhh_simple_create(yaml_path.encode(), cluster_ind, hmm_param_dir.encode(), seed,
                                             C.byref(h)))
        super().__init__(h)

    def viterbi_path(self):
        """(naive sequence of the most probable state path, log P(data, path)): SimpleHMM::ViterbiPath (K8)."""
        lp, out = C.c_double(), C.c_char_p()
        self.lib.lhh_simple_viterbi_path.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        _check(self.lib.lhh_simple_viterbi_path(self.h, C.byref(lp), C.byref(out)))
        return out.value.decode(), lp.value


class PhyloHMM(_HMM):
    def __init__(self, yaml_path, cluster_ind, hmm_param_dir, seed):
        h = C.c_void_p()
        _check(load_host().lhh_phylo_create(yaml_path.encode(), cluster_ind, hmm_param_dir.encode(), seed,
                                            C.byref(h)))
        super().__init__(h)

    def initialize_phylo_parameters(self, newick, er, pi, alpha, num_rates, is_path=True):
        er = (C.c_double * 6)(*er)
        pi = (C.c_double * 4)(*pi)
        f = self.lib.lhh_phylo_init_parameters if is_path else self.lib.lhh_phylo_init_parameters_str
        _check(f(self.h, newick.encode(), er, pi, C.c_double(alpha), num_rates))

    def initialize_phylo_emission(self):
        _check(self.lib.lhh_phylo_init_emission(self.h))

    def set_extended_range(self, on=True):
        _check(self.lib.lhh_phylo_set_extended_range(self.h, int(on)))

    def sample_states_with_words(self, words):
        """(device states, host states) of one SampleNaiveSequence whose engine outputs are `words` (test entry)."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        d = np.zeros(4096, dtype=np.int32)
        s = np.zeros(4096, dtype=np.int32)
        n = C.c_int()
        self.lib.lhh_phylo_sample_words.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.POINTER(C.c_int)]
        _check(self.lib.lhh_phylo_sample_words(self.h, w.ctypes.data, len(w), d.ctypes.data, s.ctypes.data, 4096,
                                               C.byref(n)))
        return d[:n.value].copy(), s[:n.value].copy()

    def naive_posterior(self):
        """(compact posterior [lh_forward_size], log-likelihood) of the current tree: K0-K2 + K5 on the device."""
        self.lib.lhh_phylo_posterior.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_double)]
        n, ll = C.c_int(), C.c_double()
        _check(self.lib.lhh_phylo_posterior(self.h, None, 0, C.byref(n), None))
        buf = np.zeros(n.value)
        _check(self.lib.lhh_phylo_posterior(self.h, buf.ctypes.data, n.value, C.byref(n), C.byref(ll)))
        return buf, ll.value

    def dense_posteriors(self):
        """Exact state posteriors of the current tree in the shapes of the forward members (dump(2)): vgerm, vd_junction,
        dgerm, dj_junction, jgerm."""
        from . import posterior
        return posterior.dense_posteriors(self.dump(1), self.naive_posterior()[0])

    def naive_marginals(self):
        """(site_base [L][5] over A, C, G, T, N; {"V"|"D"|"J": {gene: posterior}}) of the current tree
        (PhyloHMM::NaiveMarginals)."""
        L = self.sizes()["n_sites"]
        sb = np.zeros((L, 5))
        out = C.c_char_p()
        self.lib.lhh_phylo_naive_marginals.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
        _check(self.lib.lhh_phylo_naive_marginals(self.h, sb.ctypes.data, L, C.byref(out)))
        return sb, _parse_gene_table(out.value.decode())

    def ancestral_marginals(self, seed_seq):
        """PhyloHMM::AncestralMarginals of the current tree: dict(nodes [P] -- the lineage of the tip `seed_seq`, slot 0 its
        parent, the last slot the MRCA --, marg [P][L][4], rate_post [L][R], loglik)."""
        sz = self.sizes()
        T, L = sz["n_tips"], sz["n_sites"]
        lib = self.lib
        lib.lhh_phylo_ancestral_marginals.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        n, r, ll = C.c_int(), C.c_int(), C.c_double()
        _check(lib.lhh_phylo_ancestral_marginals(self.h, seed_seq.encode(), None, None, None, 0, C.byref(n), C.byref(r), None))
        P, R = n.value, r.value
        nodes = np.zeros(P, dtype=np.int32)
        marg = np.zeros((P, L, 4))
        rate_post = np.zeros((L, R))
        _check(lib.lhh_phylo_ancestral_marginals(self.h, seed_seq.encode(), nodes.ctypes.data, marg.ctypes.data,
                                                 rate_post.ctypes.data, P, C.byref(n), C.byref(r), C.byref(ll)))
        return dict(nodes=nodes.tolist(), marg=marg, rate_post=rate_post, loglik=ll.value)

    def run_ancestral_marginals_pipeline(self, input_path, seed_seq, output_prefix, num_rates, burnin_frac=0.0):
        """PhyloHMM::RunAncestralMarginalsPipeline: importance-weighted exact tables of the seed's parent and of the MRCA and
        the rate posteriors over a RevBayes table; returns read_ancestral_marginals(output_prefix)."""
        self.lib.lhh_run_ancestral_marginals_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                                                  C.c_double]
        _check(self.lib.lhh_run_ancestral_marginals_pipeline(self.h, input_path.encode(), seed_seq.encode(),
                                                             output_prefix.encode(), num_rates, C.c_double(burnin_frac)))
        return read_ancestral_marginals(output_prefix)

    def ancestral_candidate_posterior(self, seed_seq, node, candidates):
        """PhyloHMM::AncestralCandidatePosterior of the current tree: dict(log_cand [K], node, loglik) for candidate strings
        over ACGTN (N leaves the site open) at node 0 / "parent" (the seed's parent) or 1 / "mrca"."""
        at, node, node_t = _node_arg(node)
        lib = self.lib
        f = getattr(lib, "lhh_phylo_ancestral_candidate_posterior" + at)
        f.argtypes = [C.c_void_p, C.c_char_p, node_t, C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        lc = np.zeros(len(candidates))
        v, ll = C.c_int(), C.c_double()
        _check(f(self.h, seed_seq.encode(), node, "\n".join(candidates).encode(), len(candidates), lc.ctypes.data, C.byref(v),
                 C.byref(ll)))
        return dict(log_cand=lc, node=v.value, loglik=ll.value)

    def run_ancestral_probs_pipeline(self, input_path, seed_seq, node, candidates_path, output_prefix, num_rates,
                                     burnin_frac=0.0):
        """PhyloHMM::RunAncestralProbsPipeline: importance-weighted exact probabilities of the candidate sequences of a file
        at the seed's parent or MRCA over a RevBayes table; returns read_ancestral_probs(output_prefix)."""
        at, node, node_t = _node_arg(node)
        f = getattr(self.lib, "lhh_run_ancestral_probs_pipeline" + at)
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, node_t, C.c_char_p, C.c_char_p, C.c_int, C.c_double]
        _check(f(self.h, input_path.encode(), seed_seq.encode(), node, candidates_path.encode(), output_prefix.encode(),
                 num_rates, C.c_double(burnin_frac)))
        return read_ancestral_probs(output_prefix)

    def node_codon_marginals(self, seed_seq, node, frame=0):
        """PhyloHMM::NodeCodonMarginals of the current tree: dict(codons [n_codons][64], change [n_codons][4], aa, node,
        loglik) at node 0 / "parent" (the seed's parent) or 1 / "mrca"; aa as the host's writer folds it."""
        at, node, node_t = _node_arg(node)
        lib = self.lib
        f = getattr(lib, "lhh_phylo_node_codon_marginals" + at)
        f.argtypes = [C.c_void_p, C.c_char_p, node_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                      C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        nc, v, ll, text = C.c_int(), C.c_int(), C.c_double(), C.c_char_p()
        _check(f(self.h, seed_seq.encode(), node, frame, None, None, 0, C.byref(nc), None, None,
                                                  None))
        codons, change = np.zeros((nc.value, 64)), np.zeros((nc.value, 4))
        _check(f(self.h, seed_seq.encode(), node, frame, codons.ctypes.data, change.ctypes.data,
                                                  nc.value, C.byref(nc), C.byref(v), C.byref(ll), C.byref(text)))
        return dict(codons=codons, change=change, aa=parse_node_codons(text.value.decode())["aa"], node=v.value,
                    loglik=ll.value)

    def run_node_codons_pipeline(self, input_path, seed_seq, node, output_prefix, num_rates, burnin_frac=0.0, frame=0):
        """PhyloHMM::RunNodeCodonsPipeline: the importance-weighted codon, amino-acid and change tables of the seed's parent
        or MRCA over a RevBayes table; returns read_node_codons(output_prefix)."""
        at, node, node_t = _node_arg(node)
        f = getattr(self.lib, "lhh_run_node_codons_pipeline" + at)
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, node_t, C.c_char_p, C.c_int, C.c_double, C.c_int]
        _check(f(self.h, input_path.encode(), seed_seq.encode(), node, output_prefix.encode(), num_rates,
                 C.c_double(burnin_frac), frame))
        return read_node_codons(output_prefix)

    def lineage_replacements(self, seed_seq, frame=0):
        """PhyloHMM::LineageReplacements of the current tree: dict(nodes [P] -- the lineage of the tip `seed_seq`, slot 0 its
        parent --, codon_counts [n_codons][4], aa_counts [n_codons][21][21], seed_change [n_codons][3], edge_change
        [P + 1][n_codons][3] and edge_load [P + 1][2] (the last entry the naive edge), loglik, text as the writers print the
        first three)."""
        lib = self.lib
        lib.lhh_phylo_lineage_replacements.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                                       C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        nc, ne, ll, text = C.c_int(), C.c_int(), C.c_double(), C.c_char_p()
        _check(lib.lhh_phylo_lineage_replacements(self.h, seed_seq.encode(), frame, None, None, None, 0, None, None, None, 0,
                                                  C.byref(nc), C.byref(ne), None, None))
        n = nc.value
        cc, aa, sc = np.zeros((n, 4)), np.zeros((n, 21, 21)), np.zeros((n, 3))
        cap = 64
        while True:  # (the chain's length is known once the tree has been evaluated: a longer one is fetched again)
            ec, el, nodes = np.zeros((cap, n, 3)), np.zeros((cap, 2)), np.zeros(cap, dtype=np.int32)
            _check(lib.lhh_phylo_lineage_replacements(self.h, seed_seq.encode(), frame, cc.ctypes.data, aa.ctypes.data,
                                                      sc.ctypes.data, n, ec.ctypes.data, el.ctypes.data, nodes.ctypes.data, cap,
                                                      C.byref(nc), C.byref(ne), C.byref(ll), C.byref(text)))
            if ne.value <= cap:
                break
            cap = ne.value
        E = ne.value
        return dict(nodes=nodes[:E - 1].tolist(), codon_counts=cc, aa_counts=aa, seed_change=sc, edge_change=ec[:E],
                    edge_load=el[:E], loglik=ll.value, text=text.value.decode())

    def run_lineage_replacements_pipeline(self, input_path, seed_seq, output_prefix, num_rates, burnin_frac=0.0, frame=0):
        """PhyloHMM::RunLineageReplacementsPipeline: the importance-weighted amino-acid replacement, codon change and seed-edge
        tables of the seed's lineage over a RevBayes table; returns read_lineage_replacements(output_prefix)."""
        self.lib.lhh_run_lineage_replacements_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                                                   C.c_double, C.c_int]
        _check(self.lib.lhh_run_lineage_replacements_pipeline(self.h, input_path.encode(), seed_seq.encode(),
                                                              output_prefix.encode(), num_rates, C.c_double(burnin_frac), frame))
        return read_lineage_replacements(output_prefix)

    def lineage_substitutions(self, seed_seq):
        """PhyloHMM::LineageSubstitutions of the current tree: dict(nodes [P] -- the lineage of the tip `seed_seq`, slot 0 its
        parent, the last slot the MRCA --, edges [(upper node, lower node, branch length, expected differing sites)] of
        length P + 1 ([s] the edge below slot s, [P] naive -> MRCA), edge [P][L][4][4], naive_edge [L][5][4],
        chain_counts [L][4][4], loglik); tables indexed [ancestor base][descendant base]."""
        sz = self.sizes()
        T, L = sz["n_tips"], sz["n_sites"]
        lib = self.lib
        lib.lhh_phylo_lineage_substitutions.argtypes = [C.c_void_p, C.c_char_p] + [C.c_void_p] * 5 + \
            [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        cap = T - 2
        nodes = np.zeros(cap, dtype=np.int32)
        edge, ne, cc, edges = np.zeros((cap, L, 4, 4)), np.zeros((L, 5, 4)), np.zeros((L, 4, 4)), np.zeros((cap + 1, 4))
        n, ll = C.c_int(), C.c_double()
        _check(lib.lhh_phylo_lineage_substitutions(self.h, seed_seq.encode(), nodes.ctypes.data, edge.ctypes.data, ne.ctypes.data,
                                                   cc.ctypes.data, edges.ctypes.data, cap, C.byref(n), C.byref(ll)))
        P = n.value
        return dict(nodes=nodes[:P].tolist(), edges=[(int(e[0]), int(e[1]), float(e[2]), float(e[3])) for e in edges[:P + 1]],
                    edge=edge[:P].copy(), naive_edge=ne, chain_counts=cc, loglik=ll.value)

    def run_lineage_substitutions_pipeline(self, input_path, seed_seq, output_prefix, num_rates, burnin_frac=0.0):
        """PhyloHMM::RunLineageSubstitutionsPipeline: importance-weighted exact substitution tables of the seed's lineage over
        a RevBayes table; returns read_lineage_substitutions(output_prefix)."""
        self.lib.lhh_run_lineage_substitutions_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                                                    C.c_double]
        _check(self.lib.lhh_run_lineage_substitutions_pipeline(self.h, input_path.encode(), seed_seq.encode(),
                                                               output_prefix.encode(), num_rates, C.c_double(burnin_frac)))
        return read_lineage_substitutions(output_prefix)

    def run_marginals_pipeline(self, input_path, output_prefix, num_rates, burnin_frac=0.0):
        """PhyloHMM::RunMarginalsPipeline: importance-weighted exact marginals over a RevBayes table (burn-in
        floor(burnin_frac * rows), weights exp(LHLogLikelihood - RBLogLikelihood)).  Writes <prefix>.sites.tsv,
        .genes.tsv and .summary.tsv and returns (site_base, genes, summary) read back from them."""
        self.lib.lhh_run_marginals_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double]
        _check(self.lib.lhh_run_marginals_pipeline(self.h, input_path.encode(), output_prefix.encode(), num_rates,
                                                   C.c_double(burnin_frac)))
        return read_marginals(output_prefix)

    def naive_codon_marginals(self, frame=0):
        """(table [n_codons][125] over 25 b1 + 5 b2 + b3, [per codon {amino acid: p}]) of the current tree
        (PhyloHMM::NaiveCodonMarginals, K9)."""
        f = self.lib.lhh_phylo_codon_marginals
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
        n, out = C.c_int(), C.c_char_p()
        _check(f(self.h, frame, None, 0, C.byref(n), C.byref(out)))
        table = np.zeros((n.value, 125))
        _check(f(self.h, frame, table.ctypes.data, n.value, C.byref(n), C.byref(out)))
        return table, _parse_aa_table(out.value.decode(), n.value)

    def run_codon_marginals_pipeline(self, input_path, output_prefix, num_rates, burnin_frac=0.0, frame=0):
        """PhyloHMM::RunCodonMarginalsPipeline: importance-weighted exact codon and amino-acid tables over a RevBayes
        table.  Writes <prefix>.codons.tsv, .aa.tsv and .summary.tsv and returns read_codon_marginals(prefix)."""
        f = self.lib.lhh_run_codon_marginals_pipeline
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int]
        _check(f(self.h, input_path.encode(), output_prefix.encode(), num_rates, C.c_double(burnin_frac), frame))
        return read_codon_marginals(output_prefix)

    def events_sizes(self):
        """(length of K10's flat row, number of gene posteriors nV + nD + nJ) for this family; no device."""
        f = self.lib.lhh_phylo_events_sizes
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        size, ng = C.c_int64(), C.c_int()
        _check(f(self.h, C.byref(size), C.byref(ng)))
        return size.value, ng.value

    def map_events(self, events, genes):
        """PhyloHMM::MapEvents on one flat row and the V | D | J gene posteriors (no device): parse_events' dict."""
        size, ng = self.events_sizes()
        events, genes = np.ascontiguousarray(events, dtype=np.float64), np.ascontiguousarray(genes, dtype=np.float64)
        if events.shape != (size,) or genes.shape != (ng,):
            raise ValueError("map_events: the row must hold %d entries and the genes %d" % (size, ng))
        f = self.lib.lhh_phylo_map_events
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]
        out = C.c_char_p()
        _check(f(self.h, events.ctypes.data, genes.ctypes.data, C.byref(out)))
        return parse_events(*out.value.decode().split("\n\n"))

    def rearrangement_events(self):
        """parse_events' dict for the current tree (PhyloHMM::RearrangementEvents, K10): exact posteriors of the deletion
        lengths per gene, of the insertion lengths and of the junction spans."""
        f = self.lib.lhh_phylo_events
        f.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
        out = C.c_char_p()
        _check(f(self.h, C.byref(out)))
        return parse_events(*out.value.decode().split("\n\n"))

    def run_events_pipeline(self, input_path, output_prefix, num_rates, burnin_frac=0.0):
        """PhyloHMM::RunEventsPipeline: importance-weighted exact deletion, insertion and span tables over a RevBayes
        table.  Writes <prefix>.deletions.tsv, .insertions.tsv, .spans.tsv and .summary.tsv and returns
        read_events(prefix)."""
        f = self.lib.lhh_run_events_pipeline
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double]
        _check(f(self.h, input_path.encode(), output_prefix.encode(), num_rates, C.c_double(burnin_frac)))
        return read_events(output_prefix)

    def viterbi_annotation(self):
        """The most probable annotation of the current tree (PhyloHMM::ViterbiAnnotation, K8): (dict of the annotation
        columns NaiveSequence, VGene, ... as strings, log P(data, path | tree), log-likelihood)."""
        lp, ll, out = C.c_double(), C.c_double(), C.c_char_p()
        self.lib.lhh_phylo_viterbi_annotation.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                          C.POINTER(C.c_char_p)]
        _check(self.lib.lhh_phylo_viterbi_annotation(self.h, C.byref(lp), C.byref(ll), C.byref(out)))
        head, vals = out.value.decode().split("\n")
        vals = vals.split("\t")
        head = head.split("\t")
        return dict(zip(head, vals + [""] * (len(head) - len(vals)))), lp.value, ll.value

    def annotation_columns(self, states):
        """The annotation columns (NaiveSequence, VGene, ... tab-separated, as the annotation files print them) of state
        vectors states [n][S] in lh_eval_sample_batch's layout: HMM::ApplySampledStates on the host."""
        st = np.ascontiguousarray(states, dtype=np.int32)
        out = C.c_char_p()
        self.lib.lhh_phylo_annotation_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_char_p)]
        _check(self.lib.lhh_phylo_annotation_columns(self.h, st.shape[0], st.shape[1], st.ctypes.data, C.byref(out)))
        return out.value.decode().split("\n")[:st.shape[0]]

    def run_annotations_pipeline(self, input_path, output_prefix, num_rates, burnin_frac=0.0, max_candidates=65536):
        """PhyloHMM::RunAnnotationsPipeline; returns read_annotations(output_prefix)."""
        self.lib.lhh_run_annotations_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int]
        _check(self.lib.lhh_run_annotations_pipeline(self.h, input_path.encode(), output_prefix.encode(), num_rates,
                                                     C.c_double(burnin_frac), max_candidates))
        return read_annotations(output_prefix)

    def candidate_posterior(self, seqs):
        """(log P(s | data, tree) [K], log-likelihood, log P_HMM(s) [K]) of ACGTN candidate strings for the current tree
        (PhyloHMM::CandidatePosterior; -inf for a sequence no state path writes)."""
        K = len(seqs)
        lp, pr = np.zeros(K), np.zeros(K)
        ll = C.c_double()
        self.lib.lhh_phylo_candidate_posterior.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_double)]
        _check(self.lib.lhh_phylo_candidate_posterior(self.h, K, "".join(seqs).encode(), lp.ctypes.data, pr.ctypes.data,
                                                      C.byref(ll)))
        return lp, ll.value, pr

    def naive_sequences(self, states):
        """K6c and HMM::ApplySampledStates on the same states [n][S]: (device bytes [n][L], hashes [n], host strings)."""
        st = np.ascontiguousarray(states, dtype=np.int32)
        n = st.shape[0]
        L = self.sizes()["n_sites"]
        seqs = np.zeros((n, L), dtype=np.uint8)
        hsh = np.zeros(n, dtype=np.uint64)
        host = C.create_string_buffer(n * L + 1)
        self.lib.lhh_phylo_naive_sequences.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
        _check(self.lib.lhh_phylo_naive_sequences(self.h, n, st.ctypes.data, seqs.ctypes.data, hsh.ctypes.data, host))
        raw = host.raw[:n * L].decode()
        return seqs, hsh, [raw[i * L:(i + 1) * L] for i in range(n)]

    def run_naive_probs_pipeline(self, input_path, output_prefix, num_rates, burnin_frac=0.0, candidates_path=None,
                                 max_candidates=65536):
        """PhyloHMM::RunNaiveProbsPipeline; returns read_naive_probs(output_prefix)."""
        self.lib.lhh_run_naive_probs_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double,
                                                          C.c_char_p, C.c_int]
        _check(self.lib.lhh_run_naive_probs_pipeline(self.h, input_path.encode(), output_prefix.encode(), num_rates,
                                                     C.c_double(burnin_frac),
                                                     candidates_path.encode() if candidates_path else None,
                                                     max_candidates))
        return read_naive_probs(output_prefix)

    def run_pipeline(self, input_path, output_path, num_rates):
        _check(self.lib.lhh_run_pipeline(self.h, input_path.encode(), output_path.encode(), num_rates))

    def run_lineage_pipeline(self, input_path, seed_seq, output_prefix, seed):
        """PhyloHMM::RunLineagePipeline; returns read_lineage(output_prefix)."""
        self.lib.lhh_run_lineage_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64]
        _check(self.lib.lhh_run_lineage_pipeline(self.h, input_path.encode(), seed_seq.encode(), output_prefix.encode(),
                                                 seed))
        return read_lineage(output_prefix)

    def run_weighted_lineage_pipeline(self, input_path, seed_seq, output_prefix, num_rates, burnin_frac=0.0,
                                      draws_per_row=1, seed=0):
        """PhyloHMM::RunWeightedLineagePipeline on a RevBayes table: importance-weighted lineage tables in one pass;
        returns read_lineage(output_prefix) (with the weighted summary keys and the rows table)."""
        self.lib.lhh_run_weighted_lineage_pipeline.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                                               C.c_double, C.c_int, C.c_uint64]
        _check(self.lib.lhh_run_weighted_lineage_pipeline(self.h, input_path.encode(), seed_seq.encode(),
                                                          output_prefix.encode(), num_rates, C.c_double(burnin_frac),
                                                          draws_per_row, seed))
        return read_lineage(output_prefix)

    def run_asr(self, input_path, output_path, seed):
        lib = load_host()
        lib.lhh_run_asr.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64]
        _check(lib.lhh_run_asr(self.h, input_path.encode(), output_path.encode(), seed))

    def sizes(self):
        v = [C.c_int() for _ in range(8)]
        _check(self.lib.lhh_phylo_sizes(self.h, *[C.byref(x) for x in v]))
        keys = ["n_tips", "n_sites", "n_xmsa", "s_vd", "s_dj", "w_vd", "w_dj", "g_total"]
        return {k: x.value for k, x in zip(keys, v)}

    def set_devices(self, devices):
        """The HIP devices run_pipeline deals the table's rows to (before the first evaluation)."""
        arr = (C.c_int * len(devices))(*devices)
        _check(self.lib.lhh_phylo_set_devices(self.h, arr, len(devices)))

    def flatten_tsv(self, tsv_path, n, need_family=True, rows=None):
        """Device-ready inputs for lh_eval_batch_device: n samples taken cyclically from the table, or -- rows given --
        the table rows rows[0..n) in that order (only those are parsed: a rank flattens what it evaluates).
        Returns dict(ops, brlen, er, pi, alpha, n_tips, max_depth, n_rows, family)."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            n = len(rows)
        n_tips, depth, n_rows = C.c_int(), C.c_int(), C.c_int()
        fam = C.c_void_p()
        flag = C.c_int(1 if need_family else 0)
        T = self.sizes()["n_tips"]
        ops = np.zeros((n, T - 2, 4), dtype=np.int32)
        brlen = np.zeros((n, 2 * T - 2))
        er, pi, alpha = np.zeros((n, 6)), np.zeros((n, 4)), np.zeros(n)

        def p(a, t):
            return a.ctypes.data_as(C.POINTER(t))
        if rows is not None:
            _check(self.lib.lhh_phylo_flatten_tsv_rows(self.h, tsv_path.encode(), n, p(rows, C.c_int64), p(ops, C.c_int32),
                                                       p(brlen, C.c_double), p(er, C.c_double), p(pi, C.c_double),
                                                       p(alpha, C.c_double), C.byref(n_tips), C.byref(depth),
                                                       C.byref(n_rows), flag, C.byref(fam)))
        else:
            _check(self.lib.lhh_phylo_flatten_tsv(self.h, tsv_path.encode(), n, p(ops, C.c_int32),
                                                  p(brlen, C.c_double), p(er, C.c_double), p(pi, C.c_double),
                                                  p(alpha, C.c_double), C.byref(n_tips), C.byref(depth),
                                                  C.byref(n_rows), flag, C.byref(fam)))
        assert n_tips.value == T
        return dict(ops=ops, brlen=brlen, er=er, pi=pi, alpha=alpha, n_tips=T, max_depth=depth.value,
                    n_rows=n_rows.value, family=fam.value)
