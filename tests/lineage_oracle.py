"""Plain-Python restatement of scripts/tabulate_lineage_probs.py of matsengrp/linearham -- TEST INFRASTRUCTURE ONLY.

The script reads a file of annotated Newick trees (one per tree sample, every node carrying [&ancestral="<bases>"], as
scripts/run_bootstrap_asr_ess.R:86-101 and PhyloHMM::RunAsr write them), walks from the seed tip up to the top node and
on to the tip `naive` (seqs_of_tree, :46-63), and counts over the trees (:95-144) with collections.Counter,
itertools.groupby and frozenset.  This file does the same with the same three tools.

PARITY STATUS: **unpinned**.  The script needs dendropy, Biopython and graphviz; none is in this image, so it was never
run here and no fixture of its output exists.  This is a restatement written by us.  What differs from the script, on
purpose:
  * the tree parser below (parent links, tip labels, the ancestral annotation) stands in for dendropy;
  * the codon table below stands in for Bio.Seq.translate.  The one rule Biopython could decide differently is a codon
    with N whose resolutions mix a stop with an amino acid (TAN): we keep the host's TranslateDna rule, X;
  * a frozenset of strings has no fixed iteration order (string hashes are salted per process), so the script's order
    of "first appearance" inside one tree -- which decides ties in most_common() -- changes from run to run.  Here a
    frozenset is iterated in the order of first appearance in the list it was made from (`_in_order`);
  * pairs of equal translations are counted by the script and never shown (`if a == b: continue`); they are left out;
  * the graphviz rendering is left out; `edges` holds what the script's loop over edge_c draws for pfilter = 0.
No product code is called from here.
"""
import collections
import itertools

_CODE = dict(zip(("".join(c) for c in itertools.product("TCAG", repeat=3)),
                 "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"))


def translate_codon(codon):
    if any(ch not in "ACGTN" for ch in codon):
        return "X"
    res = {_CODE["".join(r)] for r in itertools.product(*[("TCAG" if ch == "N" else ch) for ch in codon])}
    return res.pop() if len(res) == 1 else "X"


_CACHE = {}


def translate(s):
    """util_functions.translate: frame 0, truncated to a multiple of three."""
    if s not in _CACHE:
        _CACHE[s] = "".join(translate_codon(s[i:i + 3]) for i in range(0, 3 * (len(s) // 3), 3))
    return _CACHE[s]


def find_muts(orig, mutated):
    return ["{}{}{}".format(o, idx + 1, m) for idx, (o, m) in enumerate(zip(orig, mutated)) if o != m]


def parse_annotated_newick(text):
    """[(parent index or None, label, ancestral or None, is_tip)] in order of appearance."""
    nodes, open_, last, k = [], [], None, 0

    def fresh():
        nodes.append([open_[-1] if open_ else None, "", None, True])
        return len(nodes) - 1

    while k < len(text):
        c = text[k]
        if c == "(":
            v = fresh()
            nodes[v][3] = False
            open_.append(v)
            last = None
            k += 1
        elif c == ",":
            last = None
            k += 1
        elif c == ")":
            last = open_.pop()
            k += 1
        elif c == ";":
            break
        elif c == "[":
            e = text.index("]", k)
            if last is None:
                last = fresh()
            body = text[k + 1:e]
            if body.startswith('&ancestral="'):
                nodes[last][2] = body[len('&ancestral="'):body.rindex('"')]
            k = e + 1
        elif c == ":":
            k += 1
            while k < len(text) and text[k] not in "(),;[":
                k += 1
        elif c in " \t\r\n":
            k += 1
        else:
            if last is None:
                last = fresh()
            b = k
            while k < len(text) and text[k] not in "(),;[:":
                k += 1
            nodes[last][1] += text[b:k]
    assert not open_
    return nodes


def seqs_of_tree(text, seed):
    """seqs_of_tree (:46-63): the annotations of seed, its ancestors up to the top node, then `naive`."""
    nodes = parse_annotated_newick(text)
    tips = {n[1]: i for i, n in enumerate(nodes) if n[3]}
    if seed not in tips:
        raise Exception("seed node with label '%s' not found in tree" % seed)
    lineage = [tips[seed]]
    while nodes[lineage[-1]][0] is not None:
        lineage.append(nodes[lineage[-1]][0])
    lineage.append(tips["naive"])
    return [nodes[v][2] for v in lineage]


def _in_order(fs, source):
    """The members of frozenset `fs` in the order of their first appearance in `source`."""
    return [x for x in dict.fromkeys(source) if x in fs]


def naive_names(naive_aa):
    """tabulate_naive_probs.py:57-60 over the trees' naive translations: {aa: naive_<i>_<count / num_trees>}."""
    c = collections.Counter(naive_aa)
    return {seq: "naive_" + str(i) + "_" + str(float(count) / len(naive_aa))
            for i, (seq, count) in enumerate(c.most_common(None))}


def tabulate(lineages, seed_name):
    """The counting of :95-144 on `lineages`: per tree the list naive, ..., seed (the script's reversed `l`).
    Returns dict(num_trees, node_c, node_dt, edge_c, names = {aa: name}, order = [aa] in most_common order,
    fasta / dnamap = the two files' text, nodes = [(name, kind, count)], edges = [(parent name, child name, count,
    mutations)] in most_common order)."""
    node_c = collections.Counter()
    node_dt = {}
    edge_c = collections.Counter()
    naive_aa = []
    seed_s = set()
    num_trees = 0
    for l in lineages:
        num_trees += 1
        l = list(l)
        for k, g in itertools.groupby(l, lambda seq: translate(seq)):
            g = list(g)
            node_dt.setdefault(k, collections.Counter()).update(_in_order(frozenset(g), g))
        l = [translate(seq) for seq in l]
        node_c.update(_in_order(frozenset(l), l))
        edge_c.update((v, w) for v, w in zip(l[:-1], l[1:]) if v != w)
        naive_aa.append(l[0])
        seed_s.update([l[-1]])
    assert len(seed_s) == 1
    assert num_trees == node_c.most_common(1)[0][1]
    aa_naive_seqs = naive_names(naive_aa)
    names, kinds, order = {}, {}, []
    fasta, dnamap = [], []
    i = 0
    for s, count in node_c.most_common(None):
        if s in seed_s:
            names[s], kinds[s] = seed_name, "seed"
        elif s in aa_naive_seqs:
            names[s], kinds[s] = aa_naive_seqs[s], "naive"
        else:
            names[s], kinds[s] = "intermediate_{}_{}".format(i, float(count) / num_trees), "intermediate"
            i += 1
        order.append(s)
        fasta.append(">{}\n{}\n".format(names[s], s))
        dnamap.append(">{}\n{}\n".format(names[s], "\n".join(
            str(float(cnt) / num_trees) + "," + dna for dna, cnt in node_dt[s].most_common(None))))
    return dict(num_trees=num_trees, node_c=node_c, node_dt=node_dt, edge_c=edge_c, names=names, order=order,
                fasta="".join(fasta), dnamap="".join(dnamap),
                nodes=[(names[s], kinds[s], node_c[s]) for s in order],
                edges=[(names[a], names[b], count, find_muts(a, b)) for (a, b), count in edge_c.most_common(None)])


def tabulate_trees(lines, seed_name):
    """tabulate() on annotated Newick lines."""
    return tabulate([list(reversed(seqs_of_tree(ln, seed_name))) for ln in lines if ln.strip()], seed_name)
