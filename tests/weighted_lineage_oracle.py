"""tests/lineage_oracle.py's counting with a weight per tree -- TEST INFRASTRUCTURE ONLY.

`tabulate` below is lineage_oracle.tabulate with `+ w` where the script adds 1 and the sum of the weights where it divides
by num_trees: every Counter becomes a dict of float sums (insertion-ordered, as a Counter is), most_common() a stable sort
by descending sum.  With all weights 1 it returns lineage_oracle.tabulate's tables (sums of ones are exact).

PARITY STATUS: **unpinned**, like its parent: upstream has no weighted form of scripts/tabulate_lineage_probs.py (its
weights act through the bootstrap of scripts/run_bootstrap_asr_ess.R:29-32, which resamples rows in proportion to
exp(LogWeight)); this file states the estimate that bootstrap converges to.  No product code is called from here.
"""
import itertools
import math

from tests.lineage_oracle import _in_order, find_muts, seqs_of_tree, translate


def most_common(sums):
    """[(key, sum)] by descending sum, ties in insertion order (collections.Counter.most_common's order)."""
    return sorted(sums.items(), key=lambda kv: -kv[1])


def weights_of(log_weights):
    """w_i = exp(lw_i - max lw) over the finite entries (None for the others), and the Kish effective sample size."""
    finite = [x for x in log_weights if math.isfinite(x)]
    top = max(finite)
    w = [math.exp(x - top) if math.isfinite(x) else None for x in log_weights]
    used = [x for x in w if x is not None]
    return w, sum(used) ** 2 / sum(x * x for x in used)


def tabulate(lineages, seed_name, weights):
    """lineage_oracle.tabulate with tree k counting weights[k].  Returns dict(total, node_c, node_dt, edge_c, names,
    order, fasta, dnamap, nodes = [(name, kind, sum)], edges = [(parent, child, sum, mutations)])."""
    node_c, node_dt, edge_c, naive_c = {}, {}, {}, {}
    seed_s = set()
    total = 0.0
    for l, w in zip(lineages, weights):
        total += w
        l = list(l)
        for k, g in itertools.groupby(l, lambda seq: translate(seq)):
            g = list(g)
            dt = node_dt.setdefault(k, {})
            for dna in _in_order(frozenset(g), g):
                dt[dna] = dt.get(dna, 0.0) + w
        l = [translate(seq) for seq in l]
        for s in _in_order(frozenset(l), l):
            node_c[s] = node_c.get(s, 0.0) + w
        for v, x in zip(l[:-1], l[1:]):
            if v != x:
                edge_c[(v, x)] = edge_c.get((v, x), 0.0) + w
        naive_c[l[0]] = naive_c.get(l[0], 0.0) + w
        seed_s.update([l[-1]])
    assert len(seed_s) == 1
    assert total == most_common(node_c)[0][1]
    aa_naive_seqs = {seq: "naive_" + str(i) + "_" + str(s / total) for i, (seq, s) in enumerate(most_common(naive_c))}
    names, kinds, order = {}, {}, []
    fasta, dnamap = [], []
    i = 0
    for s, count in most_common(node_c):
        if s in seed_s:
            names[s], kinds[s] = seed_name, "seed"
        elif s in aa_naive_seqs:
            names[s], kinds[s] = aa_naive_seqs[s], "naive"
        else:
            names[s], kinds[s] = "intermediate_{}_{}".format(i, count / total), "intermediate"
            i += 1
        order.append(s)
        fasta.append(">{}\n{}\n".format(names[s], s))
        dnamap.append(">{}\n{}\n".format(names[s], "\n".join(
            str(cnt / total) + "," + dna for dna, cnt in most_common(node_dt[s]))))
    return dict(total=total, node_c=node_c, node_dt=node_dt, edge_c=edge_c, names=names, order=order,
                fasta="".join(fasta), dnamap="".join(dnamap),
                nodes=[(names[s], kinds[s], node_c[s]) for s in order],
                edges=[(names[a], names[b], count, find_muts(a, b)) for (a, b), count in most_common(edge_c)])


def tabulate_trees(lines, seed_name, log_weights):
    """tabulate() on annotated Newick lines with one log-weight per line; lines whose log-weight is not finite are left
    out.  Returns (tables, kish_ess, lines skipped)."""
    lines = [ln for ln in lines if ln.strip()]
    assert len(lines) == len(log_weights)
    w, ess = weights_of(log_weights)
    keep = [k for k in range(len(lines)) if w[k] is not None]
    t = tabulate([list(reversed(seqs_of_tree(lines[k], seed_name))) for k in keep], seed_name, [w[k] for k in keep])
    return t, ess, len(lines) - len(keep)
