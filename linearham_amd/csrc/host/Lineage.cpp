#include "Lineage.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <stdexcept>

#include "NaiveProbs.hpp"
#include "utils.hpp"

namespace linearham {

namespace {

// str(float(count) / denominator), remembered: a table has few distinct counts and ReprDouble searches for its digits
class Fractions {
 public:
  const std::string& operator()(double count, double denominator) {
    const auto r = text_.emplace(std::make_pair(count, denominator), std::string());
    if (r.second) r.first->second = ReprDouble(count / denominator);
    return r.first->second;
  }

 private:
  std::map<std::pair<double, double>, std::string> text_;
};

// a count: the integer it is when no tree had a weight of its own, else str(float)
std::string CountText(const LineageTables& t, double count) {
  return t.weighted ? ReprDouble(count) : std::to_string((int64_t)count);
}

}  // namespace

void LineageTabulator::Counted::Add(int key, double weight) {
  int pos = -1;
  if (keys.size() <= kLinear) {  // most counters hold a key or two: no index until there are many
    for (std::size_t k = 0; k < keys.size() && pos < 0; ++k)
      if (keys[k] == key) pos = (int)k;
  } else {
    if (at.empty())
      for (std::size_t k = 0; k < keys.size(); ++k) at.emplace(keys[k], (int)k);
    const auto it = at.find(key);
    if (it != at.end()) pos = it->second;
  }
  if (pos < 0) {
    pos = (int)keys.size();
    keys.push_back(key);
    counts.push_back(0);
    if (!at.empty()) at.emplace(key, pos);
  }
  counts[pos] += weight;
}

std::vector<int> LineageTabulator::Counted::MostCommon() const {
  std::vector<int> order(keys.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] > counts[b]; });
  return order;
}

int LineageTabulator::AddSequence(const std::string& nt) {
  const auto r = nt_id_.emplace(nt, (int)nt_.size());
  if (r.second) {
    nt_.push_back(nt);
    const std::string aa = TranslateDna(nt);
    const auto a = aa_id_.emplace(aa, (int)aa_.size());
    if (a.second) aa_.push_back(aa);
    aa_of_nt_.push_back(a.first->second);
  }
  return r.first->second;
}

void LineageTabulator::AddTree(const std::vector<std::string>& seqs, int path_len, double weight) {
  std::vector<int> ids;
  for (const std::string& s : seqs) ids.push_back(AddSequence(s));
  AddTree(ids, path_len, weight);
}

void LineageTabulator::AddTree(const std::vector<int>& ids, int path_len, double weight) {
  if (ids.size() < 2) throw std::runtime_error("lineage: a tree's lineage holds at least naive and the seed");
  for (int id : ids)
    if (id < 0 || id >= (int)nt_.size()) throw std::runtime_error("lineage: unknown sequence id");
  if (!(weight > 0.0) || !std::isfinite(weight)) throw std::runtime_error("lineage: a tree's weight must be positive and finite");
  ++num_trees_;
  total_ += weight;
  if (weight != 1.0) weighted_ = true;
  longest_path_ = std::max<int64_t>(longest_path_, path_len);
  std::vector<int> l;
  for (int id : ids) l.push_back(aa_of_nt_[id]);
  // node_dt: groupby(l, translate), then frozenset(g)
  for (std::size_t lo = 0; lo < l.size();) {
    std::size_t hi = lo;
    while (hi < l.size() && l[hi] == l[lo]) ++hi;
    if (node_dt_.size() < aa_.size()) node_dt_.resize(aa_.size());
    Counted& c = node_dt_[l[lo]];
    for (std::size_t k = lo; k < hi; ++k)
      if (std::find(ids.begin() + lo, ids.begin() + k, ids[k]) == ids.begin() + k) c.Add(ids[k], weight);
    lo = hi;
  }
  // node_c: frozenset(l)
  for (std::size_t k = 0; k < l.size(); ++k)
    if (std::find(l.begin(), l.begin() + k, l[k]) == l.begin() + k) node_c_.Add(l[k], weight);
  // edge_c: zip(l[:-1], l[1:]) without the pairs the script never shows
  for (std::size_t k = 0; k + 1 < l.size(); ++k) {
    if (l[k] == l[k + 1]) continue;
    const std::pair<int, int> e{l[k], l[k + 1]};
    const auto r = edge_at_.emplace(e, (int)edge_keys_.size());
    if (r.second) {
      edge_keys_.push_back(e);
      edge_counts_.push_back(0);
    }
    edge_counts_[r.first->second] += weight;
  }
  naive_c_.Add(l.front(), weight);
  if (std::find(seed_aa_.begin(), seed_aa_.end(), l.back()) == seed_aa_.end()) seed_aa_.push_back(l.back());
}

LineageTables LineageTabulator::Finish(const std::string& seed_name) const {
  if (num_trees_ == 0) throw std::runtime_error("lineage: no trees");
  if (seed_aa_.size() != 1)
    throw std::runtime_error("lineage: the seed " + seed_name + " has " + std::to_string(seed_aa_.size()) +
                             " different translations over the trees");
  LineageTables t;
  t.num_trees = num_trees_;
  t.total = total_;
  t.weighted = weighted_;
  t.distinct_nt = (int64_t)nt_.size();
  t.distinct_aa = (int64_t)aa_.size();
  t.longest_path = longest_path_;
  Fractions frac;
  std::unordered_map<int, std::string> naive_name;
  {
    int i = 0;
    for (int p : naive_c_.MostCommon())
      naive_name[naive_c_.keys[p]] =
          "naive_" + std::to_string(i++) + "_" + frac(naive_c_.counts[p], total_);
  }
  std::unordered_map<int, int> node_of_aa;
  int n_inter = 0;
  for (int p : node_c_.MostCommon()) {
    const int aa = node_c_.keys[p];
    LineageTables::Node nd;
    nd.aa = aa_[aa];
    nd.count = node_c_.counts[p];
    const auto nn = naive_name.find(aa);
    if (aa == seed_aa_[0]) {
      nd.name = seed_name;
      nd.kind = "seed";
    } else if (nn != naive_name.end()) {
      nd.name = nn->second;
      nd.kind = "naive";
    } else {
      nd.name = "intermediate_" + std::to_string(n_inter++) + "_" + frac(nd.count, total_);
      nd.kind = "intermediate";
    }
    const Counted& dt = node_dt_[aa];
    for (int q : dt.MostCommon()) nd.dna.emplace_back(dt.counts[q], nt_[dt.keys[q]]);
    node_of_aa[aa] = (int)t.nodes.size();
    t.nodes.push_back(std::move(nd));
  }
  std::vector<int> order(edge_keys_.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return edge_counts_[a] > edge_counts_[b]; });
  for (int e : order)
    t.edges.push_back({node_of_aa.at(edge_keys_[e].first), node_of_aa.at(edge_keys_[e].second), edge_counts_[e]});
  return t;
}

std::string FindMuts(const std::string& orig, const std::string& mutated) {
  std::string out;
  for (std::size_t k = 0; k < orig.size() && k < mutated.size(); ++k) {
    if (orig[k] == mutated[k]) continue;
    if (!out.empty()) out.push_back(' ');
    out += orig[k] + std::to_string(k + 1) + mutated[k];
  }
  return out;
}

void WriteLineageFasta(std::ostream& o, const LineageTables& t) {
  for (const auto& n : t.nodes) o << ">" << n.name << "\n" << n.aa << "\n";
}

void WriteLineageDnaMap(std::ostream& o, const LineageTables& t) {
  Fractions frac;
  for (const auto& n : t.nodes) {
    o << ">" << n.name << "\n";
    for (const auto& d : n.dna) o << frac(d.first, t.total) << "," << d.second << "\n";
  }
}

void WriteLineageNodes(std::ostream& o, const LineageTables& t) {
  Fractions frac;
  o << "name\tkind\tcount\tfraction\n";
  for (const auto& n : t.nodes) o << n.name << "\t" << n.kind << "\t" << CountText(t, n.count) << "\t" << frac(n.count, t.total) << "\n";
}

void WriteLineageEdges(std::ostream& o, const LineageTables& t) {
  Fractions frac;
  o << "parent\tchild\tcount\tfraction\tparent_fraction\tmutations\n";
  for (const auto& e : t.edges) {
    const auto &a = t.nodes[e.parent], &b = t.nodes[e.child];
    o << a.name << "\t" << b.name << "\t" << CountText(t, e.count) << "\t" << frac(e.count, t.total) << "\t"
      << frac(e.count, a.count) << "\t" << FindMuts(a.aa, b.aa) << "\n";
  }
}

void WriteLineageSummary(std::ostream& o, const LineageTables& t, int64_t collisions, const LineageWeightSummary* ws) {
  o << "key\tvalue\nrows\t" << t.num_trees << "\ndistinct_nt\t" << t.distinct_nt << "\ndistinct_aa\t" << t.distinct_aa
    << "\nlongest_path\t" << t.longest_path << "\nhash_collisions_resolved\t" << collisions << "\n";
  if (ws)
    o << "rows_used\t" << ws->rows_used << "\nrows_skipped_nonfinite\t" << ws->rows_skipped_nonfinite << "\ndraws_per_row\t"
      << ws->draws_per_row << "\nkish_ess\t" << Fmt17(ws->kish_ess) << "\n";
}

std::vector<double> LineageWeights(const std::vector<double>& lw, LineageWeightSummary* ws) {
  double top = -INFINITY;
  for (double x : lw)
    if (std::isfinite(x)) top = std::max(top, x);
  if (!std::isfinite(top)) throw std::runtime_error("lineage: no row with a finite weight");
  std::vector<double> w(lw.size(), 0.0);
  double s1 = 0, s2 = 0;
  ws->rows_used = ws->rows_skipped_nonfinite = 0;
  for (std::size_t i = 0; i < lw.size(); ++i) {
    if (!std::isfinite(lw[i])) {
      ++ws->rows_skipped_nonfinite;
      continue;
    }
    w[i] = std::exp(lw[i] - top);
    ++ws->rows_used;
    s1 += w[i];
    s2 += w[i] * w[i];
  }
  ws->kish_ess = s1 * s1 / s2;
  return w;
}

void WriteLineageFiles(const std::string& prefix, const LineageTables& t, int64_t collisions, const LineageWeightSummary* ws) {
  std::ofstream fasta(prefix + ".fasta"), dnamap(prefix + ".dnamap"), nodes(prefix + ".nodes.tsv"),
      edges(prefix + ".edges.tsv"), summary(prefix + ".summary.tsv");
  if (!fasta || !dnamap || !nodes || !edges || !summary) throw std::runtime_error("Can't write " + prefix + ".*");
  WriteLineageFasta(fasta, t);
  WriteLineageDnaMap(dnamap, t);
  WriteLineageNodes(nodes, t);
  WriteLineageEdges(edges, t);
  WriteLineageSummary(summary, t, collisions, ws);
}

std::vector<int32_t> SeedPath(const int32_t* children, int T, int root, int seed_tip) {
  std::vector<int32_t> chain;
  if (T < 3 || seed_tip < 1 || seed_tip >= T) return chain;
  std::vector<int> parent(2 * (std::size_t)T - 2, -1);
  for (int v = T; v < 2 * T - 2; ++v)
    for (int c = 0; c < 2; ++c) {
      const int k = children[2 * (std::size_t)(v - T) + c];
      if (k >= 0 && k < 2 * T - 2) parent[k] = v;
    }
  for (int v = parent[seed_tip]; v >= T; v = parent[v]) {
    chain.push_back(v);
    if (v == root || (int)chain.size() > T) break;
  }
  if (chain.empty() || chain.back() != root) chain.clear();
  return chain;
}

CladeSlotResult CladeSlot(const int32_t* children, int T, int root, int seed_tip, const std::vector<int32_t>& with_tips) {
  const std::string who = "CladeSlot: ";
  if (with_tips.empty()) throw std::invalid_argument(who + "no tip to join the seed with (empty list)");
  std::vector<char> listed(std::max(T, 1), 0);
  for (const int32_t t : with_tips) {
    if (t == 0) throw std::invalid_argument(who + "tip 0 is naive: the node it shares with the seed is the MRCA (node 'mrca')");
    if (t < 1 || t >= T)
      throw std::invalid_argument(who + "tip " + std::to_string(t) + " is not one of the tips 1 .. " + std::to_string(T - 1));
    if (t == seed_tip) throw std::invalid_argument(who + "tip " + std::to_string(t) + " is the seed itself");
    if (listed[t]) throw std::invalid_argument(who + "tip " + std::to_string(t) + " is listed twice");
    listed[t] = 1;
  }
  CladeSlotResult r;
  r.path = SeedPath(children, T, root, seed_tip);
  if (r.path.empty())
    throw std::invalid_argument(who + "seed tip " + std::to_string(seed_tip) + " is not a tip 1 .. " + std::to_string(T - 1) +
                                " that hangs below the root");
  std::vector<int> slot_of(2 * (std::size_t)T - 2, -1);
  for (std::size_t s = 0; s < r.path.size(); ++s) slot_of[r.path[s]] = (int)s;
  r.slot = 0;
  for (const int32_t t : with_tips) {
    // the slot at which the tip's own path joins the seed's
    const std::vector<int32_t> own = SeedPath(children, T, root, t);
    int join = -1;
    for (const int32_t v : own)
      if (slot_of[v] >= 0) {
        join = slot_of[v];
        break;
      }
    if (join < 0) throw std::invalid_argument(who + "tip " + std::to_string(t) + " does not hang below the root");
    r.slot = std::max(r.slot, join);
  }
  return r;
}

std::vector<std::string> LineageOfAnnotatedTree(const std::string& s, const std::string& seed_seq) {
  struct Node {
    int parent = -1;
    std::string label, ancestral;
    bool annotated = false, tip = true;
  };
  std::vector<Node> nodes;
  std::vector<int> open;  // the nodes whose '(' is open
  int last = -1;          // the node the next label / comment / length belongs to
  const std::string key = "&ancestral=\"";
  auto fresh = [&] {
    Node n;
    n.parent = open.empty() ? -1 : open.back();
    nodes.push_back(n);
    return (int)nodes.size() - 1;
  };
  std::size_t k = 0;
  bool done = false;
  while (k < s.size() && !done) {
    const char c = s[k];
    if (c == '(') {
      const int v = fresh();
      nodes[v].tip = false;
      open.push_back(v);
      last = -1;
      ++k;
    } else if (c == ',') {
      if (last < 0) fresh();  // an empty subtree
      last = -1;
      ++k;
    } else if (c == ')') {
      if (open.empty()) throw std::runtime_error("lineage: unbalanced ')' in tree");
      if (last < 0) fresh();
      last = open.back();
      open.pop_back();
      ++k;
    } else if (c == ';') {
      done = true;
    } else if (c == '[') {
      const std::size_t e = s.find(']', k);
      if (e == std::string::npos) throw std::runtime_error("lineage: unterminated comment in tree");
      if (last < 0) last = fresh();
      const std::size_t a = s.find(key, k);
      if (a != std::string::npos && a < e) {
        const std::size_t q = s.find('"', a + key.size());
        if (q == std::string::npos || q > e) throw std::runtime_error("lineage: malformed ancestral annotation");
        nodes[last].ancestral = s.substr(a + key.size(), q - a - key.size());
        nodes[last].annotated = true;
      }
      k = e + 1;
    } else if (c == ':') {
      if (last < 0) last = fresh();
      ++k;
      while (k < s.size() && std::string("(),;[").find(s[k]) == std::string::npos) ++k;
    } else if (c == ' ' || c == '\t' || c == '\r') {
      ++k;
    } else {
      if (last < 0) last = fresh();
      const std::size_t b = k;
      while (k < s.size() && std::string("(),;[:").find(s[k]) == std::string::npos) ++k;
      nodes[last].label += s.substr(b, k - b);
    }
  }
  if (!open.empty()) throw std::runtime_error("lineage: unbalanced '(' in tree");
  auto find_tip = [&](const std::string& name) {
    for (std::size_t v = 0; v < nodes.size(); ++v)
      if (nodes[v].tip && nodes[v].label == name) return (int)v;
    return -1;
  };
  const int seed = find_tip(seed_seq), naive = find_tip("naive");
  if (seed < 0) throw std::runtime_error("seed node with label '" + seed_seq + "' not found in tree");
  if (naive < 0) throw std::runtime_error("no tip 'naive' in tree");
  std::vector<std::string> l;
  auto take = [&](int v) {
    if (!nodes[v].annotated) throw std::runtime_error("lineage: a node above '" + seed_seq + "' has no ancestral annotation");
    l.push_back(nodes[v].ancestral);
  };
  for (int v = seed; v >= 0; v = nodes[v].parent) take(v);
  take(naive);
  std::reverse(l.begin(), l.end());
  return l;
}

void TabulateLineageTrees(const std::string& trees_path, const std::string& seed_seq, const std::string& prefix,
                          const std::string& weights_path) {
  if (seed_seq == "naive") throw std::runtime_error("the seed sequence cannot be 'naive': the lineage ends there");
  std::ifstream in(trees_path);
  if (!in) throw std::runtime_error("Can't open trees file " + trees_path);
  std::string line;
  // the weights first: a tree's weight needs the largest log-weight
  const bool weighted = !weights_path.empty();
  std::vector<double> lw, w;
  LineageWeightSummary ws;
  if (weighted) {
    std::ifstream win(weights_path);
    if (!win) throw std::runtime_error("Can't open weights file " + weights_path);
    while (std::getline(win, line)) {
      const std::size_t a = line.find_first_not_of(" \t\r");
      if (a == std::string::npos) continue;
      const char* b = line.c_str() + a;
      char* end = nullptr;
      const double v = std::strtod(b, &end);
      if (end == b || std::string(end).find_first_not_of(" \t\r") != std::string::npos)
        throw std::runtime_error(weights_path + " line " + std::to_string(lw.size() + 1) + ": not a number: " + line);
      lw.push_back(v);
    }
  }
  LineageTabulator tab;
  if (weighted) tab.SetWeighted();
  std::size_t n_line = 0, n_trees = 0;
  bool have_weights = false;
  while (std::getline(in, line)) {
    ++n_line;
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const std::size_t k = n_trees++;
    if (weighted && k >= lw.size()) continue;  // (counted on: the error below names both counts)
    if (weighted && !have_weights) {
      w = LineageWeights(lw, &ws);
      have_weights = true;
    }
    if (weighted && !std::isfinite(lw[k])) continue;  // skipped and counted
    std::vector<std::string> l;
    try {
      l = LineageOfAnnotatedTree(line, seed_seq);
    } catch (const std::exception& e) {
      throw std::runtime_error(trees_path + " line " + std::to_string(n_line) + ": " + e.what());
    }
    // naive, the root RunAsr adds on the naive branch, naive's neighbour .. seed's parent, seed
    tab.AddTree(l, std::max(0, (int)l.size() - 3), weighted ? w[k] : 1.0);
  }
  if (weighted && lw.size() != n_trees)
    throw std::runtime_error("the weights file " + weights_path + " has " + std::to_string(lw.size()) + " lines, the trees file " +
                             trees_path + " has " + std::to_string(n_trees) + " trees");
  WriteLineageFiles(prefix, tab.Finish(seed_seq), 0, weighted ? &ws : nullptr);
}

}  // namespace linearham
