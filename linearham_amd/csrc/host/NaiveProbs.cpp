#include "NaiveProbs.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <stdexcept>
#include <unordered_map>

namespace linearham {

namespace {

// the standard code over T, C, A, G (first base slowest)
const char kCode[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

int CodeIndex(char b) {
  switch (b) {
    case 'T': return 0;
    case 'C': return 1;
    case 'A': return 2;
    case 'G': return 3;
    default: return -1;
  }
}

char TranslateCodon(const char* c) {
  char aa = 0;
  for (int x = 0; x < 4; ++x)
    for (int y = 0; y < 4; ++y)
      for (int z = 0; z < 4; ++z) {
        const int i = CodeIndex(c[0]), j = CodeIndex(c[1]), k = CodeIndex(c[2]);
        if ((i >= 0 && x != i) || (j >= 0 && y != j) || (k >= 0 && z != k)) continue;
        if (c[0] != 'N' && i < 0) return 'X';
        if (c[1] != 'N' && j < 0) return 'X';
        if (c[2] != 'N' && k < 0) return 'X';
        const char a = kCode[x * 16 + y * 4 + z];
        if (aa && a != aa) return 'X';
        aa = a;
      }
  return aa ? aa : 'X';
}

}  // namespace

std::string TranslateDna(const std::string& dna) {
  // TranslateCodon of every codon over ACGTN, tabulated once (a character outside the alphabet gives X)
  static const std::array<char, 125> table = [] {
    std::array<char, 125> t{};
    const char* alphabet = "ACGTN";
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b)
        for (int c = 0; c < 5; ++c) {
          const char codon[3] = {alphabet[a], alphabet[b], alphabet[c]};
          t[a * 25 + b * 5 + c] = TranslateCodon(codon);
        }
    return t;
  }();
  auto index = [](char b) {
    switch (b) {
      case 'A': return 0;
      case 'C': return 1;
      case 'G': return 2;
      case 'T': return 3;
      case 'N': return 4;
      default: return -1;
    }
  };
  std::string aa;
  aa.reserve(dna.size() / 3);
  for (std::size_t i = 0; i + 3 <= dna.size(); i += 3) {
    const int a = index(dna[i]), b = index(dna[i + 1]), c = index(dna[i + 2]);
    aa.push_back(a < 0 || b < 0 || c < 0 ? 'X' : table[a * 25 + b * 5 + c]);
  }
  return aa;
}

std::string ReprDouble(double v) {
  if (std::isnan(v)) return "nan";
  if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
  if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
  const bool neg = v < 0;
  const double a = std::fabs(v);
  std::string digits;
  int decpt = 0;  // a = 0.<digits> x 10^decpt
  char buf[64];
  for (int p = 1; p <= 17 && digits.empty(); ++p) {
    std::snprintf(buf, sizeof buf, "%.*e", p - 1, a);
    const char* e = std::strchr(buf, 'e');
    std::string m;
    for (const char* q = buf; q < e; ++q)
      if (*q != '.') m.push_back(*q);
    const int ex = std::atoi(e + 1);
    // the correctly rounded p digits and their two neighbours: the closest one that reads back to `a`
    const unsigned long long M = std::strtoull(m.c_str(), nullptr, 10);
    long double best_err = -1;
    for (long long d = -1; d <= 1; ++d) {
      const unsigned long long c = M + d;
      if (c == 0) continue;
      std::snprintf(buf, sizeof buf, "%llue%d", c, ex - (p - 1));
      if (std::strtod(buf, nullptr) != a) continue;
      const long double err = std::fabs(std::strtold(buf, nullptr) - (long double)a);
      if (best_err >= 0 && err >= best_err) continue;
      best_err = err;
      std::string s = std::to_string(c);
      decpt = ex + 1 + (int)s.size() - p;  // (999 + 1 carries into one more digit)
      while (s.size() > 1 && s.back() == '0') s.pop_back();
      digits = s;
    }
  }
  std::string out = neg ? "-" : "";
  const int nd = (int)digits.size();
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0)
      out += "0." + std::string(-decpt, '0') + digits;
    else if (decpt >= nd)
      out += digits + std::string(decpt - nd, '0') + ".0";
    else
      out += digits.substr(0, decpt) + "." + digits.substr(decpt);
  } else {
    out += digits.substr(0, 1);
    if (nd > 1) out += "." + digits.substr(1);
    const int e = decpt - 1;
    std::snprintf(buf, sizeof buf, "e%c%02d", e < 0 ? '-' : '+', std::abs(e));
    out += buf;
  }
  return out;
}

namespace {

// names: the candidates' names too (ReadNamedCandidateFile), or null
std::vector<std::string> ReadCandidates(const std::string& path, int n_sites, std::vector<std::string>* names) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("Can't read candidate file " + path);
  std::vector<std::string> seqs;
  std::vector<int> line_of;
  std::string line, cur, cur_name;
  int ln = 0, cur_line = 0, header_line = 0;
  bool fasta = false;
  auto refuse_empty_record = [&] {
    if (header_line && cur.empty())
      throw std::runtime_error(path + ", line " + std::to_string(header_line) + ": FASTA header without a sequence");
  };
  auto flush = [&] {
    if (cur.empty()) return;
    seqs.push_back(cur);
    line_of.push_back(cur_line);
    if (names) names->push_back(cur_name.empty() ? "candidate_" + std::to_string(seqs.size()) : cur_name);
    cur.clear();
    cur_name.clear();
  };
  while (std::getline(in, line)) {
    ++ln;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    if (line[0] == '>') {
      refuse_empty_record();
      fasta = true;
      flush();
      header_line = ln;
      cur_name = line.substr(1, std::min(line.find_first_of(" \t", 1), line.size()) - 1);
      continue;
    }
    for (char& ch : line) {
      if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 'a' + 'A');
      if (!std::strchr("ACGTN", ch) || ch == 0)
        throw std::runtime_error(path + ", line " + std::to_string(ln) + ": character '" + std::string(1, ch) +
                                 "' is not one of ACGTN");
    }
    if (fasta) {
      if (cur.empty()) cur_line = ln;
      cur += line;
    } else {
      cur_line = ln;
      cur = line;
      flush();
    }
  }
  refuse_empty_record();
  flush();
  if (seqs.empty()) throw std::runtime_error(path + ": no candidate sequences");
  if (seqs.size() > 65536) throw std::runtime_error(path + ": more than 65536 candidates");
  std::unordered_map<std::string, int> seen;
  for (std::size_t k = 0; k < seqs.size(); ++k) {
    if ((int)seqs[k].size() != n_sites)
      throw std::runtime_error(path + ", line " + std::to_string(line_of[k]) + ": sequence of " +
                               std::to_string(seqs[k].size()) + " sites, the alignment has " + std::to_string(n_sites));
    const auto r = seen.emplace(seqs[k], line_of[k]);
    if (!r.second)
      throw std::runtime_error(path + ", line " + std::to_string(line_of[k]) + ": repeats the sequence of line " +
                               std::to_string(r.first->second));
  }
  return seqs;
}

std::vector<std::size_t> RankByProbability(const std::vector<double>& prob) {
  std::vector<std::size_t> idx(prob.size());
  for (std::size_t k = 0; k < idx.size(); ++k) idx[k] = k;
  std::stable_sort(idx.begin(), idx.end(), [&](std::size_t a, std::size_t b) { return prob[a] > prob[b]; });
  return idx;
}

}  // namespace

std::vector<std::string> ReadCandidateFile(const std::string& path, int n_sites) { return ReadCandidates(path, n_sites, nullptr); }

NamedCandidates ReadNamedCandidateFile(const std::string& path, int n_sites) {
  NamedCandidates c;
  c.seqs = ReadCandidates(path, n_sites, &c.names);
  return c;
}

std::vector<std::size_t> RankCandidates(const NaiveProbsTable& t) { return RankByProbability(t.prob); }

void WriteAncestralProbsTable(std::ostream& o, const AncestralProbsTable& t) {
  char buf[64];
  o << "name\tsequence\tprobability\n";
  for (std::size_t k : RankByProbability(t.prob)) {
    std::snprintf(buf, sizeof buf, "%.17g", t.prob[k]);
    o << t.names[k] << '\t' << t.seqs[k] << '\t' << buf << '\n';
  }
}

double CoveredMass(const AncestralProbsTable& t) {
  double mass = 0.0;
  for (std::size_t k = 0; k < t.seqs.size(); ++k)
    if (t.seqs[k].find('N') == std::string::npos) mass += t.prob[k];
  return mass;
}

int ParseLineageNode(const std::string& name) { return ParseLineageNodeText(name).node; }

LineageNode ParseLineageNodeText(const std::string& text) {
  static const std::string kWith = "mrca-with:";
  LineageNode n;
  n.text = text;
  if (text == "parent") return n;
  n.node = 1;
  if (text == "mrca") return n;
  n.node = 2;
  bool ok = text.compare(0, kWith.size(), kWith) == 0;
  for (std::size_t a = kWith.size(); ok;) {
    const std::size_t b = std::min(text.find(',', a), text.size());
    n.with.push_back(text.substr(a, b - a));
    ok = !n.with.back().empty() && std::count(n.with.begin(), n.with.end(), n.with.back()) == 1;
    if (b == text.size()) break;
    a = b + 1;
  }
  if (!ok)
    throw std::runtime_error("--node must be 'parent' (the seed's parent), 'mrca' or 'mrca-with:<name>[,<name>...]' (the most "
                             "recent common ancestor of the seed and the named sequences, each named once), not '" + text + "'");
  return n;
}

void WriteNaiveTable(std::ostream& o, const NaiveProbsTable& t, bool with_sampled) {
  char buf[64];
  auto num = [&](double v) {
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return std::string(buf);
  };
  o << "rank\tNaiveSequence\tprobability\tlog_prior" << (with_sampled ? "\tsampled_count\tsampled_frequency" : "") << "\n";
  const std::vector<std::size_t> idx = RankCandidates(t);
  for (std::size_t r = 0; r < idx.size(); ++r) {
    const std::size_t k = idx[r];
    o << (r + 1) << '\t' << t.seqs[k] << '\t' << num(t.prob[k]) << '\t' << num(t.log_prior[k]);
    if (with_sampled) {
      if (t.sampled)
        o << '\t' << t.count[k] << '\t' << num(t.freq[k]);
      else
        o << "\tNA\tNA";
    }
    o << '\n';
  }
}

namespace {

struct AaGroup {
  std::string aa;
  double p = 0.0;
  std::vector<std::size_t> members;  // candidate order
};

std::vector<AaGroup> GroupByTranslation(const NaiveProbsTable& t) {
  std::vector<AaGroup> g;
  std::unordered_map<std::string, std::size_t> at;
  for (std::size_t k = 0; k < t.seqs.size(); ++k) {
    const std::string aa = TranslateDna(t.seqs[k]);
    const auto r = at.emplace(aa, g.size());
    if (r.second) g.push_back(AaGroup{aa, 0.0, {}});
    AaGroup& x = g[r.first->second];
    x.p += t.prob[k];
    x.members.push_back(k);
  }
  std::stable_sort(g.begin(), g.end(), [](const AaGroup& a, const AaGroup& b) { return a.p > b.p; });
  for (AaGroup& x : g)
    std::stable_sort(x.members.begin(), x.members.end(),
                     [&](std::size_t a, std::size_t b) { return t.prob[a] > t.prob[b]; });
  return g;
}

}  // namespace

void WriteAaFasta(std::ostream& o, const NaiveProbsTable& t) {
  const std::vector<AaGroup> g = GroupByTranslation(t);
  for (std::size_t i = 0; i < g.size(); ++i) o << ">naive_" << i << "_" << ReprDouble(g[i].p) << "\n" << g[i].aa << "\n";
}

void WriteDnaMap(std::ostream& o, const NaiveProbsTable& t) {
  const std::vector<AaGroup> g = GroupByTranslation(t);
  for (std::size_t i = 0; i < g.size(); ++i) {
    o << ">naive_" << i << "_" << ReprDouble(g[i].p) << "\n";
    for (std::size_t k : g[i].members) o << ReprDouble(t.prob[k]) << "," << t.seqs[k] << "\n";
  }
}

}  // namespace linearham
