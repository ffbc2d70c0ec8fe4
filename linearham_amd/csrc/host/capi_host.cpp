// Test/bench-facing C entry points of liblinearham_host.so: construct the C++ host classes and dump
// their accessors as JSON so that the pytest suite can compare them with the reference's goldens
// (test/test.cpp) -- the role the Catch binary plays upstream.
#include <chrono>
#include <cmath>
#include <unordered_map>
#include <cstring>
#include <iomanip>
#include <sstream>
#include <random>
#include <string>

#include "Lineage.hpp"
#include "NaiveProbs.hpp"
#include "PhyloHMM.hpp"
#include "SimpleHMM.hpp"

using namespace linearham;

namespace {

thread_local std::string g_err, g_out;

struct Json {
  std::ostringstream o;
  bool first = true;
  Json() { o << std::setprecision(17); }
  void key(const std::string& k) {
    o << (first ? "{" : ",") << "\"" << k << "\":";
    first = false;
  }
  static std::string esc(const std::string& s) {
    std::string r = "\"";
    for (char c : s) {
      if (c == '"' || c == '\\') r.push_back('\\');
      r.push_back(c);
    }
    return r + "\"";
  }
  void num(double v) {
    if (std::isnan(v)) o << "NaN";
    else if (std::isinf(v)) o << (v > 0 ? "Infinity" : "-Infinity");
    else o << v;
  }
  void put(const std::string& k, const std::string& v) { key(k); o << esc(v); }
  void put(const std::string& k, int v) { key(k); o << v; }
  void put(const std::string& k, bool v) { key(k); o << (v ? "true" : "false"); }
  void put(const std::string& k, double v) { key(k); num(v); }
  void put(const std::string& k, const std::vector<int>& v) {
    key(k); o << "[";
    for (std::size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << v[i];
    o << "]";
  }
  void put(const std::string& k, const std::vector<double>& v) {
    key(k); o << "[";
    for (std::size_t i = 0; i < v.size(); ++i) { if (i) o << ","; num(v[i]); }
    o << "]";
  }
  void put(const std::string& k, const std::vector<std::string>& v) {
    key(k); o << "[";
    for (std::size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << esc(v[i]);
    o << "]";
  }
  void put(const std::string& k, const std::vector<GermlineType>& v) {
    key(k); o << "[";
    for (std::size_t i = 0; i < v.size(); ++i)
      o << (i ? "," : "") << (v[i] == GermlineType::V ? "\"V\"" : v[i] == GermlineType::D ? "\"D\"" : "\"J\"");
    o << "]";
  }
  template <typename T>
  void put(const std::string& k, const Matrix<T>& m) {
    key(k); o << "[";
    for (int r = 0; r < m.rows(); ++r) {
      o << (r ? ",[" : "[");
      for (int c = 0; c < m.cols(); ++c) { if (c) o << ","; num((double)m(r, c)); }
      o << "]";
    }
    o << "]";
  }
  void put(const std::string& k, const GeneRanges& g) {
    key(k); o << "{";
    bool f = true;
    for (const auto& kv : g) {
      o << (f ? "" : ",") << esc(kv.first) << ":[" << kv.second.first << "," << kv.second.second << "]";
      f = false;
    }
    o << "}";
  }
  void put(const std::string& k, const std::map<std::string, int>& g) {
    key(k); o << "{";
    bool f = true;
    for (const auto& kv : g) { o << (f ? "" : ",") << esc(kv.first) << ":" << kv.second; f = false; }
    o << "}";
  }
  std::string str() { return first ? "{}" : o.str() + "}"; }
};

void DumpHMM(const HMM& h, Json& j) {
  j.put("locus", h.locus());
  j.put("flexbounds", GeneRanges(h.flexbounds().begin(), h.flexbounds().end()));
  j.put("relpos", h.relpos());
  j.put("alphabet", h.alphabet());
  j.put("msa", h.msa());
#define DUMP(name) j.put(#name, h.name());
  DUMP(vpadding_ggene_ranges) DUMP(vpadding_naive_bases) DUMP(vpadding_site_inds)
  DUMP(vgerm_state_strs) DUMP(vgerm_left_del) DUMP(vgerm_right_del) DUMP(vgerm_ggene_ranges)
  DUMP(vgerm_naive_bases) DUMP(vgerm_germ_inds) DUMP(vgerm_site_inds)
  DUMP(vd_junction_state_strs) DUMP(vd_junction_del) DUMP(vd_junction_ggene_types)
  DUMP(vd_junction_ggene_ranges) DUMP(vd_junction_naive_bases) DUMP(vd_junction_germ_inds)
  DUMP(vd_junction_site_inds)
  DUMP(dgerm_state_strs) DUMP(dgerm_left_del) DUMP(dgerm_right_del) DUMP(dgerm_ggene_ranges)
  DUMP(dgerm_naive_bases) DUMP(dgerm_germ_inds) DUMP(dgerm_site_inds)
  DUMP(dj_junction_state_strs) DUMP(dj_junction_del) DUMP(dj_junction_ggene_types)
  DUMP(dj_junction_ggene_ranges) DUMP(dj_junction_naive_bases) DUMP(dj_junction_germ_inds)
  DUMP(dj_junction_site_inds)
  DUMP(jgerm_state_strs) DUMP(jgerm_left_del) DUMP(jgerm_right_del) DUMP(jgerm_ggene_ranges)
  DUMP(jgerm_naive_bases) DUMP(jgerm_germ_inds) DUMP(jgerm_site_inds)
  DUMP(jpadding_ggene_ranges) DUMP(jpadding_naive_bases) DUMP(jpadding_site_inds)
  DUMP(vpadding_transition) DUMP(vgerm_vd_junction_transition) DUMP(vd_junction_transition)
  DUMP(vd_junction_dgerm_transition) DUMP(dgerm_dj_junction_transition) DUMP(dj_junction_transition)
  DUMP(dj_junction_jgerm_transition) DUMP(jpadding_transition) DUMP(cache_forward)
}

void DumpForward(const HMM& h, Json& j) {
  DUMP(vgerm_forward) DUMP(vd_junction_forward) DUMP(dgerm_forward) DUMP(dj_junction_forward) DUMP(jgerm_forward)
  DUMP(vgerm_scaler_count) DUMP(vd_junction_scaler_counts) DUMP(dgerm_scaler_count)
  DUMP(dj_junction_scaler_counts) DUMP(jgerm_scaler_count)
}

void DumpSample(const HMM& h, Json& j) {
  DUMP(naive_seq_samp) DUMP(vgerm_state_str_samp) DUMP(vgerm_state_ind_samp) DUMP(vgerm_left_del_samp)
  DUMP(vgerm_right_del_samp) DUMP(vgerm_left_insertion_samp) DUMP(vd_junction_state_str_samps)
  DUMP(vd_junction_state_ind_samps) DUMP(vd_junction_insertion_samp) DUMP(dgerm_state_str_samp)
  DUMP(dgerm_state_ind_samp) DUMP(dgerm_left_del_samp) DUMP(dgerm_right_del_samp)
  DUMP(dj_junction_state_str_samps) DUMP(dj_junction_state_ind_samps) DUMP(dj_junction_insertion_samp)
  DUMP(jgerm_state_str_samp) DUMP(jgerm_state_ind_samp) DUMP(jgerm_left_del_samp) DUMP(jgerm_right_del_samp)
  DUMP(jgerm_right_insertion_samp)
}

void DumpPhylo(const PhyloHMM& h, Json& j) {
  DUMP(xmsa) DUMP(xmsa_labels) DUMP(xmsa_seqs) DUMP(xmsa_naive_ind) DUMP(vpadding_xmsa_inds) DUMP(vgerm_xmsa_inds)
  DUMP(vd_junction_xmsa_inds) DUMP(dgerm_xmsa_inds) DUMP(dj_junction_xmsa_inds) DUMP(jgerm_xmsa_inds)
  DUMP(jpadding_xmsa_inds)
}
#undef DUMP

template <typename F>
int Guard(F f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}

}  // namespace

extern "C" {

const char* lhh_last_error() { return g_err.c_str(); }

// Germline parameter parsing only (no GPU): JSON of one allele file parsed as V, D or J.
int lhh_germline_json(const char* yaml_path, char type, const char** out) {
  return Guard([&] {
    const yaml_lite::Node root = yaml_lite::LoadFile(yaml_path);
    Json j;
    const Germline g(root);
    j.put("landing_in", g.landing_in());
    j.put("landing_out", g.landing_out());
    j.put("transition", g.transition());
    j.put("gene_prob", g.gene_prob());
    j.put("alphabet", g.alphabet());
    j.put("name", g.name());
    j.put("emission", g.emission());
    j.put("bases", g.bases());
    j.put("length", g.length());
    if (type == 'D' || type == 'J') {
      const NTInsertion n(root);
      j.put("nti_landing_in", n.nti_landing_in());
      j.put("nti_landing_out", n.nti_landing_out());
      j.put("nti_transition", n.nti_transition());
      j.put("nti_emission", n.nti_emission());
    }
    if (type == 'V' || type == 'J') {
      const NPadding p(root);
      j.put("n_transition", p.n_transition());
      j.put("n_emission", p.n_emission());
    }
    g_out = j.str();
    *out = g_out.c_str();
  });
}

int lhh_simple_create(const char* yaml, int cluster_ind, const char* dir, int seed, void** out) {
  return Guard([&] { *out = new SimpleHMM(yaml, cluster_ind, dir, seed); });
}
int lhh_phylo_create(const char* yaml, int cluster_ind, const char* dir, int seed, void** out) {
  return Guard([&] { *out = static_cast<HMM*>(new PhyloHMM(yaml, cluster_ind, dir, seed)); });
}
void lhh_destroy(void* h) { delete static_cast<HMM*>(h); }

int lhh_phylo_init_parameters(void* h, const char* newick_path, const double* er, const double* pi, double alpha,
                              int num_rates) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h))
        .InitializePhyloParameters(newick_path, std::vector<double>(er, er + 6), std::vector<double>(pi, pi + 4),
                                   alpha, num_rates);
  });
}
int lhh_phylo_init_parameters_str(void* h, const char* newick, const double* er, const double* pi, double alpha,
                                  int num_rates) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h))
        .InitializePhyloParametersFromString(newick, std::vector<double>(er, er + 6),
                                             std::vector<double>(pi, pi + 4), alpha, num_rates);
  });
}
int lhh_phylo_init_emission(void* h) {
  return Guard([&] { dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).InitializePhyloEmission(); });
}
int lhh_phylo_set_extended_range(void* h, int on) {
  return Guard([&] { dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).SetExtendedRange(on != 0); });
}
int lhh_loglikelihood(void* h, double* out) {
  return Guard([&] { *out = static_cast<HMM*>(h)->LogLikelihood(); });
}
int lhh_sample(void* h, const char** out) {
  return Guard([&] {
    g_out = static_cast<HMM*>(h)->SampleNaiveSequence();
    *out = g_out.c_str();
  });
}
// Test entry (PhyloHMM::SampleStatesWithWords): device_states / host_states [n_states]; returns the count in *n_states.
int lhh_phylo_sample_words(void* h, const uint32_t* words, int n_words, int32_t* device_states, int32_t* host_states,
                           int cap, int* n_states) {
  return Guard([&] {
    std::vector<int32_t> d, s;
    static_cast<linearham::PhyloHMM*>(h)->SampleStatesWithWords(words, n_words, d, s);
    if ((int)d.size() > cap || d.size() != s.size()) throw std::runtime_error("lhh_phylo_sample_words: state count");
    std::copy(d.begin(), d.end(), device_states);
    std::copy(s.begin(), s.end(), host_states);
    *n_states = (int)d.size();
  });
}

// PhyloHMM::NaivePosterior: post [cap >= lh_forward_size]; *n receives the count, *loglik the log-likelihood.
// post == NULL: only *n (the family's lh_forward_size), nothing is evaluated.
int lhh_phylo_posterior(void* h, double* post, int cap, int* n, double* loglik) {
  return Guard([&] {
    if (!post) {
      *n = (int)lh_forward_size(dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).family());
      return;
    }
    const std::vector<double> p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).NaivePosterior(loglik);
    if ((int)p.size() > cap) throw std::runtime_error("lhh_phylo_posterior: output too small");
    std::copy(p.begin(), p.end(), post);
    *n = (int)p.size();
  });
}

// PhyloHMM::NaiveMarginals through the C++ mapping: site_base [L][5]; the gene table as lines "R\tgene\tp" in *genes.
int lhh_phylo_naive_marginals(void* h, double* site_base, int cap_sites, const char** genes) {
  return Guard([&] {
    const PhyloHMM::NaiveMarginalsResult m = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).NaiveMarginals();
    if ((int)m.site_base.size() > cap_sites) throw std::runtime_error("lhh_phylo_naive_marginals: output too small");
    for (std::size_t s = 0; s < m.site_base.size(); ++s)
      for (int b = 0; b < 5; ++b) site_base[s * 5 + b] = m.site_base[s][b];
    std::ostringstream o;
    PhyloHMM::WriteGeneTable(o, m);
    g_out = o.str();
    *genes = g_out.c_str();
  });
}

int lhh_run_marginals_pipeline(void* h, const char* input_path, const char* output_prefix, int num_rates,
                               double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunMarginalsPipeline(input_path, output_prefix, num_rates, burnin_frac);
  });
}

// linearham::SeedPath (no family, no device): path [cap >= n_tips - 2]; *n receives the length, 0 if the tip does not hang
// below the root.
int lhh_seed_path(const int32_t* children, int n_tips, int root, int seed_tip, int32_t* path, int cap, int* n) {
  return Guard([&] {
    const std::vector<int32_t> c = linearham::SeedPath(children, n_tips, root, seed_tip);
    if ((int)c.size() > cap) throw std::runtime_error("lhh_seed_path: output too small");
    std::copy(c.begin(), c.end(), path);
    *n = (int)c.size();
  });
}

// linearham::CladeSlot (no family, no device): with_tips [n_with]; path [cap >= n_tips - 2], *n its length, *slot the index
// on it of the most recent common ancestor of the seed and the listed tips.
int lhh_clade_slot(const int32_t* children, int n_tips, int root, int seed_tip, const int32_t* with_tips, int n_with,
                   int32_t* path, int cap, int* n, int* slot) {
  return Guard([&] {
    const linearham::CladeSlotResult r = linearham::CladeSlot(
        children, n_tips, root, seed_tip, std::vector<int32_t>(with_tips, with_tips + std::max(n_with, 0)));
    if ((int)r.path.size() > cap) throw std::runtime_error("lhh_clade_slot: output too small");
    std::copy(r.path.begin(), r.path.end(), path);
    *n = (int)r.path.size();
    *slot = r.slot;
  });
}

// PhyloHMM::AncestralMarginals: nodes [cap_slots], marg [cap_slots][L][4], rate_post [L][R]; *n_slots receives the chain's
// length, *num_rates R.  marg == NULL: only those two.
int lhh_phylo_ancestral_marginals(void* h, const char* seed_seq, int32_t* nodes, double* marg, double* rate_post,
                                  int cap_slots, int* n_slots, int* num_rates, double* loglik) {
  return Guard([&] {
    const PhyloHMM::AncestralMarginalsResult r = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).AncestralMarginals(seed_seq);
    *n_slots = (int)r.nodes.size();
    *num_rates = r.num_rates;
    if (!marg) return;
    if ((int)r.nodes.size() > cap_slots) throw std::runtime_error("lhh_phylo_ancestral_marginals: output too small");
    std::copy(r.nodes.begin(), r.nodes.end(), nodes);
    std::copy(r.marg.begin(), r.marg.end(), marg);
    if (rate_post) std::copy(r.rate_post.begin(), r.rate_post.end(), rate_post);
    if (loglik) *loglik = r.loglik;
  });
}

int lhh_run_ancestral_marginals_pipeline(void* h, const char* input_path, const char* seed_seq, const char* output_prefix,
                                         int num_rates, double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunAncestralMarginalsPipeline(input_path, seed_seq, output_prefix, num_rates,
                                                                               burnin_frac);
  });
}

// PhyloHMM::LineageSubstitutions: nodes [cap_slots], edge [cap_slots][L][16], naive_edge [L][20], chain_counts [L][16],
// edges [cap_slots + 1][4] (upper node, lower node, branch length, load); *n_slots receives the chain's length.
int lhh_phylo_lineage_substitutions(void* h, const char* seed_seq, int32_t* nodes, double* edge, double* naive_edge,
                                    double* chain_counts, double* edges, int cap_slots, int* n_slots, double* loglik) {
  return Guard([&] {
    const PhyloHMM::LineageSubstitutionsResult r = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).LineageSubstitutions(seed_seq);
    if ((int)r.nodes.size() > cap_slots) throw std::runtime_error("lhh_phylo_lineage_substitutions: output too small");
    *n_slots = (int)r.nodes.size();
    std::copy(r.nodes.begin(), r.nodes.end(), nodes);
    std::copy(r.edge.begin(), r.edge.end(), edge);
    std::copy(r.naive_edge.begin(), r.naive_edge.end(), naive_edge);
    std::copy(r.chain_counts.begin(), r.chain_counts.end(), chain_counts);
    for (std::size_t e = 0; e < r.edges.size(); ++e) {
      edges[e * 4] = r.edges[e].upper;
      edges[e * 4 + 1] = r.edges[e].lower;
      edges[e * 4 + 2] = r.edges[e].brlen;
      edges[e * 4 + 3] = r.edges[e].load;
    }
    if (loglik) *loglik = r.loglik;
  });
}

// PhyloHMM::WritePairTable's text of table [n_sites][n_rows][4]
int lhh_write_pair_table(const double* table, int n_sites, int n_rows, int with_sum, const char** out) {
  return Guard([&] {
    if (n_sites < 0 || n_rows < 1 || n_rows > 5) throw std::runtime_error("lhh_write_pair_table: bad shape");
    std::ostringstream o;
    PhyloHMM::WritePairTable(o, table, (std::size_t)n_sites, n_rows, with_sum != 0);
    g_out = o.str();
    *out = g_out.c_str();
  });
}

// PhyloHMM::AncestralCandidatePosterior: candidates = K sequences joined by '\n'; log_cand [K]
int lhh_phylo_ancestral_candidate_posterior(void* h, const char* seed_seq, int node, const char* candidates, int K,
                                            double* log_cand, int* node_id, double* loglik) {
  return Guard([&] {
    std::vector<std::string> seqs;
    std::istringstream in(candidates);
    for (std::string line; std::getline(in, line);) seqs.push_back(line);
    if ((int)seqs.size() != K) throw std::runtime_error("lhh_phylo_ancestral_candidate_posterior: K does not match the candidates");
    const PhyloHMM::AncestralCandidateResult r =
        dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).AncestralCandidatePosterior(seed_seq, node, seqs);
    std::copy(r.log_cand.begin(), r.log_cand.end(), log_cand);
    if (node_id) *node_id = r.node;
    if (loglik) *loglik = r.loglik;
  });
}

// The same with the node as --node's text (ParseLineageNodeText): 'parent', 'mrca' or 'mrca-with:<name>[,<name>...]'
int lhh_phylo_ancestral_candidate_posterior_at(void* h, const char* seed_seq, const char* node_text, const char* candidates,
                                               int K, double* log_cand, int* node_id, double* loglik) {
  return Guard([&] {
    std::vector<std::string> seqs;
    std::istringstream in(candidates);
    for (std::string line; std::getline(in, line);) seqs.push_back(line);
    if ((int)seqs.size() != K) throw std::runtime_error("lhh_phylo_ancestral_candidate_posterior_at: K does not match the candidates");
    const linearham::LineageNode n = linearham::ParseLineageNodeText(node_text);
    const PhyloHMM::AncestralCandidateResult r =
        dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).AncestralCandidatePosterior(seed_seq, n.node, seqs, n.with);
    std::copy(r.log_cand.begin(), r.log_cand.end(), log_cand);
    if (node_id) *node_id = r.node;
    if (loglik) *loglik = r.loglik;
  });
}

int lhh_run_ancestral_probs_pipeline_at(void* h, const char* input_path, const char* seed_seq, const char* node_text,
                                        const char* candidates_path, const char* output_prefix, int num_rates,
                                        double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunAncestralProbsPipeline(input_path, seed_seq, std::string(node_text),
                                                                           candidates_path, output_prefix, num_rates, burnin_frac);
  });
}

int lhh_run_ancestral_probs_pipeline(void* h, const char* input_path, const char* seed_seq, int node, const char* candidates_path,
                                     const char* output_prefix, int num_rates, double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunAncestralProbsPipeline(input_path, seed_seq, node, candidates_path,
                                                                           output_prefix, num_rates, burnin_frac);
  });
}

// The three tables of a NodeCodonsResult, separated by blank lines (WriteNodeCodonTable, WriteNodeAminoAcidTable,
// WriteChangeTable)
static const char* NodeCodonsText(const PhyloHMM::NodeCodonsResult& m) {
  std::ostringstream o;
  PhyloHMM::WriteNodeCodonTable(o, m);
  o << "\n";
  PhyloHMM::WriteNodeAminoAcidTable(o, m);
  o << "\n";
  PhyloHMM::WriteChangeTable(o, m);
  g_out = o.str();
  return g_out.c_str();
}

// PhyloHMM::NodeCodonMarginals: codons [cap_codons][64], change [cap_codons][4]; *n_codons receives the count, *text the
// three tables as the writers print them.  codons == NULL: only *n_codons (after the node and frame checks), nothing is
// evaluated.
// The body of both forms below, behind their check of the node: `with` empty: the node is `node`.
static void NodeCodonMarginalsOut(void* h, const char* seed_seq, int node, const std::vector<std::string>& with, int frame,
                                  double* codons, double* change, int cap_codons, int* n_codons, int* node_id, double* loglik,
                                  const char** text) {
  PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
  if (frame < 0 || frame > 2) throw std::runtime_error("NodeCodonMarginals: frame must be 0, 1 or 2");
  const int L = (int)p.msa().cols();
  *n_codons = L >= frame ? (L - frame) / 3 : 0;
  if (!codons) return;
  const PhyloHMM::NodeCodonsResult m = p.NodeCodonMarginals(seed_seq, node, frame, with);
  if ((int)m.codons.size() > cap_codons) throw std::runtime_error("lhh_phylo_node_codon_marginals: output too small");
  for (std::size_t c = 0; c < m.codons.size(); ++c) {
    std::copy(m.codons[c].begin(), m.codons[c].end(), codons + c * 64);
    if (change) std::copy(m.change[c].begin(), m.change[c].end(), change + c * 4);
  }
  if (node_id) *node_id = m.node;
  if (loglik) *loglik = m.loglik;
  if (text) *text = NodeCodonsText(m);
}

int lhh_phylo_node_codon_marginals(void* h, const char* seed_seq, int node, int frame, double* codons, double* change,
                                   int cap_codons, int* n_codons, int* node_id, double* loglik, const char** text) {
  return Guard([&] {
    if (node != 0 && node != 1) throw std::runtime_error("NodeCodonMarginals: node must be 0 (the seed's parent) or 1 (the MRCA)");
    NodeCodonMarginalsOut(h, seed_seq, node, {}, frame, codons, change, cap_codons, n_codons, node_id, loglik, text);
  });
}

// The same with the node as --node's text; codons as lhh_phylo_node_codon_marginals takes them (NULL: only *n_codons,
// after the node text and the frame have been checked)
int lhh_phylo_node_codon_marginals_at(void* h, const char* seed_seq, const char* node_text, int frame, double* codons,
                                      double* change, int cap_codons, int* n_codons, int* node_id, double* loglik,
                                      const char** text) {
  return Guard([&] {
    const linearham::LineageNode n = linearham::ParseLineageNodeText(node_text);
    NodeCodonMarginalsOut(h, seed_seq, n.node, n.with, frame, codons, change, cap_codons, n_codons, node_id, loglik, text);
  });
}

int lhh_run_node_codons_pipeline_at(void* h, const char* input_path, const char* seed_seq, const char* node_text,
                                    const char* output_prefix, int num_rates, double burnin_frac, int frame) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunNodeCodonsPipeline(input_path, seed_seq, std::string(node_text),
                                                                       output_prefix, num_rates, burnin_frac, frame);
  });
}

int lhh_run_node_codons_pipeline(void* h, const char* input_path, const char* seed_seq, int node, const char* output_prefix,
                                 int num_rates, double burnin_frac, int frame) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunNodeCodonsPipeline(input_path, seed_seq, node, output_prefix, num_rates,
                                                                       burnin_frac, frame);
  });
}

// The writers' text of caller tables: codons [n_codons][64], change [n_codons][4]
int lhh_write_node_codons(const double* codons, const double* change, int n_codons, int frame, const char** out) {
  return Guard([&] {
    if (n_codons < 0 || frame < 0 || frame > 2) throw std::runtime_error("lhh_write_node_codons: bad shape");
    PhyloHMM::NodeCodonsResult m;
    m.frame = frame;
    m.codons.resize(n_codons);
    m.change.resize(n_codons);
    for (int c = 0; c < n_codons; ++c) {
      std::copy(codons + c * 64, codons + (c + 1) * 64, m.codons[c].begin());
      std::copy(change + c * 4, change + (c + 1) * 4, m.change[c].begin());
    }
    *out = NodeCodonsText(m);
  });
}

// The three tables of a LineageReplacementsResult, separated by blank lines (WriteReplacementTable, WriteCodonChangeTable,
// WriteSeedChangeTable)
static const char* LineageReplacementsText(const PhyloHMM::LineageReplacementsResult& m) {
  std::ostringstream o;
  PhyloHMM::WriteReplacementTable(o, m);
  o << "\n";
  PhyloHMM::WriteCodonChangeTable(o, m);
  o << "\n";
  PhyloHMM::WriteSeedChangeTable(o, m);
  g_out = o.str();
  return g_out.c_str();
}

// PhyloHMM::LineageReplacements: codon_counts [cap_codons][4], aa_counts [cap_codons][441], seed_change [cap_codons][3],
// edge_change [cap_edges][cap_codons][3], edge_load [cap_edges][2], nodes [cap_edges]; *n_codons and *n_edges (the chain's
// length + 1) receive the counts, *text the three tables as the writers print them.  codon_counts == NULL: only the frame
// check and *n_codons, nothing is evaluated; cap_edges too small: *n_edges alone is set and nothing is copied.
int lhh_phylo_lineage_replacements(void* h, const char* seed_seq, int frame, double* codon_counts, double* aa_counts,
                                   double* seed_change, int cap_codons, double* edge_change, double* edge_load, int32_t* nodes,
                                   int cap_edges, int* n_codons, int* n_edges, double* loglik, const char** text) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    if (frame < 0 || frame > 2) throw std::runtime_error("LineageReplacements: frame must be 0, 1 or 2");
    const int L = (int)p.msa().cols();
    *n_codons = L >= frame ? (L - frame) / 3 : 0;
    if (!codon_counts) return;
    const PhyloHMM::LineageReplacementsResult m = p.LineageReplacements(seed_seq, frame);
    const std::size_t C = m.codon_counts.size(), E = m.nodes.size() + 1;
    if ((int)C > cap_codons) throw std::runtime_error("lhh_phylo_lineage_replacements: output too small");
    *n_edges = (int)E;
    for (std::size_t c = 0; c < C; ++c) {
      std::copy(m.codon_counts[c].begin(), m.codon_counts[c].end(), codon_counts + c * 4);
      if (aa_counts) std::copy(m.aa_counts[c].begin(), m.aa_counts[c].end(), aa_counts + c * 441);
      if (seed_change) std::copy(m.seed_change[c].begin(), m.seed_change[c].end(), seed_change + c * 3);
    }
    if ((int)E <= cap_edges) {
      if (edge_change) std::copy(m.edge_change.begin(), m.edge_change.end(), edge_change);
      for (std::size_t e = 0; e < E && edge_load; ++e) std::copy(m.edge_load[e].begin(), m.edge_load[e].end(), edge_load + 2 * e);
      if (nodes) std::copy(m.nodes.begin(), m.nodes.end(), nodes);
    }
    if (loglik) *loglik = m.loglik;
    if (text) *text = LineageReplacementsText(m);
  });
}

int lhh_run_lineage_replacements_pipeline(void* h, const char* input_path, const char* seed_seq, const char* output_prefix,
                                          int num_rates, double burnin_frac, int frame) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunLineageReplacementsPipeline(input_path, seed_seq, output_prefix, num_rates,
                                                                                burnin_frac, frame);
  });
}

// The writers' text of caller tables: codon_counts [n_codons][4], aa_counts [n_codons][441], seed_change [n_codons][3]
int lhh_write_lineage_replacements(const double* codon_counts, const double* aa_counts, const double* seed_change, int n_codons,
                                   int frame, const char** out) {
  return Guard([&] {
    if (n_codons < 0 || frame < 0 || frame > 2) throw std::runtime_error("lhh_write_lineage_replacements: bad shape");
    PhyloHMM::LineageReplacementsResult m;
    m.frame = frame;
    m.codon_counts.resize(n_codons);
    m.aa_counts.resize(n_codons);
    m.seed_change.resize(n_codons);
    for (int c = 0; c < n_codons; ++c) {
      std::copy(codon_counts + c * 4, codon_counts + (c + 1) * 4, m.codon_counts[c].begin());
      std::copy(aa_counts + c * 441, aa_counts + (c + 1) * 441, m.aa_counts[c].begin());
      std::copy(seed_change + c * 3, seed_change + (c + 1) * 3, m.seed_change[c].begin());
    }
    *out = LineageReplacementsText(m);
  });
}

// WriteAncestralProbsTable's text of K candidates: names and seqs joined by '\n'; *covered receives CoveredMass
int lhh_write_ancestral_probs_table(const char* names, const char* seqs, const double* prob, int K, const char** out,
                                    double* covered) {
  return Guard([&] {
    linearham::AncestralProbsTable t;
    std::istringstream a(names), b(seqs);
    for (std::string line; std::getline(a, line);) t.names.push_back(line);
    for (std::string line; std::getline(b, line);) t.seqs.push_back(line);
    if ((int)t.names.size() != K || (int)t.seqs.size() != K) throw std::runtime_error("lhh_write_ancestral_probs_table: bad shape");
    t.prob.assign(prob, prob + K);
    std::ostringstream o;
    linearham::WriteAncestralProbsTable(o, t);
    g_out = o.str();
    *out = g_out.c_str();
    if (covered) *covered = linearham::CoveredMass(t);
  });
}

// ReadNamedCandidateFile: "name\tsequence" lines
int lhh_read_named_candidates(const char* path, int n_sites, const char** out) {
  return Guard([&] {
    const linearham::NamedCandidates c = linearham::ReadNamedCandidateFile(path, n_sites);
    std::string s;
    for (std::size_t k = 0; k < c.seqs.size(); ++k) s += c.names[k] + "\t" + c.seqs[k] + "\n";
    g_out = s;
    *out = g_out.c_str();
  });
}

int lhh_parse_lineage_node(const char* name, int* node) {
  return Guard([&] { *node = linearham::ParseLineageNode(name); });
}

// ParseLineageNodeText: *names receives the names of 'mrca-with:...' joined by '\n' (empty for the two fixed nodes)
int lhh_parse_lineage_node_text(const char* text, int* node, const char** names) {
  return Guard([&] {
    const linearham::LineageNode n = linearham::ParseLineageNodeText(text);
    *node = n.node;
    g_out.clear();
    for (const std::string& s : n.with) g_out += (g_out.empty() ? "" : "\n") + s;
    *names = g_out.c_str();
  });
}

int lhh_run_lineage_substitutions_pipeline(void* h, const char* input_path, const char* seed_seq, const char* output_prefix,
                                           int num_rates, double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunLineageSubstitutionsPipeline(input_path, seed_seq, output_prefix, num_rates,
                                                                                 burnin_frac);
  });
}

// PhyloHMM::NaiveCodonMarginals: table [cap_codons][125]; *n_codons receives the count; the amino-acid table
// (WriteAminoAcidTable) in *aa.  table == NULL: only *n_codons, nothing is evaluated.
int lhh_phylo_codon_marginals(void* h, int frame, double* table, int cap_codons, int* n_codons, const char** aa) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    if (frame < 0 || frame > 2) throw std::runtime_error("frame must be 0, 1 or 2");
    const int L = (int)p.msa().cols();
    *n_codons = L >= frame ? (L - frame) / 3 : 0;
    if (!table) return;
    const PhyloHMM::CodonMarginalsResult m = p.NaiveCodonMarginals(frame);
    if ((int)m.codons.size() > cap_codons) throw std::runtime_error("lhh_phylo_codon_marginals: output too small");
    for (std::size_t c = 0; c < m.codons.size(); ++c) std::copy(m.codons[c].begin(), m.codons[c].end(), table + c * 125);
    std::ostringstream o;
    PhyloHMM::WriteAminoAcidTable(o, m);
    g_out = o.str();
    *aa = g_out.c_str();
  });
}

int lhh_run_codon_marginals_pipeline(void* h, const char* input_path, const char* output_prefix, int num_rates,
                                     double burnin_frac, int frame) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunCodonMarginalsPipeline(input_path, output_prefix, num_rates,
                                                                             burnin_frac, frame);
  });
}

// The three tables of an EventsResult, separated by blank lines (WriteDeletionTable, WriteInsertionTable, WriteSpanTable).
static const char* EventsText(const PhyloHMM::EventsResult& m) {
  std::ostringstream o;
  PhyloHMM::WriteDeletionTable(o, m);
  o << "\n";
  PhyloHMM::WriteInsertionTable(o, m);
  o << "\n";
  PhyloHMM::WriteSpanTable(o, m);
  g_out = o.str();
  return g_out.c_str();
}

// PhyloHMM::EventsSize / EventsGenes: the lengths MapEvents expects (no device).
int lhh_phylo_events_sizes(void* h, int64_t* size, int* n_genes) {
  return Guard([&] {
    const PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    *size = (int64_t)p.EventsSize();
    *n_genes = (int)p.EventsGenes();
  });
}

// PhyloHMM::MapEvents on a caller's row events[EventsSize] and genes[EventsGenes] (no device): the tables' text in *text.
int lhh_phylo_map_events(void* h, const double* events, const double* genes, const char** text) {
  return Guard([&] { *text = EventsText(dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).MapEvents(events, genes)); });
}

// PhyloHMM::RearrangementEvents of the current tree: the tables' text in *text.
int lhh_phylo_events(void* h, const char** text) {
  return Guard([&] { *text = EventsText(dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RearrangementEvents()); });
}

int lhh_run_events_pipeline(void* h, const char* input_path, const char* output_prefix, int num_rates, double burnin_frac) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunEventsPipeline(input_path, output_prefix, num_rates, burnin_frac);
  });
}

// PhyloHMM::CandidatePosterior: seqs = K candidates of n_sites characters, back to back; log_post [K], log_prior [K]
// (may be NULL), *loglik.
int lhh_phylo_candidate_posterior(void* h, int K, const char* seqs, double* log_post, double* log_prior, double* loglik) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    const std::size_t L = p.msa().cols();
    std::vector<std::string> v;
    for (int k = 0; k < K; ++k) v.emplace_back(seqs + k * L, L);
    std::vector<double> lp;
    const std::vector<double> lc = p.CandidatePosterior(v, loglik, &lp);
    std::copy(lc.begin(), lc.end(), log_post);
    if (log_prior) std::copy(lp.begin(), lp.end(), log_prior);
  });
}

// K6c against HMM::ApplySampledStates on the same states [n][lh_sample_states()]: dev_seqs [n][L] (0..4) and hash [n]
// from lh_naive_sequences, host_seqs [n][L] the host's naive_seq characters.
int lhh_phylo_naive_sequences(void* h, int n, const int32_t* states, uint8_t* dev_seqs, uint64_t* hash, char* host_seqs) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    lh_family* f = p.family();
    const std::size_t L = p.msa().cols(), S = (std::size_t)lh_sample_states(f);
    if (S == 0) throw std::runtime_error("the family has no device sampler");
    if (lh_naive_sequences(f, n, states, dev_seqs, hash)) throw std::runtime_error(lh_last_error());
    HMM::RowSampler s;
    for (int i = 0; i < n; ++i) {
      p.ApplySampledStates(s, states + i * S);
      std::copy(s.naive_seq.begin(), s.naive_seq.end(), host_seqs + i * L);
    }
  });
}

// The host way of collecting draws, for the benchmark: HMM::ApplySampledStates on states [n][S] and a map from the naive
// sequence strings to ids in first-appearance order; *n_distinct, and the seconds it took in *seconds.
int lhh_phylo_apply_states_map(void* h, int n, const int32_t* states, int* n_distinct, double* seconds) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    const std::size_t S = (std::size_t)lh_sample_states(p.family());
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_map<std::string, int> ids;
    std::vector<int> row(n);
    HMM::RowSampler s;
    for (int i = 0; i < n; ++i) {
      p.ApplySampledStates(s, states + i * S);
      row[i] = ids.emplace(s.naive_seq, (int)ids.size()).first->second;
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *n_distinct = (int)ids.size();
  });
}

// PhyloHMM::ViterbiAnnotation: *out = "header line\nvalue line" of the annotation columns (tab-separated); *log_path,
// *loglik.  states (optional, cap ints): the path in lh_eval_sample_batch's layout, *n_states its length.
int lhh_phylo_viterbi_annotation(void* h, double* log_path, double* loglik, const char** out) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    const HMM::RowSampler s = p.ViterbiAnnotation(log_path, loglik);
    g_out = p.AnnotationHeader() + "\n";
    p.AppendAnnotationColumns(g_out, s);
    *out = g_out.c_str();
  });
}

// The annotation columns (PhyloHMM::AppendAnnotationColumns) of n state vectors states [n][lh_sample_states()], one line
// each in *out; no device work.
int lhh_phylo_annotation_columns(void* h, int n, int n_states, const int32_t* states, const char** out) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    HMM::RowSampler s;
    g_out.clear();
    for (int i = 0; i < n; ++i) {
      p.ApplySampledStates(s, states + (std::size_t)i * n_states);
      p.AppendAnnotationColumns(g_out, s);
      g_out.push_back('\n');
    }
    *out = g_out.c_str();
  });
}

// SimpleHMM::ViterbiPath: the naive sequence of the most probable path in *out, log P(data, path) in *log_path.
int lhh_simple_viterbi_path(void* h, double* log_path, const char** out) {
  return Guard([&] {
    const HMM::RowSampler s = dynamic_cast<SimpleHMM&>(*static_cast<HMM*>(h)).ViterbiPath(log_path);
    g_out = s.naive_seq;
    *out = g_out.c_str();
  });
}

int lhh_run_annotations_pipeline(void* h, const char* input_path, const char* output_prefix, int num_rates,
                                 double burnin_frac, int max_candidates) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h))
        .RunAnnotationsPipeline(input_path, output_prefix, num_rates, burnin_frac, max_candidates);
  });
}

int lhh_run_naive_probs_pipeline(void* h, const char* input_path, const char* output_prefix, int num_rates,
                                 double burnin_frac, const char* candidates_path, int max_candidates) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h))
        .RunNaiveProbsPipeline(input_path, output_prefix, num_rates, burnin_frac, candidates_path ? candidates_path : "",
                               max_candidates);
  });
}

// The naive-probability writers and helpers on caller data (no GPU).  seqs: K lines; count / freq NULL: no sampled
// columns (NA).  *out: the .naive.tsv text, then a line "\x1e", the .aa.fasta text, "\x1e", the .dnamap text.
int lhh_naive_probs_write(int K, const char* seqs, const double* prob, const double* log_prior, const int64_t* count,
                          const double* freq, const char** out) {
  return Guard([&] {
    NaiveProbsTable t;
    std::istringstream in(seqs);
    std::string line;
    while (std::getline(in, line))
      if (!line.empty()) t.seqs.push_back(line);
    if ((int)t.seqs.size() != K) throw std::runtime_error("lhh_naive_probs_write: K does not match the sequences");
    t.prob.assign(prob, prob + K);
    t.log_prior.assign(log_prior, log_prior + K);
    if (count && freq) {
      t.sampled = true;
      t.count.assign(count, count + K);
      t.freq.assign(freq, freq + K);
    }
    std::ostringstream o;
    WriteNaiveTable(o, t);
    o << "\x1e\n";
    WriteAaFasta(o, t);
    o << "\x1e\n";
    WriteDnaMap(o, t);
    g_out = o.str();
    *out = g_out.c_str();
  });
}
int lhh_translate(const char* dna, const char** out) {
  return Guard([&] {
    g_out = TranslateDna(dna);
    *out = g_out.c_str();
  });
}
int lhh_repr_double(double v, const char** out) {
  return Guard([&] {
    g_out = ReprDouble(v);
    *out = g_out.c_str();
  });
}
// ReadCandidateFile: the sequences, one per line
int lhh_read_candidates(const char* path, int n_sites, const char** out) {
  return Guard([&] {
    std::string s;
    for (const std::string& q : ReadCandidateFile(path, n_sites)) s += q + "\n";
    g_out = s;
    *out = g_out.c_str();
  });
}

int lhh_run_pipeline(void* h, const char* input_path, const char* output_path, int num_rates) {
  return Guard([&] { dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunPipeline(input_path, output_path, num_rates); });
}
int lhh_run_asr(void* h, const char* input_path, const char* output_path, uint64_t seed) {
  return Guard([&] { dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunAsr(input_path, output_path, seed); });
}
int lhh_run_lineage_pipeline(void* h, const char* input_path, const char* seed_seq, const char* output_prefix,
                             uint64_t seed) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunLineagePipeline(input_path, seed_seq, output_prefix, seed);
  });
}
int lhh_run_weighted_lineage_pipeline(void* h, const char* input_path, const char* seed_seq, const char* output_prefix,
                                      int num_rates, double burnin_frac, int draws_per_row, uint64_t seed) {
  return Guard([&] {
    dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).RunWeightedLineagePipeline(input_path, seed_seq, output_prefix, num_rates,
                                                                             burnin_frac, draws_per_row, seed);
  });
}
// TabulateLineageTrees: a file of RunAsr lines -> the lineage tables (no family, no GPU)
int lhh_lineage_tabulate_trees(const char* trees_path, const char* seed_seq, const char* output_prefix) {
  return Guard([&] { TabulateLineageTrees(trees_path, seed_seq, output_prefix); });
}
// the same with one log-weight per tree line (weights_path NULL or empty: none)
int lhh_lineage_tabulate_trees_weighted(const char* trees_path, const char* seed_seq, const char* output_prefix,
                                        const char* weights_path) {
  return Guard([&] { TabulateLineageTrees(trees_path, seed_seq, output_prefix, weights_path ? weights_path : ""); });
}
// what: bit 0 = state space + transitions, bit 1 = forward arrays, bit 2 = sample, bit 3 = xMSA structures

int lhh_dump_json(void* h, int what, const char** out) {
  return Guard([&] {
    HMM* hmm = static_cast<HMM*>(h);
    Json j;
    if (what & 1) DumpHMM(*hmm, j);
    if (what & 2) DumpForward(*hmm, j);
    if (what & 4) DumpSample(*hmm, j);
    if (what & 8) {
      PhyloHMM& p = dynamic_cast<PhyloHMM&>(*hmm);
      DumpPhylo(p, j);
      j.put("xmsa_emission", p.xmsa_emission());
      j.put("sr", p.sr());
      j.put("er", p.er());
      j.put("pi", p.pi());
      j.put("alpha", p.alpha());
    }
    g_out = j.str();
    *out = g_out.c_str();
  });
}

// Flatten a RevBayes table into the device inputs of lh_eval_batch_device (bench.py): fills
// caller-allocated arrays; returns max_depth through *max_depth.  n rows are taken cyclically from
// the table.  ops [n][T-2][4], brlen [n][2T-2], er [n][6], pi [n][4], alpha [n].
int lhh_phylo_flatten_tsv(void* h, const char* tsv_path, int n, int32_t* ops, double* brlen, double* er,
                          double* pi, double* alpha, int* n_tips, int* max_depth, int* n_rows_in_file,
                          int need_family, void** family) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    int n_file = 0;
    const PhyloHMM::DeviceBatch b = p.FlattenTsv(tsv_path, &n_file);
    *n_rows_in_file = n_file;
    struct {
      std::size_t n;
      std::size_t size() const { return n; }
    } rows{(std::size_t)n_file};
    *n_tips = b.n_tips;
    *max_depth = b.max_depth;
    *family = need_family ? p.family() : nullptr;
    if (n > 0 && ops) {
      const std::size_t T = b.n_tips, no = (T - 2) * 4, nb = 2 * T - 2;
      for (int s = 0; s < n; ++s) {
        const std::size_t r = s % rows.size();
        std::memcpy(ops + s * no, b.ops.data() + r * no, no * sizeof(int32_t));
        std::memcpy(brlen + s * nb, b.brlen.data() + r * nb, nb * sizeof(double));
        std::memcpy(er + s * 6, b.er.data() + r * 6, 6 * sizeof(double));
        std::memcpy(pi + s * 4, b.pi.data() + r * 4, 4 * sizeof(double));
        alpha[s] = b.alpha[r];
      }
    }
  });
}

// The rows `row_ids[0..n)` of the table (any order, repeats allowed) as device inputs: only these rows are parsed and
// scheduled (a rank of a multi-GPU run flattens the rows it evaluates, not the whole table).
int lhh_phylo_flatten_tsv_rows(void* h, const char* tsv_path, int n, const int64_t* row_ids, int32_t* ops, double* brlen,
                               double* er, double* pi, double* alpha, int* n_tips, int* max_depth, int* n_rows_in_file,
                               int need_family, void** family) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    int n_file = 0;
    const PhyloHMM::DeviceBatch b = p.FlattenTsvRows(tsv_path, row_ids, n, &n_file);
    *n_rows_in_file = n_file;
    *n_tips = b.n_tips;
    *max_depth = b.max_depth;
    *family = need_family ? p.family() : nullptr;
    std::memcpy(ops, b.ops.data(), b.ops.size() * sizeof(int32_t));
    std::memcpy(brlen, b.brlen.data(), b.brlen.size() * sizeof(double));
    std::memcpy(er, b.er.data(), b.er.size() * sizeof(double));
    std::memcpy(pi, b.pi.data(), b.pi.size() * sizeof(double));
    std::memcpy(alpha, b.alpha.data(), b.alpha.size() * sizeof(double));
  });
}

int lhh_phylo_set_devices(void* h, const int* devices, int n) {
  return Guard([&] { dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h)).SetDevices(std::vector<int>(devices, devices + n)); });
}

int lhh_phylo_sizes(void* h, int* n_tips, int* n_sites, int* n_xmsa, int* s_vd, int* s_dj, int* w_vd, int* w_dj,
                    int* g_total) {
  return Guard([&] {
    PhyloHMM& p = dynamic_cast<PhyloHMM&>(*static_cast<HMM*>(h));
    *n_tips = p.msa().rows() + 1;
    *n_sites = p.msa().cols();
    *n_xmsa = p.n_xmsa();
    *s_vd = (int)p.vd_junction_state_strs().size();
    *s_dj = (int)p.dj_junction_state_strs().size();
    *w_vd = p.vd_junction_xmsa_inds().rows();
    *w_dj = p.dj_junction_xmsa_inds().rows();
    *g_total = (int)(p.vpadding_xmsa_inds().size() + p.vgerm_xmsa_inds().size() + p.dgerm_xmsa_inds().size() +
                     p.jgerm_xmsa_inds().size() + p.jpadding_xmsa_inds().size());
  });
}

// Self-test of DrawDiscreteSparse (HMM.hpp) against std::discrete_distribution on the full weight vector:
// random sizes and sparsity patterns plus the corner cases (first / last weight zero or not, a single
// non-zero weight, all weights zero, fewer than two weights).  Both generators start from the same seed
// and must agree on every sampled index and stay in the same state.  Returns the number of disagreements.
int lhh_selftest_sparse_draw(int seed, int trials) {
  std::mt19937 gen(seed), a(seed + 1), b(seed + 1);
  int bad = 0;
  for (int t = 0; t < trials; ++t) {
    const int size = (t % 17 == 0) ? 1 : 2 + (int)(gen() % 60);
    std::vector<double> w(size, 0.0);
    const int mode = (int)(gen() % 6);
    for (int i = 0; i < size; ++i) {
      const bool on = mode == 0 ? (gen() % 4 == 0) : mode == 1 ? (i == size - 1) : mode == 2 ? (i == 0)
                    : mode == 3 ? false : mode == 4 ? (i != 0 && i != size - 1 && gen() % 3 == 0) : true;
      if (on) w[i] = std::ldexp((double)(gen() % 100000 + 1), -(int)(gen() % 600));
    }
    std::vector<int> idx;
    std::vector<double> nz;
    for (int i = 0; i < size; ++i)
      if (w[i] != 0.0) {
        idx.push_back(i);
        nz.push_back(w[i]);
      }
    std::discrete_distribution<int> dist;
    dist.param(std::discrete_distribution<int>::param_type(w.data(), w.data() + size));
    const int dense = dist(a);
    const int sparse = DrawDiscreteSparse(b, idx.data(), nz.data(), (int)idx.size(), size);
    if (dense != sparse || a != b) ++bad;
  }
  return bad;
}

// Self-test of ParseDouble / AppendFixed6 (newick.hpp) against strtod / printf("%f"): random values in the forms
// a RevBayes table and libpll's exporter produce, plus exact ties of the sixth decimal.  Returns the mismatches.
int lhh_selftest_numbers(int seed, int trials) {
  std::mt19937_64 rng((uint64_t)seed);
  int bad = 0;
  char buf[96];
  auto check_parse = [&](const char* s) {
    const char* e1 = nullptr;
    char* e2 = nullptr;
    const double a = ParseDouble(s, &e1), b = std::strtod(s, &e2);
    if (std::memcmp(&a, &b, sizeof a) != 0 || e1 != e2) ++bad;
  };
  auto check_fixed = [&](double v) {
    std::string o;
    AppendFixed6(o, v);
    std::snprintf(buf, sizeof buf, "%f", v);
    if (o != buf) ++bad;
  };
  const char* fixed_cases[] = {"0", "0.0", "1e-06", "1E-6", "0.0078125", ".5", "5.", "12345678901234567890", "1e400",
                               "0.1e-320", "123.456e+10", "7e", "1e+", "0.30000000000000004", "9007199254740993",
                               "4.9e-324", "x", "", "-0.25", "+3.5e2:"};
  for (const char* c : fixed_cases) check_parse(c);
  for (int i = 0; i < trials; ++i) {
    const double u = (double)(rng() >> 11) * 0x1p-53;
    const int e = (int)(rng() % 14) - 9;
    const double v = u * std::pow(10.0, e);
    const char* fmts[] = {"%.6g", "%.8g", "%.10g", "%.17g", "%f", "%.12f", "%e"};
    std::snprintf(buf, sizeof buf, fmts[rng() % 7], v);
    check_parse(buf);
    check_fixed(v);
    // exact halves of the sixth decimal that are binary fractions: (2m + 1) * 15625 / 2^(7 + j)
    const double tie = (double)(2 * (rng() % 4096) + 1) * 15625.0 * std::ldexp(1.0, -7 - (int)(rng() % 6)) / 15625.0 /
                       15625.0 * 15625.0;
    check_fixed(tie);
    check_fixed((double)(rng() % 2000001) * 0.0078125);
    check_fixed((double)(rng() % 1000) + 0.5e-6 * (double)(rng() % 3));
  }
  check_fixed(0.0078125);
  check_fixed(0.0);
  check_fixed(1e-7);
  check_fixed(4e9);
  check_fixed(123456789.9999995);
  return bad;
}

// Newick ingest + re-export without a device: `labels` is a '\n'-separated list (first = naive).  *out is the
// output table's tree column (ExportNewick); children/brlen/root may be NULL.
int lhh_newick_roundtrip(const char* newick, const char* labels, const char** out, int32_t* children,
                         double* brlen, int32_t* root) {
  return Guard([&] {
    std::vector<std::string> labs;
    std::string cur;
    for (const char* c = labels; *c; ++c) {
      if (*c == '\n') {
        labs.push_back(cur);
        cur.clear();
      } else {
        cur.push_back(*c);
      }
    }
    if (!cur.empty()) labs.push_back(cur);
    const TreeArrays tr = ParseNewick(newick, labs, EPS, true);
    g_out = ExportNewick(tr, labs);
    *out = g_out.c_str();
    if (children) std::copy(tr.children.begin(), tr.children.end(), children);
    if (brlen) std::copy(tr.brlen.begin(), tr.brlen.end(), brlen);
    if (root) *root = tr.root;
  });
}

}  // extern "C"
