#include "PhyloHMM.hpp"

#include "Lineage.hpp"
#include "NaiveProbs.hpp"

#include <cerrno>
#include <fcntl.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>
#include <tuple>
#include <unordered_map>

namespace linearham {

// src/PhyloHMM.cpp:29-34
PhyloHMM::PhyloHMM(const std::string& yaml_path, int cluster_ind, const std::string& hmm_param_dir, int seed)
    : HMM(yaml_path, cluster_ind, hmm_param_dir, seed) {
  InitializeXmsaStructs();
}

// src/PhyloHMM.cpp:45-89 (+ BuildXmsa, :123-144)
void PhyloHMM::InitializeXmsaStructs() {
  xmsa_labels_.push_back("naive");
  for (const auto& n : cluster_data_["unique_ids"].seq) xmsa_labels_.push_back(n.as_string());
  xmsa_naive_ind_ = 0;
  std::map<std::pair<int, int>, int> xmsa_ids;
  StoreGermlinePaddingXmsaIndices(vpadding_.naive_bases, vpadding_.site_inds, xmsa_ids, vpadding_xmsa_inds_);
  StoreGermlinePaddingXmsaIndices(vgerm_.naive_bases, vgerm_.site_inds, xmsa_ids, vgerm_xmsa_inds_);
  if (locus_ == "igh") {
    StoreJunctionXmsaIndices(vd_junction_.naive_bases, vd_junction_.site_inds, flexbounds_.at("v_r"),
                             flexbounds_.at("d_l"), xmsa_ids, vd_junction_xmsa_inds_);
    StoreGermlinePaddingXmsaIndices(dgerm_.naive_bases, dgerm_.site_inds, xmsa_ids, dgerm_xmsa_inds_);
    StoreJunctionXmsaIndices(dj_junction_.naive_bases, dj_junction_.site_inds, flexbounds_.at("d_r"),
                             flexbounds_.at("j_l"), xmsa_ids, dj_junction_xmsa_inds_);
  } else {
    StoreJunctionXmsaIndices(vd_junction_.naive_bases, vd_junction_.site_inds, flexbounds_.at("v_r"),
                             flexbounds_.at("j_l"), xmsa_ids, vd_junction_xmsa_inds_);
  }
  StoreGermlinePaddingXmsaIndices(jgerm_.naive_bases, jgerm_.site_inds, xmsa_ids, jgerm_xmsa_inds_);
  StoreGermlinePaddingXmsaIndices(jpadding_.naive_bases, jpadding_.site_inds, xmsa_ids, jpadding_xmsa_inds_);

  const int n = msa_.rows(), C = (int)xmsa_ids.size();
  xmsa_.setConstant(n + 1, C, -1);
  xmsa_site_.assign(C, 0);
  xmsa_base_.assign(C, 0);
  for (auto it = xmsa_ids.begin(); it != xmsa_ids.end(); ++it) {
    const int naive_base = it->first.first, msa_ind = it->first.second, xmsa_ind = it->second;
    xmsa_(0, xmsa_ind) = naive_base;
    for (int r = 0; r < n; ++r) xmsa_(r + 1, xmsa_ind) = msa_(r, msa_ind);
    xmsa_site_[xmsa_ind] = msa_ind;
    xmsa_base_[xmsa_ind] = (uint8_t)naive_base;
  }
  xmsa_seqs_.assign(n + 1, "");
  for (int r = 0; r < n + 1; ++r) {
    VectorXi row(xmsa_.row(r), xmsa_.row(r) + C);
    xmsa_seqs_[r] = ConvertIntsToSeq(row, alphabet_);
  }
}

namespace {

// Worker threads a host stage may start: the cores this process may run on (its affinity mask; a container's share can
// be smaller than the machine), at most `cap`; LH_HOST_THREADS overrides the count (experiments, small containers).
// The stages of RunPipeline run side by side with up to 16 workers each (measured on a 256-thread host, 262144 rows of
// configs[2]: 8 workers 1.22 s, 16 1.02 s, 24 1.22 s, 32 1.05 s -- profiles/r03_pipeline_e2e.txt).
int HostThreads(int cap) {
  static const int avail = [] {
    if (host_options().host_threads > 0) return host_options().host_threads;
    int n = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min(n > 0 ? n : 1 << 20, CPU_COUNT(&set));
    return std::max(1, n);
  }();
  return std::max(1, std::min(avail, cap));
}

// fn(w, lo, hi) for every worker w < n_threads with its share [lo, hi) of 0 .. total: inline when there is one worker,
// on threads of their own otherwise.  All are joined; then the first exception in worker order is rethrown here.
template <class Fn>
void ForRanges(int n_threads, std::size_t total, Fn&& fn) {
  std::vector<std::exception_ptr> errors(n_threads);
  std::vector<std::thread> pool;
  for (int w = 0; w < n_threads; ++w) {
    const std::size_t lo = total * w / n_threads, hi = total * (w + 1) / n_threads;
    auto body = [&, w, lo, hi] {
      try {
        fn(w, lo, hi);
      } catch (...) {
        errors[w] = std::current_exception();
      }
    };
    if (n_threads == 1)
      body();
    else
      pool.emplace_back(body);
  }
  for (std::thread& th : pool) th.join();
  for (const std::exception_ptr& e : errors)
    if (e) std::rethrow_exception(e);
}

SegmentTables MakeSegments(const GeneRanges& ranges, const VectorXi& inds) {
  SegmentTables s;
  s.offsets.push_back(0);
  for (auto it = ranges.begin(); it != ranges.end(); ++it) {
    for (int j = it->second.first; j < it->second.second; ++j) s.xmsa_inds.push_back(inds[j]);
    s.offsets.push_back((int32_t)s.xmsa_inds.size());
  }
  return s;
}

}  // namespace

// Upload everything that is constant for this clonal family (lh_family_create).  Done lazily at the
// first evaluation so that the host-only state (state space, transitions, xMSA) can be inspected on a
// machine without a GPU; any evaluation without a GPU fails here (there is no CPU path).
void PhyloHMM::CreateFamily() {
  if (family_) return;
  const bool igh = locus_ == "igh";
  const int n = msa_.rows(), L = msa_.cols();
  std::vector<uint8_t> msa8((std::size_t)n * L);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < L; ++c) msa8[(std::size_t)r * L + c] = (uint8_t)msa_(r, c);
  const SegmentTables vpad = MakeSegments(vpadding_.ggene_ranges, vpadding_xmsa_inds_);
  const SegmentTables vger = MakeSegments(vgerm_.ggene_ranges, vgerm_xmsa_inds_);
  const SegmentTables dger = MakeSegments(dgerm_.ggene_ranges, dgerm_xmsa_inds_);
  const SegmentTables jger = MakeSegments(jgerm_.ggene_ranges, jgerm_xmsa_inds_);
  const SegmentTables jpad = MakeSegments(jpadding_.ggene_ranges, jpadding_xmsa_inds_);
  std::vector<double> gene_prob, trans_prod;
  for (auto it = vgerm_.ggene_ranges.begin(); it != vgerm_.ggene_ranges.end(); ++it) {
    const Germline& g = *ggenes_.at(it->first).germ_ptr;
    gene_prob.push_back(g.gene_prob());
    const int gis = vgerm_.germ_inds[it->second.first];
    double prod = 1.0;  // src/HMM.cpp:310-313
    for (int k = 0; k < it->second.second - it->second.first - 1; ++k) prod *= g.transition()[gis + k];
    trans_prod.push_back(prod);
  }
  JunctionTables vd, dj;
  if (igh) {
    vd = BuildJunctionTables(vd_junction_, vgerm_, dgerm_, flexbounds_.at("v_r"), flexbounds_.at("d_l"),
                             vd_junction_xmsa_inds_);
    dj = BuildJunctionTables(dj_junction_, dgerm_, jgerm_, flexbounds_.at("d_r"), flexbounds_.at("j_l"),
                             dj_junction_xmsa_inds_);
  } else {
    vd = BuildJunctionTables(vd_junction_, vgerm_, jgerm_, flexbounds_.at("v_r"), flexbounds_.at("j_l"),
                             vd_junction_xmsa_inds_);
  }
  lh_family_desc d{};
  d.abi_version = LH_ABI_VERSION;
  d.has_d = igh ? 1 : 0;
  d.n_seqs = n;
  d.n_sites = L;
  d.msa = msa8.data();
  d.n_xmsa = xmsa_.cols();
  d.xmsa_site = xmsa_site_.data();
  d.xmsa_naive_base = xmsa_base_.data();
  d.vpadding = vpad.c();
  d.vgerm = vger.c();
  d.dgerm = dger.c();
  d.jgerm = jger.c();
  d.jpadding = jpad.c();
  d.vgerm_gene_prob = gene_prob.data();
  d.vpadding_transition = vpadding_transition_.data();
  d.vgerm_trans_prod = trans_prod.data();
  d.jpadding_transition = jpadding_transition_.data();
  d.vd = vd.c();
  if (igh) d.dj = dj.c();
  StageTimer timer;
  if (!devices_.empty()) CheckHip(lh_set_device(devices_[0]), "lh_set_device");
  CheckHip(lh_family_create(&d, &family_), "lh_family_create");
  timer.Mark("lh_family_create (+ HIP init)");
  // Device-side naive-sequence sampling (lh_eval_sample_batch).  The one structural condition it has -- the left and
  // the right genes of a junction occupy two blocks of the junction's state vector, true for gene names that start
  // with their locus and segment letters -- is checked by the library; a family that does not meet it keeps the
  // host sampler (the same algorithm, HMM::SampleRow), and so does LH_HOST_SAMPLING=1.
  if (!host_options().host_sampling) {
    SamplerJunction svd, sdj;
    lh_sampler_desc sd{};
    if (igh) {
      svd = BuildSamplerJunction(vd_junction_, vgerm_, dgerm_, flexbounds_.at("v_r"), flexbounds_.at("d_l"));
      sdj = BuildSamplerJunction(dj_junction_, dgerm_, jgerm_, flexbounds_.at("d_r"), flexbounds_.at("j_l"));
      sd.dj = sdj.c();
    } else {
      svd = BuildSamplerJunction(vd_junction_, vgerm_, jgerm_, flexbounds_.at("v_r"), flexbounds_.at("j_l"));
    }
    sd.vd = svd.c();
    device_sampler_ = lh_family_set_sampler(family_, &sd) == 0 && lh_sample_words(family_) == RawDrawsPerSample();
    timer.Mark("lh_family_set_sampler");
    // the other devices' handles: the same descriptors, uploaded with that device current (only when the rows will be
    // sampled on the devices: nothing else shards)
    for (std::size_t k = 1; device_sampler_ && k < devices_.size(); ++k) {
      CheckHip(lh_set_device(devices_[k]), "lh_set_device");
      lh_family* f = nullptr;
      CheckHip(lh_family_create(&d, &f), "lh_family_create");
      more_families_.push_back(f);
      if (device_sampler_ && lh_family_set_sampler(f, &sd) != 0) throw std::runtime_error(lh_last_error());
    }
  }
  // Only RunPipeline's device-sampling branch deals rows to several handles.  A family that keeps the host sampler
  // (LH_HOST_SAMPLING, or genes that do not form two blocks of a junction's state vector) evaluates everything on the
  // first listed device: say so instead of building handles nobody uses.
  if (devices_.size() > 1 && !device_sampler_) {
    std::fprintf(stderr, "linearham: --devices lists %zu devices, but this run samples on the host: all rows are evaluated on "
                 "device %d\n", devices_.size(), devices_[0]);
    for (lh_family* f : more_families_) lh_family_destroy(f);
    more_families_.clear();
  }
  if (devices_.size() > 1) CheckHip(lh_set_device(devices_[0]), "lh_set_device");
}

void PhyloHMM::SetDevices(const std::vector<int>& devices) {
  Require(family_ == nullptr, "SetDevices must be called before the first evaluation");
  for (int dev : devices) Require(dev >= 0 && dev < lh_device_count(), "SetDevices: no such device");
  devices_ = devices;
}

// src/PhyloHMM.cpp:350-361
void PhyloHMM::InitializePhyloParameters(const std::string& newick_path, const std::vector<double>& er,
                                         const std::vector<double>& pi, double alpha, int num_rates) {
  std::ifstream in(newick_path);
  if (!in) throw std::runtime_error("Can't open Newick file " + newick_path);
  std::stringstream ss;
  ss << in.rdbuf();
  InitializePhyloParametersFromString(ss.str(), er, pi, alpha, num_rates);
}

void PhyloHMM::InitializePhyloParametersFromString(const std::string& newick, const std::vector<double>& er,
                                                   const std::vector<double>& pi, double alpha, int num_rates) {
  Require(er.size() == 6 && pi.size() == 4, "er must have 6 and pi 4 entries");
  Require(num_rates >= 1, "num_rates must be positive");
  tree_ = ParseNewick(newick, xmsa_labels_, EPS, true);
  have_tree_ = true;
  er_ = er;
  pi_ = pi;
  alpha_ = alpha;
  num_rates_ = num_rates;
  sr_.assign(num_rates, 0.0);
}

PhyloHMM::DeviceBatch PhyloHMM::FlattenBatch(const std::vector<TreeSample>& samples, std::vector<TreeArrays>* trees,
                                             std::vector<std::string>* exported) const {
  DeviceBatch b;
  const int T = (int)xmsa_labels_.size();
  b.n = (int)samples.size();
  b.n_tips = T;
  b.ops.resize((std::size_t)b.n * (T - 2) * 4);
  b.brlen.resize((std::size_t)b.n * (2 * T - 2));
  b.er.resize((std::size_t)b.n * 6);
  b.pi.resize((std::size_t)b.n * 4);
  b.alpha.resize(b.n);
  if (trees) trees->resize(b.n);
  if (exported) exported->resize(b.n);
  // Rows are independent (parse, unroot at naive's neighbour, schedule): the GPU evaluates a few million
  // trees per second, one host core flattens a few ten thousand, so the rows are spread over the cores.
  auto flatten_rows = [&](int lo, int hi, int* max_depth) {
    for (int s = lo; s < hi; ++s) {
      const TreeSample& ts = samples[s];
      Require(ts.er.size() == 6 && ts.pi.size() == 4, "er must have 6 and pi 4 entries");
      TreeArrays tr = ParseNewick(ts.newick, xmsa_labels_, EPS, exported != nullptr);
      int32_t depth = 0;
      CheckHip(lh_schedule_tree(T, tr.children.data(), tr.root, b.ops.data() + (std::size_t)s * (T - 2) * 4, &depth),
               "lh_schedule_tree");
      *max_depth = std::max(*max_depth, (int)depth);
      std::copy(tr.brlen.begin(), tr.brlen.end(), b.brlen.begin() + (std::size_t)s * (2 * T - 2));
      std::copy(ts.er.begin(), ts.er.end(), b.er.begin() + (std::size_t)s * 6);
      std::copy(ts.pi.begin(), ts.pi.end(), b.pi.begin() + (std::size_t)s * 4);
      b.alpha[s] = ts.alpha;
      if (exported) {
        (*exported)[s] = ExportNewick(tr, xmsa_labels_);
        tr.as_parsed = std::string();
      }
      if (trees) (*trees)[s] = std::move(tr);
    }
  };
  const int hw = HostThreads(16);
  const int n_threads = std::max(1, std::min(hw, b.n / 64));
  std::vector<int> depths(n_threads, 0);
  // (an error: the first failing row range, in file order)
  ForRanges(n_threads, (std::size_t)b.n,
            [&](int w, std::size_t lo, std::size_t hi) { flatten_rows((int)lo, (int)hi, &depths[w]); });
  for (int d : depths) b.max_depth = std::max(b.max_depth, d);
  return b;
}

std::vector<double> PhyloHMM::LogLikelihoodBatch(const std::vector<TreeSample>& samples, int num_rates) {
  CreateFamily();
  const DeviceBatch b = FlattenBatch(samples);
  std::vector<double> ll(b.n);
  if (b.n == 0) return ll;
  CheckHip(lh_eval_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                         b.pi.data(), b.alpha.data(), num_rates, ll.data(), nullptr),
           "lh_eval_batch");
  return ll;
}

// src/PhyloHMM.cpp:366-383: one evaluation on the device (gamma rates, P-matrices, pruning, emission
// assembly, forward sweep).  The results are unpacked lazily, like the reference's cache_forward_.
void PhyloHMM::InitializePhyloEmission() {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  xmsa_emission_.assign(xmsa_.cols(), 0.0);
  pending_forward_.assign(lh_forward_size(family_), 0.0);
  pending_scalers_.assign(lh_scaler_size(family_), 0);
  lh_eval_outputs outs{sr_.data(), xmsa_emission_.data(), pending_forward_.data(), pending_scalers_.data()};
  CheckHip(lh_eval_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                         num_rates_, &pending_loglik_, &outs),
           "lh_eval_batch");
  cache_forward_ = true;
}

namespace {

// the state word whose tempered value is y (inverse of std::mt19937's output transformation)
uint32_t Untemper(uint32_t y) {
  y ^= y >> 18;
  y ^= (y << 15) & 0xEFC60000u;
  uint32_t t = y;
  for (int i = 0; i < 5; ++i) t = y ^ ((t << 7) & 0x9D2C5680u);
  y = t;
  t = y;
  for (int i = 0; i < 3; ++i) t = y ^ (t >> 11);
  return t;
}

}  // namespace

void PhyloHMM::SampleStatesWithWords(const uint32_t* words, int n_words, std::vector<int32_t>& device_states,
                                     std::vector<int32_t>& host_states) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler");
  const int raw = RawDrawsPerSample();
  Require(n_words >= raw && n_words <= 624, "SampleStatesWithWords: need RawDrawsPerSample() .. 624 words");
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  // device
  device_states.assign(lh_sample_states(family_), -1);
  double ll = 0;
  std::vector<double> rates(num_rates_);
  CheckHip(lh_eval_sample_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                num_rates_, words, &ll, rates.data(), device_states.data()),
           "lh_eval_sample_batch");
  // host: the same forward arrays, an engine that returns the same words
  std::vector<double> fwd(lh_forward_size(family_));
  std::vector<int32_t> sco(lh_scaler_size(family_));
  lh_eval_outputs outs{nullptr, nullptr, fwd.data(), sco.data()};
  CheckHip(lh_eval_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                         num_rates_, &ll, &outs),
           "lh_eval_batch");
  std::ostringstream st;
  for (int i = 0; i < 624; ++i) st << Untemper(i < n_words ? words[i] : 0u) << ' ';
  st << 0;  // position: the next output is the first word
  std::istringstream in(st.str());
  std::mt19937 rng;
  in >> rng;
  for (int i = 0; i < std::min(n_words, 4); ++i) {
    std::mt19937 probe = rng;
    probe.discard(i);
    Require((uint32_t)probe() == words[i], "SampleStatesWithWords: engine state construction failed");
  }
  EnsureSamplingLists();
  RowSampler s;
  SampleRow(s, fwd.data(), rng);
  host_states.clear();
  host_states.push_back(s.jgerm_state_ind);
  if (locus_ == "igh") {
    host_states.insert(host_states.end(), s.dj_junction_state_inds.begin(), s.dj_junction_state_inds.end());
    host_states.push_back(s.dgerm_state_ind);
  }
  host_states.insert(host_states.end(), s.vd_junction_state_inds.begin(), s.vd_junction_state_inds.end());
  host_states.push_back(s.vgerm_state_ind);
}

std::vector<double> PhyloHMM::NaivePosterior(double* loglik) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the posterior kernel)");
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  std::vector<double> post(lh_forward_size(family_));
  lh_posterior_outputs outs{nullptr, loglik, post.data(), nullptr, nullptr};
  CheckHip(lh_eval_posterior_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                   num_rates_, &outs),
           "lh_eval_posterior_batch");
  return post;
}

HMM::RowSampler PhyloHMM::ViterbiAnnotation(double* log_path, double* loglik) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the Viterbi kernel)");
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  std::vector<int32_t> states(lh_sample_states(family_));
  double lp = 0, ll = 0;
  lh_viterbi_outputs outs{nullptr, &ll, states.data(), &lp, nullptr};
  CheckHip(lh_eval_viterbi_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                 num_rates_, &outs),
           "lh_eval_viterbi_batch");
  Require(std::isfinite(ll), "ViterbiAnnotation: the log-likelihood is not finite");
  Require(states[0] >= 0, "ViterbiAnnotation: no state path has positive probability");
  if (log_path) *log_path = lp;
  if (loglik) *loglik = ll;
  RowSampler s;
  ApplySampledStates(s, states.data());
  return s;
}

// One walk over the compact posterior layout (lh_eval_outputs.forward: V | V-D rows | D | D-J rows | J): calls
// germ(region letter, gene name, index in the region, value, region) for every germline-region gene and
// junc(junction, row, dense state, site, naive base, value) for every junction state.  (Dense state posteriors in the
// shapes of the forward members: linearham_amd/posterior.py.)
template <typename G, typename J>
static void WalkPosterior(const std::string& locus, const std::map<std::string, std::pair<int, int>>& fb,
                          const RegionStates& vgerm, const RegionStates& vd, const RegionStates& dgerm,
                          const RegionStates& dj, const RegionStates& jgerm, const double* post, G&& germ, J&& junc) {
  const bool igh = locus == "igh";
  std::size_t off = 0;
  auto region = [&](char letter, const RegionStates& R) {
    int g = 0;
    for (const auto& kv : R.ggene_ranges) germ(letter, kv.first, g, post[off + g], R), ++g;
    off += R.ggene_ranges.size();
  };
  auto junction = [&](const RegionStates& Jn, const RegionStates& L, const RegionStates& Rt, int site0, int W) {
    const int nL = (int)L.ggene_ranges.size(), nR = (int)Rt.ggene_ranges.size();
    const std::size_t stride = (std::size_t)nL + 5 * (std::size_t)nR;
    int l = 0;
    for (const auto& kv : L.ggene_ranges) {
      const auto it = Jn.ggene_ranges.find(kv.first);
      if (it != Jn.ggene_ranges.end())
        for (int k = it->second.first; k < it->second.second; ++k) {
          const int i = Jn.site_inds[k] - site0;
          junc(Jn, i, k, Jn.site_inds[k], Jn.naive_bases[k], post[off + i * stride + l]);
        }
      ++l;
    }
    int r = 0;
    for (const auto& kv : Rt.ggene_ranges) {
      const auto it = Jn.ggene_ranges.find(kv.first);
      Require(it != Jn.ggene_ranges.end(), "posterior layout: right gene missing from its junction");
      const int rs = it->second.first, re = it->second.second;
      for (int i = 0; i < W; ++i)
        for (int a = 0; a < 4; ++a) junc(Jn, i, rs + a, site0 + i, a, post[off + i * stride + nL + 4 * r + a]);
      for (int k = rs + 4; k < re; ++k) {
        const int i = Jn.site_inds[k] - site0;
        junc(Jn, i, k, Jn.site_inds[k], Jn.naive_bases[k], post[off + i * stride + nL + 4 * (std::size_t)nR + r]);
      }
      ++r;
    }
    off += (std::size_t)W * stride;
  };
  region('V', vgerm);
  if (igh) {
    junction(vd, vgerm, dgerm, fb.at("v_r").first, fb.at("d_l").second - fb.at("v_r").first);
    region('D', dgerm);
    junction(dj, dgerm, jgerm, fb.at("d_r").first, fb.at("j_l").second - fb.at("d_r").first);
  } else {
    junction(vd, vgerm, jgerm, fb.at("v_r").first, fb.at("j_l").second - fb.at("v_r").first);
  }
  region('J', jgerm);
}

PhyloHMM::NaiveMarginalsResult PhyloHMM::MapPosterior(const double* post) const {
  NaiveMarginalsResult m;
  m.site_base.assign(msa_.cols(), {0.0, 0.0, 0.0, 0.0, 0.0});
  WalkPosterior(
      locus_, flexbounds_, vgerm_, vd_junction_, dgerm_, dj_junction_, jgerm_, post,
      [&](char letter, const std::string& name, int, double p, const RegionStates& R) {
        m.genes.emplace_back(letter, name, p);
        const auto& rg = R.ggene_ranges.at(name);
        for (int k = rg.first; k < rg.second; ++k) m.site_base[R.site_inds[k]][R.naive_bases[k]] += p;
      },
      [&](const RegionStates&, int, int, int site, int base, double p) { m.site_base[site][base] += p; });
  for (auto& s : m.site_base) s[4] += 1.0 - (s[0] + s[1] + s[2] + s[3] + s[4]);  // what no state writes stays N
  return m;
}

PhyloHMM::NaiveMarginalsResult PhyloHMM::NaiveMarginals() {
  double ll = 0;
  const std::vector<double> post = NaivePosterior(&ll);
  return MapPosterior(post.data());
}

void PhyloHMM::WriteSiteTable(std::ostream& o, const NaiveMarginalsResult& m) {
  static const char kBases[] = "ACGTN";
  char buf[64];
  o << "site\tA\tC\tG\tT\tN\tmap_base\n";
  for (std::size_t s = 0; s < m.site_base.size(); ++s) {
    const auto& p = m.site_base[s];
    o << s;
    for (double v : p) {
      std::snprintf(buf, sizeof buf, "%.17g", v);
      o << '\t' << buf;
    }
    o << '\t' << kBases[std::max_element(p.begin(), p.end()) - p.begin()] << '\n';
  }
}

void PhyloHMM::WriteGeneTable(std::ostream& o, const NaiveMarginalsResult& m) {
  std::vector<std::tuple<char, std::string, double>> g = m.genes;
  std::stable_sort(g.begin(), g.end(), [](const auto& a, const auto& b) { return std::get<2>(a) > std::get<2>(b); });
  char buf[64];
  o << "region\tgene\tprobability\n";
  for (const auto& t : g) {
    std::snprintf(buf, sizeof buf, "%.17g", std::get<2>(t));
    o << std::get<0>(t) << '\t' << std::get<1>(t) << '\t' << buf << '\n';
  }
}

void PhyloHMM::RunForwardAlgorithm() {
  UnpackForward(pending_forward_.data(), pending_scalers_.data());
  loglikelihood_ = pending_loglik_;
}

// src/PhyloHMM.cpp:244-282
void PhyloHMM::WriteOutputHeaders(std::ofstream& outfile) const {
  outfile << "Iteration\tRBLogLikelihood\tPrior\talpha\t";
  for (std::size_t i = 1; i <= er_.size(); i++) outfile << ("er[" + std::to_string(i) + "]\t");
  for (std::size_t i = 1; i <= pi_.size(); i++) outfile << ("pi[" + std::to_string(i) + "]\t");
  outfile << "tree\t";
  for (std::size_t i = 1; i <= sr_.size(); i++) outfile << ("sr[" + std::to_string(i) + "]\t");
  outfile << "LHLogLikelihood\tLogWeight\tNaiveSequence\tVGene\tV5pDel\tV3pDel\tVFwkInsertion\t";
  if (locus_ == "igh") {
    outfile << "VDInsertion\tDGene\tD5pDel\tD3pDel\tDJInsertion\t";
  } else {
    outfile << "VJInsertion\t";
  }
  outfile << "JGene\tJ5pDel\tJ3pDel\tJFwkInsertion\n";
}

namespace {

// operator<<(std::ostream&, double) with the stream's defaults = printf("%g")
void AppendG(std::string& o, double v) {
  char b[40];
  const int n = std::snprintf(b, sizeof b, "%g", v);
  o.append(b, (std::size_t)n);
}
void AppendInt(std::string& o, long long v) {
  char b[24];
  const int n = std::snprintf(b, sizeof b, "%lld", v);
  o.append(b, (std::size_t)n);
}

}  // namespace

// One line of the output table (src/PhyloHMM.cpp:288-327), from explicit pieces so that RunPipeline's worker
// threads can format rows side by side.
void PhyloHMM::FormatOutputLine(std::string& o, int iteration, double rb_loglikelihood, double prior, double alpha,
                                const double* er, const double* pi, const std::string& tree, const double* sr,
                                int num_rates, double lh_loglikelihood, const RowSampler& s) const {
  AppendInt(o, iteration);
  o.push_back('\t');
  AppendG(o, rb_loglikelihood);
  o.push_back('\t');
  AppendG(o, prior);
  o.push_back('\t');
  AppendG(o, alpha);
  o.push_back('\t');
  for (int k = 0; k < 6; ++k) AppendG(o, er[k]), o.push_back('\t');
  for (int k = 0; k < 4; ++k) AppendG(o, pi[k]), o.push_back('\t');
  o += tree;
  o.push_back('\t');
  for (int k = 0; k < num_rates; ++k) AppendG(o, sr[k]), o.push_back('\t');
  AppendG(o, lh_loglikelihood);
  o.push_back('\t');
  AppendG(o, lh_loglikelihood - rb_loglikelihood);
  o.push_back('\t');
  AppendAnnotationColumns(o, s);
  o.push_back('\n');
}

void PhyloHMM::AppendAnnotationColumns(std::string& o, const RowSampler& s) const {
  o += s.naive_seq;
  o.push_back('\t');
  o += s.vgerm_state_str;
  o.push_back('\t');
  AppendInt(o, s.vgerm_left_del);
  o.push_back('\t');
  AppendInt(o, s.vgerm_right_del);
  o.push_back('\t');
  o += s.vgerm_left_insertion;
  o.push_back('\t');
  o += s.vd_junction_insertion;
  o.push_back('\t');
  if (locus_ == "igh") {
    o += s.dgerm_state_str;
    o.push_back('\t');
    AppendInt(o, s.dgerm_left_del);
    o.push_back('\t');
    AppendInt(o, s.dgerm_right_del);
    o.push_back('\t');
    o += s.dj_junction_insertion;
    o.push_back('\t');
  }
  o += s.jgerm_state_str;
  o.push_back('\t');
  AppendInt(o, s.jgerm_left_del);
  o.push_back('\t');
  AppendInt(o, s.jgerm_right_del);
  o.push_back('\t');
  o += s.jgerm_right_insertion;
}

std::string PhyloHMM::AnnotationHeader() const {
  std::string h = "NaiveSequence\tVGene\tV5pDel\tV3pDel\tVFwkInsertion\t";
  h += locus_ == "igh" ? "VDInsertion\tDGene\tD5pDel\tD3pDel\tDJInsertion\t" : "VJInsertion\t";
  return h + "JGene\tJ5pDel\tJ3pDel\tJFwkInsertion";
}

// src/PhyloHMM.cpp:288-327
void PhyloHMM::WriteOutputLine(std::ofstream& outfile) const {
  RowSampler s;  // a view of the members the line is made of
  s.naive_seq = naive_sequence_;
  s.vgerm_state_str = vgerm_state_str_samp_;
  s.vgerm_left_del = vgerm_left_del_samp_;
  s.vgerm_right_del = vgerm_right_del_samp_;
  s.vgerm_left_insertion = vgerm_left_insertion_samp_;
  s.vd_junction_insertion = vd_junction_insertion_samp_;
  s.dgerm_state_str = dgerm_state_str_samp_;
  s.dgerm_left_del = dgerm_left_del_samp_;
  s.dgerm_right_del = dgerm_right_del_samp_;
  s.dj_junction_insertion = dj_junction_insertion_samp_;
  s.jgerm_state_str = jgerm_state_str_samp_;
  s.jgerm_left_del = jgerm_left_del_samp_;
  s.jgerm_right_del = jgerm_right_del_samp_;
  s.jgerm_right_insertion = jgerm_right_insertion_samp_;
  std::string line;
  FormatOutputLine(line, iteration_, rb_loglikelihood_, prior_, alpha_, er_.data(), pi_.data(),
                   pending_newick_ ? *pending_newick_ : ExportNewick(tree_, xmsa_labels_), sr_.data(), (int)sr_.size(),
                   lh_loglikelihood_, s);
  outfile << line;
}

namespace {

// One row of the RevBayes table (io::CSVReader<15, trim_chars<>, double_quote_escape<'\t','"'>>,
// src/PhyloHMM.cpp:396-400): tab separated, optional double quotes, extra columns ignored.
std::vector<std::string> SplitTsv(const std::string& line) {
  std::vector<std::string> out;
  std::string cur;
  bool quoted = false;
  for (std::size_t i = 0; i < line.size(); ++i) {
    const char c = line[i];
    if (c == '"') {
      if (quoted && i + 1 < line.size() && line[i + 1] == '"') {
        cur.push_back('"');
        ++i;
      } else {
        quoted = !quoted;
      }
    } else if (c == '\t' && !quoted) {
      out.push_back(cur);
      cur.clear();
    } else if (c != '\r') {
      cur.push_back(c);
    }
  }
  out.push_back(cur);
  return out;
}

}  // namespace

// A RevBayes table held in memory: the rows are located once (no per-field strings) and handed to worker
// threads; a field is converted where it is needed.
// A file's bytes, NUL-terminated, read by several threads into memory that is not cleared first (a 400 MB table:
// 0.03 s instead of 0.10 s for a zero-filled std::string and one fread).
struct FileBytes {
  std::unique_ptr<char[]> data;
  std::size_t n = 0;
  const char* c_str() const { return data.get(); }
  std::size_t size() const { return n; }
  static FileBytes Read(const std::string& path, const char* what) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error(std::string("Can't open ") + what + " " + path);
    struct stat st;
    if (::fstat(fd, &st) != 0) {
      ::close(fd);
      throw std::runtime_error("Can't read " + path);
    }
    FileBytes b;
    if (!S_ISREG(st.st_mode) || st.st_size == 0) {
      // a pipe, a FIFO, /dev/stdin, a process substitution (or a /proc-style file that reports no size): no length to
      // divide among threads -- read to the end into a growing buffer
      std::size_t cap = 1u << 20;
      std::unique_ptr<char[]> buf(new char[cap + 1]);
      for (;;) {
        if (b.n == cap) {
          std::unique_ptr<char[]> more(new char[2 * cap + 1]);
          std::memcpy(more.get(), buf.get(), b.n);
          buf.swap(more);
          cap *= 2;
        }
        const ssize_t got = ::read(fd, buf.get() + b.n, cap - b.n);
        if (got < 0) {
          if (errno == EINTR) continue;
          ::close(fd);
          throw std::runtime_error("Can't read " + path);
        }
        if (got == 0) break;
        b.n += (std::size_t)got;
      }
      ::close(fd);
      buf[b.n] = '\0';
      b.data = std::move(buf);
      return b;
    }
    b.n = (std::size_t)st.st_size;
    b.data.reset(new char[b.n + 1]);
    b.data[b.n] = '\0';
    const int n_threads = b.n < (8u << 20) ? 1 : HostThreads(8);
    std::vector<int> bad(n_threads, 0);
    auto part = [&](int w) {
      std::size_t lo = b.n * w / n_threads;
      const std::size_t hi = b.n * (w + 1) / n_threads;
      while (lo < hi) {
        const ssize_t got = ::pread(fd, b.data.get() + lo, hi - lo, (off_t)lo);
        if (got <= 0) {
          bad[w] = 1;
          return;
        }
        lo += (std::size_t)got;
      }
    };
    if (n_threads == 1) {
      part(0);
    } else {
      std::vector<std::thread> pool;
      for (int w = 0; w < n_threads; ++w) pool.emplace_back(part, w);
      for (std::thread& t : pool) t.join();
    }
    ::close(fd);
    for (int x : bad)
      if (x) throw std::runtime_error("Can't read " + path);
    return b;
  }
};

struct PhyloHMM::TsvTable {
  FileBytes buf;                                          // the file, NUL-terminated
  std::vector<std::pair<std::size_t, std::size_t>> rows;  // data lines: offset and length (empty lines skipped)
  std::vector<std::string> header;
  int col[15];                                            // columns of RunPipeline's fifteen fields

  static TsvTable Read(const std::string& path, const char* what) {
    TsvTable t;
    t.buf = FileBytes::Read(path, what);
    const char* p = t.buf.c_str();
    const std::size_t n = t.buf.size();
    std::size_t pos = 0;
    bool first = true;
    while (pos < n) {
      const char* nl = static_cast<const char*>(std::memchr(p + pos, '\n', n - pos));
      const std::size_t end = nl ? (std::size_t)(nl - p) : n;
      std::size_t len = end - pos;
      if (len && p[pos + len - 1] == '\r') --len;
      if (first) {
        t.header = SplitTsv(std::string(p + pos, len));
        first = false;
      } else if (len) {
        t.rows.push_back({pos, len});
      }
      pos = end + 1;
    }
    if (first) throw std::runtime_error(std::string("Empty ") + what + " " + path);
    return t;
  }

  // a RevBayes output table with the columns of RunPipeline's fifteen fields located
  static TsvTable OpenRevBayesTable(const std::string& path) {
    TsvTable t = Read(path, "RevBayes output file");
    const char* names[15] = {"Iteration", "Likelihood", "Prior", "alpha", "er[1]", "er[2]", "er[3]", "er[4]",
                             "er[5]",     "er[6]",      "pi[1]", "pi[2]", "pi[3]", "pi[4]", "tree"};
    t.Locate(names, 15, t.col, path);
    return t;
  }

  void Locate(const char* const* names, int n, int* out, const std::string& path) const {
    for (int k = 0; k < n; ++k) {
      const auto it = std::find(header.begin(), header.end(), names[k]);
      if (it == header.end()) throw std::runtime_error(std::string("Missing column \"") + names[k] + "\" in " + path);
      out[k] = (int)(it - header.begin());
    }
  }

  // Field boundaries of row r (begin offsets of every field and the end of the row); a quoted field keeps its
  // quotes here and loses them in Field().  `quoted` tells whether the row holds a double quote at all.
  void Split(std::size_t r, std::vector<std::size_t>& starts, bool* quoted) const {
    const char* p = buf.c_str() + rows[r].first;
    const std::size_t len = rows[r].second;
    starts.clear();
    starts.push_back(0);
    *quoted = std::memchr(p, '"', len) != nullptr;
    if (!*quoted) {
      std::size_t pos = 0;
      while (const char* tab = static_cast<const char*>(std::memchr(p + pos, '\t', len - pos))) {
        pos = (std::size_t)(tab - p) + 1;
        starts.push_back(pos);
      }
    } else {
      bool in = false;
      for (std::size_t i = 0; i < len; ++i) {
        if (p[i] == '"')
          in = !in;
        else if (p[i] == '\t' && !in)
          starts.push_back(i + 1);
      }
    }
    starts.push_back(len + 1);
  }
};

namespace {

struct FieldView {
  const char* p;
  std::size_t n;
};

}  // namespace

// The part of FlattenBatch that also reads its rows from the table: rows [r0, r1) are parsed (numbers, tree),
// rooted at naive's neighbour and scheduled by `n_threads` workers straight into the device arrays.
struct PhyloHMM::TableBatch {
  DeviceBatch dev;
  std::vector<int> iteration;
  std::vector<double> lik, prior;
  std::vector<std::string> exported;  // per row: the output table's tree column (with_export)
  std::vector<int32_t> children, root;  // per row: the child lists lh_schedule_tree got and the root (with_children)
};

PhyloHMM::TableBatch PhyloHMM::FlattenTable(const TsvTable& t, std::size_t r0, std::size_t r1, bool with_export,
                                            bool with_scalars, const std::string& path, bool with_children) const {
  const auto t_begin = SteadyNow();
  TableBatch tb;
  DeviceBatch& b = tb.dev;
  const int T = (int)xmsa_labels_.size();
  const std::size_t m = r1 - r0;
  b.n = (int)m;
  b.n_tips = T;
  b.ops.resize(m * (std::size_t)(T - 2) * 4);
  b.brlen.resize(m * (std::size_t)(2 * T - 2));
  b.er.resize(m * 6);
  b.pi.resize(m * 4);
  b.alpha.resize(m);
  if (with_export) tb.exported.resize(m);
  if (with_children) {
    tb.children.resize(m * 2 * (std::size_t)(T - 2));
    tb.root.resize(m);
  }
  if (with_scalars) {
    tb.iteration.resize(m);
    tb.lik.resize(m);
    tb.prior.resize(m);
  }
  const LabelIndex labels(xmsa_labels_);
  auto work = [&](std::size_t lo, std::size_t hi, int* max_depth) {
    NewickScratch scratch;
    std::vector<std::size_t> starts;
    std::vector<int32_t> children(2 * (std::size_t)(T - 2));
    std::string unq;
    for (std::size_t i = lo; i < hi; ++i) {
      bool quoted = false;
      t.Split(r0 + i, starts, &quoted);
      const char* row = t.buf.c_str() + t.rows[r0 + i].first;
      auto field = [&](int k) {
        const int c = t.col[k];
        if (c + 1 >= (int)starts.size()) throw std::runtime_error("Too few columns in " + path);
        FieldView f{row + starts[c], starts[c + 1] - 1 - starts[c]};
        if (quoted && f.n >= 2 && f.p[0] == '"' && f.p[f.n - 1] == '"') f = FieldView{f.p + 1, f.n - 2};
        return f;
      };
      auto number = [&](int k) {
        const FieldView f = field(k);
        const char* end = nullptr;
        const double v = ParseDouble(f.p, &end);
        if (end == f.p || end > f.p + f.n) throw std::runtime_error("Bad number in column \"" + t.header[t.col[k]] + "\" of " + path);
        return v;
      };
      if (with_scalars) {
        tb.iteration[i] = (int)number(0);
        tb.lik[i] = number(1);
        tb.prior[i] = number(2);
      }
      b.alpha[i] = number(3);
      for (int k = 0; k < 6; ++k) b.er[i * 6 + k] = number(4 + k);
      for (int k = 0; k < 4; ++k) b.pi[i * 4 + k] = number(10 + k);
      FieldView tree = field(14);
      if (quoted && std::memchr(tree.p, '"', tree.n)) {  // doubled quotes inside a quoted field (never seen; kept right)
        unq.clear();
        for (std::size_t q = 0; q < tree.n; ++q) {
          unq.push_back(tree.p[q]);
          if (tree.p[q] == '"' && q + 1 < tree.n && tree.p[q + 1] == '"') ++q;
        }
        tree = FieldView{unq.c_str(), unq.size()};
      }
      int32_t root = -1, depth = 0;
      ParseNewickInto(tree.p, tree.n, labels, EPS, scratch, children.data(), &root,
                      b.brlen.data() + i * (std::size_t)(2 * T - 2), with_export ? &tb.exported[i] : nullptr);
      CheckHip(lh_schedule_tree(T, children.data(), root, b.ops.data() + i * (std::size_t)(T - 2) * 4, &depth),
               "lh_schedule_tree");
      if (with_children) {
        std::copy(children.begin(), children.end(), tb.children.begin() + i * children.size());
        tb.root[i] = root;
      }
      *max_depth = std::max(*max_depth, (int)depth);
    }
  };
  const int hw = HostThreads(16);
  const int n_threads = (int)std::max<std::size_t>(1, std::min<std::size_t>(hw, m / 32));
  std::vector<int> depths(n_threads, 0);
  // (an error: the first failing row range, in file order)
  ForRanges(n_threads, m, [&](int w, std::size_t lo, std::size_t hi) { work(lo, hi, &depths[w]); });
  for (int d : depths) b.max_depth = std::max(b.max_depth, d);
  if (host_options().pipeline_timing)
    std::fprintf(stderr, "[FlattenTable] %zu rows on %d threads: %.3f s\n", m, n_threads,
                 Seconds(t_begin, SteadyNow()));
  return tb;
}

PhyloHMM::DeviceBatch PhyloHMM::FlattenTsv(const std::string& path, int* n_rows) const {
  const auto t0 = SteadyNow();
  TsvTable t = TsvTable::Read(path, "RevBayes output file");
  if (host_options().pipeline_timing)
    std::fprintf(stderr, "[FlattenTsv] read + line index %.3f s\n", Seconds(t0, SteadyNow()));
  const char* names[15] = {"alpha", "alpha", "alpha", "alpha", "er[1]", "er[2]", "er[3]", "er[4]",
                           "er[5]", "er[6]",  "pi[1]", "pi[2]", "pi[3]", "pi[4]", "tree"};
  t.Locate(names, 15, t.col, path);
  if (t.rows.empty()) throw std::runtime_error("no rows in table");
  *n_rows = (int)t.rows.size();
  return FlattenTable(t, 0, t.rows.size(), false, false, path).dev;
}

PhyloHMM::DeviceBatch PhyloHMM::FlattenTsvRows(const std::string& path, const int64_t* row_ids, int n, int* n_rows) const {
  TsvTable t = TsvTable::Read(path, "RevBayes output file");
  const char* names[15] = {"alpha", "alpha", "alpha", "alpha", "er[1]", "er[2]", "er[3]", "er[4]",
                           "er[5]", "er[6]",  "pi[1]", "pi[2]", "pi[3]", "pi[4]", "tree"};
  t.Locate(names, 15, t.col, path);
  if (t.rows.empty()) throw std::runtime_error("no rows in table");
  *n_rows = (int)t.rows.size();
  // the line index restricted to the rows asked for: the rest of the table is never parsed
  std::vector<std::pair<std::size_t, std::size_t>> sel((std::size_t)std::max(n, 0));
  for (int i = 0; i < n; ++i) {
    if (row_ids[i] < 0 || (std::size_t)row_ids[i] >= t.rows.size()) throw std::runtime_error("FlattenTsvRows: row outside the table");
    sel[i] = t.rows[(std::size_t)row_ids[i]];
  }
  t.rows.swap(sel);
  if (t.rows.empty()) return DeviceBatch{};
  return FlattenTable(t, 0, t.rows.size(), false, false, path).dev;
}

// src/PhyloHMM.cpp:393-446.  The reference evaluates, samples and writes row by row on one core.  Here the table
// is read once, and per batch of rows: worker threads parse and schedule the trees, the GPU evaluates the batch and
// draws every row's states (lh_eval_sample_batch), and worker threads derive the naive sequences from the states and
// format the output lines, which are written in file order.
// Sampling consumes ONE std::mt19937 stream in file order (src/HMM.cpp:56); a sample takes a fixed number of
// engine outputs (HMM::RawDrawsPerSample), so a row's outputs can be handed to whoever draws for it: the device
// gets them as words[row][...], a host worker that starts at row r copies the engine and skips r samples' worth
// (LH_HOST_SAMPLING=1, or a family whose junction genes do not form two blocks of the state vector).  Every row
// sees exactly the numbers it would see in the serial loop (the host sampler repeats the device's first and last
// row on every run; the seed-0 goldens).  The last row also goes through the object's own members, which are then
// in the state the reference's loop leaves behind.
void PhyloHMM::RunPipeline(const std::string& input_path, const std::string& output_path, int num_rates) {
  const bool timing = host_options().pipeline_timing;
  const auto t_start = SteadyNow();
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t N = table.rows.size();
  const auto t_read = SteadyNow();

  StageTimer stage;
  CreateFamily();
  stage.Mark("CreateFamily");
  EnsureSamplingLists();
  stage.Mark("sampling column lists");
  std::ofstream outfile(output_path);
  if (!outfile) throw std::runtime_error("Can't open output file " + output_path);
  er_.assign(6, 0.0);
  pi_.assign(4, 0.0);
  sr_.assign(num_rates, 0.0);
  num_rates_ = num_rates;
  const std::size_t FS = lh_forward_size(family_), SS = lh_scaler_size(family_);
  const int T = (int)xmsa_labels_.size();
  const int raw_per_sample = RawDrawsPerSample();
  // Sampling on the device when the family has its sampler tables: the forward arrays then never leave the GPU, the
  // host sends each row's slice of the engine's output stream and gets the sampled states back.
  const bool dev_sampling = device_sampler_;
  const std::size_t NS = dev_sampling ? (std::size_t)lh_sample_states(family_) : 0;
  // Two stages, two batches in flight: a producer thread parses / schedules batch k + 1 and has the GPU
  // evaluate it into one of two page-locked result slots while this thread's workers sample and format batch k.
  // Batch size: a sixteenth of the table (the stages overlap batch by batch: few batches mean a long fill and drain),
  // between 2048 rows and 16384 (768 tree samples fill the chip's resident workgroups once; from 8192 on the kernels run
  // at their full-batch rate).
  const std::size_t kBatch = std::min<std::size_t>(std::max<std::size_t>(N, 1), std::min<std::size_t>(16384, std::max<std::size_t>(2048, (N + 15) / 16)));
  struct Slot {
    TableBatch tb;
    double *ll = nullptr, *rates = nullptr, *fwd = nullptr;
    int32_t *sco = nullptr, *states = nullptr;
    std::vector<uint32_t> words;
    std::size_t off = 0, m = 0;
    int state = 0;  // 0 free, 1 filled
  };
  Slot slots[2];
  std::mutex mu;
  std::condition_variable cv;
  std::exception_ptr producer_error;
  bool cancel = false;  // the consumer gave up (error): the producer must not wait for a slot
  double t_flat = 0, t_eval = 0, t_samp = 0, t_write = 0, t_wait = 0;
  auto alloc_slot = [&](Slot& s) {
    s.ll = static_cast<double*>(lh_host_alloc(sizeof(double) * kBatch));
    s.rates = static_cast<double*>(lh_host_alloc(sizeof(double) * kBatch * num_rates));
    // device sampling keeps forward arrays for two rows only: the table's first (cross-check) and last (members)
    const std::size_t fwd_rows = dev_sampling ? 2 : kBatch;
    s.fwd = static_cast<double*>(lh_host_alloc(sizeof(double) * fwd_rows * FS));
    s.sco = static_cast<int32_t*>(lh_host_alloc(sizeof(int32_t) * fwd_rows * SS));
    if (dev_sampling) s.states = static_cast<int32_t*>(lh_host_alloc(sizeof(int32_t) * kBatch * NS));
    if (!s.ll || !s.rates || !s.fwd || !s.sco || (dev_sampling && !s.states)) throw std::runtime_error(lh_last_error());
  };
  auto free_slots = [&] {
    for (Slot& s : slots) {
      lh_host_free(s.ll);
      lh_host_free(s.rates);
      lh_host_free(s.fwd);
      lh_host_free(s.sco);
      lh_host_free(s.states);
    }
  };
  double t_words = 0;
  // Stage 0: a parser thread turns the next batches of rows into device arrays (worker threads inside FlattenTable) and
  // keeps at most two of them waiting, so that parsing batch k + 1 overlaps the device's work on batch k.
  std::deque<TableBatch> parsed;
  bool parser_done = false;
  std::thread parser([&] {
    try {
      for (std::size_t off = 0; off < N; off += kBatch) {
        const std::size_t m = std::min(kBatch, N - off);
        const auto t0 = SteadyNow();
        TableBatch tb = FlattenTable(table, off, off + m, true, true, input_path);
        t_flat += Seconds(t0, SteadyNow());
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return parsed.size() < 2 || cancel; });
        if (cancel) return;
        parsed.push_back(std::move(tb));
        cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lock(mu);
      if (!producer_error) producer_error = std::current_exception();
    }
    std::lock_guard<std::mutex> lock(mu);
    parser_done = true;
    cv.notify_all();
  });
  // The device sampler's random words: one engine stream in file order (a copy of rng_ that just runs on), drawn by a
  // thread of its own, at most two batches ahead of the producer.
  std::deque<std::vector<uint32_t>> drawn;
  std::thread drawer([&] {
    if (!dev_sampling) return;
    try {
      std::mt19937 word_rng = rng_;
      for (std::size_t off = 0; off < N; off += kBatch) {
        const std::size_t m = std::min(kBatch, N - off);
        const auto t0 = SteadyNow();
        std::vector<uint32_t> w(m * (std::size_t)raw_per_sample);
        for (uint32_t& x : w) x = (uint32_t)word_rng();
        t_words += Seconds(t0, SteadyNow());
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return drawn.size() < 2 || cancel; });
        if (cancel) return;
        drawn.push_back(std::move(w));
        cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lock(mu);
      if (!producer_error) producer_error = std::current_exception();
      cv.notify_all();
    }
  });
  std::thread producer([&] {
    try {
      int k = 0;
      for (std::size_t off = 0; off < N; off += kBatch, k ^= 1) {
        Slot& s = slots[k];
        const std::size_t m = std::min(kBatch, N - off);
        TableBatch tb;
        {
          std::unique_lock<std::mutex> lock(mu);
          cv.wait(lock, [&] { return !parsed.empty() || parser_done || cancel || producer_error; });
          if (cancel || producer_error || parsed.empty()) return;  // (an empty queue with the parser gone: it failed)
          tb = std::move(parsed.front());
          parsed.pop_front();
          cv.notify_all();
        }
        {
          std::unique_lock<std::mutex> lock(mu);
          cv.wait(lock, [&] { return s.state == 0 || cancel; });
          if (cancel) return;
        }
        if (!s.ll) alloc_slot(s);
        s.tb = std::move(tb);
        s.off = off;
        s.m = m;
        const DeviceBatch& b = s.tb.dev;
        const auto t2 = SteadyNow();
        if (dev_sampling) {
          {
            std::unique_lock<std::mutex> lock(mu);
            cv.wait(lock, [&] { return !drawn.empty() || cancel || producer_error; });
            if (cancel || producer_error) return;
            s.words = std::move(drawn.front());
            drawn.pop_front();
            cv.notify_all();
          }
          if (more_families_.empty()) {
            CheckHip(lh_eval_sample_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                          b.pi.data(), b.alpha.data(), num_rates, s.words.data(), s.ll, s.rates, s.states),
                     "lh_eval_sample_batch");
          } else {
            // Several devices: table row i goes to device i mod N.  One host thread per device gathers its rows of
            // the batch, has its handle evaluate and sample them, and puts the results back at the rows' places
            // (host memory, in-process: no collective; RCCL only joins separate processes, bench.py --gpus N).
            const std::size_t D = 1 + more_families_.size();
            const std::size_t n_ops4 = (std::size_t)(b.n_tips - 2) * 4, nodes = 2 * (std::size_t)b.n_tips - 2;
            const std::size_t W = (std::size_t)raw_per_sample;
            ForRanges((int)D, D, [&](int w, std::size_t, std::size_t) {  // (D >= 2: one thread per device)
              const std::size_t d = (std::size_t)w;
              std::vector<std::size_t> idx;
              for (std::size_t i = 0; i < m; ++i)
                if ((off + i) % D == d) idx.push_back(i);
              const std::size_t q = idx.size();
              if (q == 0) return;
              std::vector<int32_t> ops(q * n_ops4), states(q * NS);
              std::vector<double> brlen(q * nodes), er(q * 6), pi(q * 4), alpha(q), ll(q), rates(q * (std::size_t)num_rates);
              std::vector<uint32_t> words(q * W);
              for (std::size_t j = 0; j < q; ++j) {
                const std::size_t i = idx[j];
                std::copy_n(b.ops.data() + i * n_ops4, n_ops4, ops.data() + j * n_ops4);
                std::copy_n(b.brlen.data() + i * nodes, nodes, brlen.data() + j * nodes);
                std::copy_n(b.er.data() + i * 6, 6, er.data() + j * 6);
                std::copy_n(b.pi.data() + i * 4, 4, pi.data() + j * 4);
                alpha[j] = b.alpha[i];
                std::copy_n(s.words.data() + i * W, W, words.data() + j * W);
              }
              lh_family* fam = d == 0 ? family_ : more_families_[d - 1];
              if (lh_eval_sample_batch(fam, (int32_t)q, b.n_tips, b.max_depth, ops.data(), brlen.data(), er.data(), pi.data(),
                                       alpha.data(), num_rates, words.data(), ll.data(), rates.data(), states.data()))
                throw std::runtime_error(std::string("lh_eval_sample_batch: ") + lh_last_error());
              for (std::size_t j = 0; j < q; ++j) {
                const std::size_t i = idx[j];
                s.ll[i] = ll[j];
                std::copy_n(rates.data() + j * (std::size_t)num_rates, (std::size_t)num_rates, s.rates + i * (std::size_t)num_rates);
                std::copy_n(states.data() + j * NS, NS, s.states + i * NS);
              }
            });
          }
          auto one_row = [&](std::size_t i, int k_fwd) {  // forward arrays of one row, for the host-side checks
            const std::size_t n_ops = (std::size_t)(b.n_tips - 2) * 4, nodes = 2 * (std::size_t)b.n_tips - 2;
            double ll1 = 0;
            lh_eval_outputs outs{nullptr, nullptr, s.fwd + k_fwd * FS, s.sco + k_fwd * SS};
            CheckHip(lh_eval_batch(family_, 1, b.n_tips, b.max_depth, b.ops.data() + i * n_ops, b.brlen.data() + i * nodes,
                                   b.er.data() + i * 6, b.pi.data() + i * 4, b.alpha.data() + i, num_rates, &ll1, &outs),
                     "lh_eval_batch");
          };
          if (off == 0) one_row(0, 0);
          if (off + m == N) one_row(m - 1, 1);
        } else {
          lh_eval_outputs outs{s.rates, nullptr, s.fwd, s.sco};
          CheckHip(lh_eval_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                 b.pi.data(), b.alpha.data(), num_rates, s.ll, &outs),
                   "lh_eval_batch");
        }
        const auto t3 = SteadyNow();
        t_eval += Seconds(t2, t3);
        {
          std::lock_guard<std::mutex> lock(mu);
          s.state = 1;
        }
        cv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> lock(mu);
      producer_error = std::current_exception();
      cv.notify_all();
    }
  });
  struct Joiner {  // the three threads are stopped, joined and the slots are freed on every way out
    std::thread &t, &t0, &t1;
    std::function<void()> before, after;
    ~Joiner() {
      before();
      if (t0.joinable()) t0.join();
      if (t1.joinable()) t1.join();
      if (t.joinable()) t.join();
      after();
    }
  } joiner{producer, parser, drawer,
           [&] {
             {
               std::lock_guard<std::mutex> lock(mu);
               cancel = true;
             }
             cv.notify_all();
           },
           free_slots};

  bool header_written = false;
  int k = 0;
  for (std::size_t off = 0; off < N; off += kBatch, k ^= 1) {
    Slot& slot = slots[k];
    const auto tw = SteadyNow();
    {
      std::unique_lock<std::mutex> lock(mu);
      cv.wait(lock, [&] { return slot.state == 1 || producer_error; });
      if (producer_error) std::rethrow_exception(producer_error);
    }
    const std::size_t m = slot.m;
    const TableBatch& tb = slot.tb;
    const DeviceBatch& b = tb.dev;
    const double *ll = slot.ll, *rates = slot.rates, *fwd = slot.fwd;
    const int32_t* sco = slot.sco;
    const auto t2 = SteadyNow();
    t_wait += Seconds(tw, t2);
    // rows of this batch except the table's very last one: sampled and formatted by the workers
    const std::size_t m_par = (off + m == N) ? m - 1 : m;
    const int hw = HostThreads(16);
    const int n_threads = (int)std::max<std::size_t>(1, std::min<std::size_t>(hw, m_par / 8));
    std::vector<std::string> chunks(n_threads);
    auto sample_rows = [&](int w, std::size_t lo, std::size_t hi) {
      RowSampler s;
      std::mt19937 rng = rng_;
      if (!dev_sampling) rng.discard((unsigned long long)(off + lo) * (unsigned long long)raw_per_sample);
      std::string& o = chunks[w];
      o.reserve((hi - lo) * (tb.exported.empty() ? 512 : tb.exported[lo].size() + 1024));
      for (std::size_t i = lo; i < hi; ++i) {
        if (dev_sampling) {
          ApplySampledStates(s, slot.states + i * NS);
          if (off + i == 0) {  // the device's draws against the host sampler's, where it is cheap
            RowSampler h;
            SampleRow(h, fwd, rng);
            if (h.naive_seq != s.naive_seq || h.vd_junction_state_inds != s.vd_junction_state_inds ||
                h.dj_junction_state_inds != s.dj_junction_state_inds || h.vgerm_state_ind != s.vgerm_state_ind ||
                h.dgerm_state_ind != s.dgerm_state_ind || h.jgerm_state_ind != s.jgerm_state_ind)
              throw std::runtime_error("RunPipeline: the device sampler and the host sampler disagree on the first row");
          }
        } else if (off + i == 0) {  // the bookkeeping above rests on this count: check it where it is cheap
          std::mt19937 expect = rng;
          SampleRow(s, fwd + i * FS, rng);
          expect.discard((unsigned long long)raw_per_sample);
          if (!(expect == rng)) throw std::runtime_error("RunPipeline: a sample consumed an unexpected number of random numbers");
        } else {
          SampleRow(s, fwd + i * FS, rng);
        }
        FormatOutputLine(o, tb.iteration[i], tb.lik[i], tb.prior[i], b.alpha[i], b.er.data() + i * 6,
                         b.pi.data() + i * 4, tb.exported[i], rates + i * num_rates, num_rates, ll[i], s);
      }
    };
    ForRanges(n_threads, m_par, sample_rows);
    const auto t3 = SteadyNow();
    if (!header_written) {
      WriteOutputHeaders(outfile);
      header_written = true;
    }
    for (const std::string& c : chunks) outfile.write(c.data(), (std::streamsize)c.size());
    if (m_par < m) {
      // the last row of the table, through the members (as every row goes in the reference)
      const std::size_t i = m - 1;
      // (with device sampling the forward arrays of this row sit in the slot's second place)
      const double* fwd_i = dev_sampling ? slot.fwd + FS : fwd + i * FS;
      const int32_t* sco_i = dev_sampling ? slot.sco + SS : sco + i * SS;
      rng_.discard((unsigned long long)(N - 1) * (unsigned long long)raw_per_sample);
      iteration_ = tb.iteration[i];
      rb_loglikelihood_ = tb.lik[i];
      prior_ = tb.prior[i];
      alpha_ = b.alpha[i];
      er_.assign(b.er.begin() + i * 6, b.er.begin() + (i + 1) * 6);
      pi_.assign(b.pi.begin() + i * 4, b.pi.begin() + (i + 1) * 4);
      {  // the tree's arrays again (the batch keeps schedules, not child lists)
        const std::pair<std::size_t, std::size_t> row = table.rows[off + i];
        std::vector<std::size_t> starts;
        bool quoted = false;
        table.Split(off + i, starts, &quoted);
        const int c = table.col[14];
        std::string text(table.buf.c_str() + row.first + starts[c], starts[c + 1] - 1 - starts[c]);
        if (quoted) text = SplitTsv(std::string(table.buf.c_str() + row.first, row.second)).at(c);
        tree_ = ParseNewick(text, xmsa_labels_, EPS, true);
      }
      have_tree_ = true;
      pending_newick_ = &tb.exported[i];
      sr_.assign(rates + i * num_rates, rates + (i + 1) * num_rates);
      pending_forward_.assign(fwd_i, fwd_i + FS);
      pending_scalers_.assign(sco_i, sco_i + SS);
      pending_loglik_ = ll[i];
      cache_forward_ = true;
      lh_loglikelihood_ = LogLikelihood();
      logweight_ = lh_loglikelihood_ - rb_loglikelihood_;
      naive_sequence_ = SampleNaiveSequence();
      if (dev_sampling) {
        RowSampler d;
        ApplySampledStates(d, slot.states + i * NS);
        if (d.naive_seq != naive_sequence_)
          throw std::runtime_error("RunPipeline: the device sampler and the host sampler disagree on the last row");
      }
      WriteOutputLine(outfile);
      pending_newick_ = nullptr;
    }
    const auto t4 = SteadyNow();
    t_samp += Seconds(t2, t3);
    t_write += Seconds(t3, t4);
    {
      std::lock_guard<std::mutex> lock(mu);
      slot.state = 0;
    }
    cv.notify_all();
  }
  (void)T;
  outfile.close();
  if (timing)
    std::fprintf(stderr,
                 "[RunPipeline] %zu rows: read %.3f s; producer: parse+schedule %.3f s, device (incl. copies%s) %.3f s; "
                 "consumer (%s): waiting %.3f s, sample+format %.3f s, write %.3f s; total %.3f s\n",
                 N, Seconds(t_start, t_read), t_flat, dev_sampling ? (", engine words " + std::to_string(t_words) + " s").c_str() : "",
                 t_eval, dev_sampling ? "device sampler" : "host sampler", t_wait, t_samp,
                 t_write, Seconds(t_start, SteadyNow()));
}

// scripts/run_bootstrap_asr_ess.R:86-101: the tree rooted on the naive branch (the added root node sits at
// distance 0 from naive's neighbour, :53), every node followed by [&ancestral="..."] as
// phylotate::print_annotated writes node comments.  Branch lengths "%.10g" (R's own formatting of doubles is
// not restated).
std::string PhyloHMM::AnnotatedNewick(const TreeArrays& tr, const std::string& naive_sequence,
                                      const uint8_t* anc) const {
  const int T = tr.n_tips;
  const int L = (int)msa_.cols();
  auto comment = [&](int v) {
    std::string s = "[&ancestral=\"";
    if (v == 0) {
      s += naive_sequence;
    } else if (v < T) {
      for (int j = 0; j < L; ++j) s.push_back(alphabet_[msa_(v - 1, j)]);
    } else {
      s += DecodeBases(anc + (std::size_t)(v - T) * L, (std::size_t)L, alphabet_);
    }
    return s + "\"]";
  };
  auto len = [](double l) {
    char b[48];
    std::snprintf(b, sizeof b, ":%.10g", l);
    return std::string(b);
  };
  std::string out;
  struct Fr {
    int node, next_kid;
  };
  std::vector<Fr> stack{{tr.root, 0}};
  out = "(" + xmsa_labels_[0] + comment(0) + len(tr.brlen[0]) + ",";
  while (!stack.empty()) {
    Fr& f = stack.back();
    if (f.node < T) {
      out += xmsa_labels_[f.node] + comment(f.node) + len(tr.brlen[f.node]);
      stack.pop_back();
      continue;
    }
    if (f.next_kid < 2) {
      out.push_back(f.next_kid == 0 ? '(' : ',');
      const int k = tr.children[2 * (std::size_t)(f.node - T) + f.next_kid++];
      stack.push_back({k, 0});
      continue;
    }
    out += ")" + comment(f.node) + len(f.node == tr.root ? 0.0 : tr.brlen[f.node]);
    stack.pop_back();
  }
  return out + ")" + comment(tr.root) + ";";
}

struct PhyloHMM::AsrRow {
  TreeSample ts;
  std::vector<double> sr;
  std::string naive;
};

std::vector<PhyloHMM::AsrRow> PhyloHMM::ReadAsrRows(const std::string& input_path, int* num_rates) const {
  std::ifstream in(input_path);
  if (!in) throw std::runtime_error("Can't open linearham output file " + input_path);
  std::string line;
  if (!std::getline(in, line)) throw std::runtime_error("Empty linearham output file " + input_path);
  const std::vector<std::string> header = SplitTsv(line);
  auto find = [&](const std::string& name) {
    const auto it = std::find(header.begin(), header.end(), name);
    return it == header.end() ? -1 : (int)(it - header.begin());
  };
  std::vector<int> col;
  for (int k = 1; k <= 6; ++k) col.push_back(find("er[" + std::to_string(k) + "]"));
  for (int k = 1; k <= 4; ++k) col.push_back(find("pi[" + std::to_string(k) + "]"));
  col.push_back(find("tree"));
  col.push_back(find("NaiveSequence"));
  const char* names[12] = {"er[1]", "er[2]", "er[3]", "er[4]", "er[5]", "er[6]", "pi[1]", "pi[2]", "pi[3]", "pi[4]",
                           "tree",  "NaiveSequence"};
  for (int k = 0; k < 12; ++k)
    if (col[k] < 0) throw std::runtime_error(std::string("Missing column \"") + names[k] + "\" in " + input_path);
  std::vector<int> sr_col;
  for (int k = 1;; ++k) {
    const int c = find("sr[" + std::to_string(k) + "]");
    if (c < 0) break;
    sr_col.push_back(c);
  }
  if (sr_col.empty()) throw std::runtime_error("Missing column \"sr[1]\" in " + input_path);
  *num_rates = (int)sr_col.size();
  const int L = (int)msa_.cols();
  std::vector<AsrRow> rows;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    const std::vector<std::string> f = SplitTsv(line);
    auto get = [&](int c) -> const std::string& {
      if (c >= (int)f.size()) throw std::runtime_error("Too few columns in " + input_path);
      return f[c];
    };
    AsrRow r;
    for (int k = 0; k < 6; ++k) r.ts.er.push_back(std::stod(get(col[k])));
    for (int k = 0; k < 4; ++k) r.ts.pi.push_back(std::stod(get(col[6 + k])));
    r.ts.alpha = 1.0;  // unused: the rates come from the sr[] columns
    r.ts.newick = get(col[10]);
    r.naive = get(col[11]);
    if ((int)r.naive.size() != L) throw std::runtime_error("NaiveSequence length differs from the alignment's in " + input_path);
    for (int c : sr_col) r.sr.push_back(std::stod(get(c)));
    rows.push_back(std::move(r));
  }
  return rows;
}

void PhyloHMM::EncodeAsrRows(const std::vector<AsrRow>& rows, std::size_t off, std::size_t m, int R,
                             std::vector<TreeSample>* samples, std::vector<double>* rates,
                             std::vector<uint8_t>* naive) const {
  const int L = (int)msa_.cols();
  samples->clear();
  for (std::size_t i = 0; i < m; ++i) samples->push_back(rows[off + i].ts);
  rates->assign(m * R, 0.0);
  naive->assign(m * (std::size_t)L, 0);
  for (std::size_t i = 0; i < m; ++i) {
    std::copy(rows[off + i].sr.begin(), rows[off + i].sr.end(), rates->begin() + i * R);
    for (int j = 0; j < L; ++j) {
      const std::size_t a = alphabet_.find(rows[off + i].naive[j]);
      if (a == std::string::npos) throw std::runtime_error("NaiveSequence holds a character outside the alphabet");
      (*naive)[i * L + j] = (uint8_t)a;
    }
  }
}

void PhyloHMM::RunAsr(const std::string& input_path, const std::string& output_path, uint64_t seed) {
  int R = 0;
  const std::vector<AsrRow> rows = ReadAsrRows(input_path, &R);
  const int L = (int)msa_.cols();
  CreateFamily();
  std::ofstream outfile(output_path);
  if (!outfile) throw std::runtime_error("Can't open output file " + output_path);
  const int T = (int)xmsa_labels_.size();
  const std::size_t kBatch = 1024;
  for (std::size_t off = 0; off < rows.size(); off += kBatch) {
    const std::size_t m = std::min(kBatch, rows.size() - off);
    std::vector<TreeSample> samples;
    std::vector<double> rates;
    std::vector<uint8_t> naive, anc(m * (std::size_t)(T - 2) * L);
    EncodeAsrRows(rows, off, m, R, &samples, &rates, &naive);
    std::vector<TreeArrays> trees;
    const DeviceBatch b = FlattenBatch(samples, &trees);
    CheckHip(lh_asr_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(), b.pi.data(),
                          rates.data(), R, naive.data(), seed, (uint64_t)off, anc.data(), nullptr),
             "lh_asr_batch");
    // the annotated strings (86 KB per tree for 100 leaves x 400 sites) are most of this step's host time:
    // rows are formatted by several threads, written in order
    std::vector<std::string> lines(m);
    const int hw = HostThreads(16);
    const int n_threads = std::max(1, std::min(hw, (int)(m / 16)));
    ForRanges(n_threads, m, [&](int, std::size_t lo, std::size_t hi) {
      for (std::size_t i = lo; i < hi; ++i)
        lines[i] = AnnotatedNewick(trees[i], rows[off + i].naive, anc.data() + i * (std::size_t)(T - 2) * L);
    });
    for (std::size_t i = 0; i < m; ++i) outfile << lines[i] << "\n";
  }
}

void PhyloHMM::RunLineagePipeline(const std::string& input_path, const std::string& seed_seq,
                                  const std::string& output_prefix, uint64_t seed) {
  Require(seed_seq != "naive", "the seed sequence cannot be 'naive': the lineage ends there");
  const int T = (int)xmsa_labels_.size();
  int seed_tip = -1;
  for (int v = 1; v < T; ++v)
    if (xmsa_labels_[v] == seed_seq) seed_tip = v;
  Require(seed_tip > 0, "the seed sequence '" + seed_seq + "' is not a sequence of this clonal family");
  const bool timing = host_options().pipeline_timing;
  const auto t_start = SteadyNow();
  double t_flat = 0, t_dev = 0, t_resolve = 0, t_count = 0;
  int R = 0;
  const std::vector<AsrRow> rows = ReadAsrRows(input_path, &R);
  const auto t_read = SteadyNow();
  const int L = (int)msa_.cols();
  CreateFamily();
  CheckHip(lh_lineage_reset(family_), "lh_lineage_reset");
  LineageTabulator tab;
  std::string seed_nt((std::size_t)L, 'N');
  for (int j = 0; j < L; ++j) seed_nt[j] = alphabet_[msa_(seed_tip - 1, j)];
  const int seed_id = tab.AddSequence(seed_nt);  // (tips keep their observed characters: one sequence for every tree)
  SeqInterner interner(family_, lh_lineage_resolve, lh_lineage_rows_read, L, "lineage pipeline");  // by base hash
  std::vector<int> tab_of_store;      // store id -> tabulator id
  std::vector<uint64_t> aa_of_store;  // store id -> translation hash of its first slot
  const std::size_t kBatch = host_options().lineage_batch > 0 ? (std::size_t)host_options().lineage_batch : 1024;
  for (std::size_t off = 0; off < rows.size(); off += kBatch) {
    const std::size_t m = std::min(kBatch, rows.size() - off);
    const auto t0 = SteadyNow();
    std::vector<TreeSample> samples;
    std::vector<double> rates;
    std::vector<uint8_t> naive;
    EncodeAsrRows(rows, off, m, R, &samples, &rates, &naive);
    std::vector<TreeArrays> trees;
    const DeviceBatch b = FlattenBatch(samples, &trees);
    // the seed tip's ancestors up to naive's neighbour
    std::vector<std::vector<int32_t>> chain(m);
    std::size_t P = 1;
    for (std::size_t i = 0; i < m; ++i) {
      chain[i] = SeedPath(trees[i].children.data(), T, trees[i].root, seed_tip);
      Require(!chain[i].empty(),
              "row " + std::to_string(off + i) + ": the seed sequence '" + seed_seq + "' does not descend from the root");
      P = std::max(P, chain[i].size());
    }
    std::vector<int32_t> path(m * P, -1);
    for (std::size_t i = 0; i < m; ++i) std::copy(chain[i].begin(), chain[i].end(), path.begin() + i * P);
    const std::size_t S = P + 1;
    std::vector<uint64_t> nt_hash(m * S), aa_hash(m * S);
    const auto t1 = SteadyNow();
    CheckHip(lh_lineage_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(), b.pi.data(),
                              rates.data(), R, naive.data(), seed, (uint64_t)off, path.data(), (int32_t)P,
                              nt_hash.data(), aa_hash.data()),
             "lh_lineage_batch");
    const auto t2 = SteadyNow();
    // every slot but the padding ones takes part
    std::vector<uint8_t> take(m * S, 1);
    for (std::size_t i = 0; i < m; ++i) std::fill(take.begin() + i * S + chain[i].size(), take.begin() + i * S + P, 0);
    std::vector<int32_t> ids(m * S);
    const int32_t K_before = interner.K();
    const int32_t K = K_before + interner.Assign(m * S, nt_hash.data(), take.data(), ids.data());
    std::vector<uint8_t> bytes;
    // only the bases of the sequences first seen in this batch come back
    if (K > K_before) {
      bytes.resize((std::size_t)(K - K_before) * L);
      CheckHip(lh_lineage_store_read(family_, K_before, K - K_before, nullptr, bytes.data()), "lh_lineage_store_read");
      for (int32_t k = K_before; k < K; ++k)
        tab_of_store.push_back(tab.AddSequence(DecodeBases(bytes.data() + (std::size_t)(k - K_before) * L, (std::size_t)L, alphabet_)));
      aa_of_store.resize(K);
      std::vector<bool> have(K - K_before, false);
      for (std::size_t x = 0; x < m * S; ++x)
        if (ids[x] >= K_before && !have[ids[x] - K_before]) {
          have[ids[x] - K_before] = true;
          aa_of_store[ids[x]] = aa_hash[x];
        }
    }
    const auto t3 = SteadyNow();
    std::vector<int> l;
    for (std::size_t i = 0; i < m; ++i) {
      for (std::size_t s = 0; s < S; ++s)
        if (ids[i * S + s] >= 0)
          Require(aa_hash[i * S + s] == aa_of_store[ids[i * S + s]],
                  "lineage pipeline: equal sequences with different translation hashes at row " + std::to_string(off + i));
      l.clear();
      l.push_back(tab_of_store[ids[i * S + P]]);
      for (std::size_t s = chain[i].size(); s-- > 0;) l.push_back(tab_of_store[ids[i * S + s]]);
      l.push_back(seed_id);
      tab.AddTree(l, (int)chain[i].size());
    }
    const auto t4 = SteadyNow();
    t_flat += Seconds(t0, t1);
    t_dev += Seconds(t1, t2);
    t_resolve += Seconds(t2, t3);
    t_count += Seconds(t3, t4);
  }
  const auto t_w = SteadyNow();
  WriteLineageFiles(output_prefix, tab.Finish(seed_seq), interner.collisions());
  if (timing)
    std::fprintf(stderr,
                 "[RunLineagePipeline] %zu rows: read %.3f s, parse+schedule+paths %.3f s, device (K1 + K3 + K7, copies) "
                 "%.3f s, resolve+read back (%d sequences) %.3f s, count %.3f s, write %.3f s; total %.3f s\n",
                 rows.size(), Seconds(t_start, t_read), t_flat, t_dev, (int)interner.K(), t_resolve, t_count, Seconds(t_w, SteadyNow()),
                 Seconds(t_start, SteadyNow()));
}

// The weighted lineage tables in one pass over the RevBayes table.  Per batch the chain lh_eval_lineage_batch evaluates the
// rows, draws each row's naive sequence from RunPipeline's std::mt19937 words, draws `draws_per_row` sets of ancestral
// sequences (Philox stream `seed`, sample number = table row, draw d in the upper half) and hashes the lineage slots; the
// host interns the sequences as RunLineagePipeline does.  A tree's weight needs the largest log-weight of the table, so
// the batches' id lists are kept and counted after the last batch: the result does not depend on the batch size.
void PhyloHMM::RunWeightedLineagePipeline(const std::string& input_path, const std::string& seed_seq,
                                          const std::string& output_prefix, int num_rates, double burnin_frac,
                                          int draws_per_row, uint64_t seed) {
  Require(devices_.size() <= 1, "the weighted lineage pipeline runs on one device: --devices may list only one");
  Require(burnin_frac >= 0.0 && burnin_frac < 1.0, "burn-in fraction must be in [0, 1)");
  Require(draws_per_row >= 1 && draws_per_row <= 64, "draws-per-row must be in 1 .. 64");
  Require(seed_seq != "naive", "the seed sequence cannot be 'naive': the lineage ends there");
  const int T = (int)xmsa_labels_.size();
  int seed_tip = -1;
  for (int v = 1; v < T; ++v)
    if (xmsa_labels_[v] == seed_seq) seed_tip = v;
  Require(seed_tip > 0, "the seed sequence '" + seed_seq + "' is not a sequence of this clonal family");
  CreateFamily();
  Require(device_sampler_, "the weighted lineage pipeline draws the naive sequences on the device: this family has no "
                           "device sampler tables (or LH_HOST_SAMPLING is set)");
  const bool timing = host_options().pipeline_timing;
  const auto t_start = SteadyNow();
  double t_flat = 0, t_dev = 0, t_resolve = 0;
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t N = table.rows.size();
  const std::size_t first = (std::size_t)std::floor(burnin_frac * (double)N);
  const std::size_t U = N - first;  // rows after the burn-in
  const std::size_t D = (std::size_t)draws_per_row;
  const int L = (int)msa_.cols();
  // the id lists of every (row, draw) wait for the last batch: at most T ids each; 1 GiB of them is the limit
  const std::size_t kHeldLimit = (std::size_t)1 << 30;
  Require(U * D * (std::size_t)T * sizeof(int32_t) <= kHeldLimit,
          "weighted lineage pipeline: " + std::to_string(U) + " rows x " + std::to_string(D) + " draws x " + std::to_string(T) +
              " lineage nodes exceed the 1 GiB the pipeline keeps until the weights are known; at most " +
              std::to_string(kHeldLimit / (D * (std::size_t)T * sizeof(int32_t))) + " rows for this family and draws-per-row");
  const auto t_read = SteadyNow();
  CheckHip(lh_lineage_reset(family_), "lh_lineage_reset");
  LineageTabulator tab;
  tab.SetWeighted();
  std::string seed_nt((std::size_t)L, 'N');
  for (int j = 0; j < L; ++j) seed_nt[j] = alphabet_[msa_(seed_tip - 1, j)];
  const int seed_id = tab.AddSequence(seed_nt);  // (tips keep their observed characters: one sequence for every tree)
  SeqInterner interner(family_, lh_lineage_resolve, lh_lineage_rows_read, L, "weighted lineage pipeline");
  std::vector<int> tab_of_store;      // store id -> tabulator id
  std::vector<uint64_t> aa_of_store;  // store id -> translation hash of its first slot
  const int raw = RawDrawsPerSample();
  std::mt19937 word_rng = rng_;
  word_rng.discard((unsigned long long)first * (unsigned long long)raw);
  std::vector<double> ll(U), lw(U);
  std::vector<int32_t> path_len(U, 0), naive_tab(U, -1);
  std::vector<int32_t> held;              // per used (row, draw): naive, root .. seed's parent (tabulator ids)
  std::vector<std::size_t> held_at(U + 1, 0);  // row -> its first entry in held (D lists of path_len + 1 ids)
  const std::size_t kBatch = host_options().lineage_batch > 0 ? (std::size_t)host_options().lineage_batch : 1024;
  for (std::size_t off = first; off < N; off += kBatch) {
    const std::size_t m = std::min(kBatch, N - off);
    const auto t0 = SteadyNow();
    TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path, true);
    const DeviceBatch& b = tb.dev;
    // the seed tip's ancestors up to naive's neighbour
    std::vector<std::vector<int32_t>> chain(m);
    std::size_t P = 1;
    for (std::size_t i = 0; i < m; ++i) {
      chain[i] = SeedPath(tb.children.data() + i * 2 * (std::size_t)(T - 2), T, tb.root[i], seed_tip);
      Require(!chain[i].empty(),
              "row " + std::to_string(off + i) + ": the seed sequence '" + seed_seq + "' does not descend from the root");
      P = std::max(P, chain[i].size());
    }
    std::vector<int32_t> path(m * P, -1);
    for (std::size_t i = 0; i < m; ++i) std::copy(chain[i].begin(), chain[i].end(), path.begin() + i * P);
    const std::size_t S = P + 1;
    std::vector<uint32_t> words(m * (std::size_t)raw);
    for (uint32_t& x : words) x = (uint32_t)word_rng();
    std::vector<uint64_t> nt_hash(m * D * S), aa_hash(m * D * S);
    double* ll_b = ll.data() + (off - first);
    lh_lineage_eval_outputs outs{};
    outs.loglik = ll_b;
    outs.nt_hash = nt_hash.data();
    outs.aa_hash = aa_hash.data();
    const auto t1 = SteadyNow();
    CheckHip(lh_eval_lineage_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                   b.pi.data(), b.alpha.data(), num_rates, words.data(), seed, (uint64_t)off,
                                   draws_per_row, path.data(), (int32_t)P, &outs),
             "lh_eval_lineage_batch");
    const auto t2 = SteadyNow();
    // every slot of a used row but the padding ones takes part
    std::vector<uint8_t> take(m * D * S, 0);
    for (std::size_t i = 0; i < m; ++i) {
      const std::size_t u = off - first + i;
      lw[u] = ll_b[i] - tb.lik[i];
      path_len[u] = (int32_t)chain[i].size();
      if (!std::isfinite(lw[u])) continue;
      for (std::size_t d = 0; d < D; ++d) {
        uint8_t* tk = take.data() + (i * D + d) * S;
        std::fill(tk, tk + chain[i].size(), 1);
        tk[P] = 1;
      }
    }
    std::vector<int32_t> ids(m * D * S);
    const int32_t K_before = interner.K();
    const int32_t K = K_before + interner.Assign(m * D * S, nt_hash.data(), take.data(), ids.data());
    if (K > K_before) {  // only the bases of the sequences first seen in this batch come back
      std::vector<uint8_t> bytes((std::size_t)(K - K_before) * L);
      CheckHip(lh_lineage_store_read(family_, K_before, K - K_before, nullptr, bytes.data()), "lh_lineage_store_read");
      for (int32_t k = K_before; k < K; ++k)
        tab_of_store.push_back(tab.AddSequence(DecodeBases(bytes.data() + (std::size_t)(k - K_before) * L, (std::size_t)L, alphabet_)));
      aa_of_store.resize(K);
      std::vector<bool> have(K - K_before, false);
      for (std::size_t x = 0; x < m * D * S; ++x)
        if (ids[x] >= K_before && !have[ids[x] - K_before]) {
          have[ids[x] - K_before] = true;
          aa_of_store[ids[x]] = aa_hash[x];
        }
    }
    for (std::size_t i = 0; i < m; ++i) {
      const std::size_t u = off - first + i;
      held_at[u] = held.size();
      if (!std::isfinite(lw[u])) continue;
      for (std::size_t d = 0; d < D; ++d) {
        const std::size_t x0 = (i * D + d) * S;
        for (std::size_t s = 0; s < S; ++s)
          if (ids[x0 + s] >= 0)
            Require(aa_hash[x0 + s] == aa_of_store[ids[x0 + s]],
                    "weighted lineage pipeline: equal sequences with different translation hashes at row " + std::to_string(off + i));
        held.push_back(tab_of_store[ids[x0 + P]]);
        for (std::size_t s = chain[i].size(); s-- > 0;) held.push_back(tab_of_store[ids[x0 + s]]);
      }
      naive_tab[u] = tab_of_store[ids[i * D * S + P]];
    }
    const auto t3 = SteadyNow();
    t_flat += Seconds(t0, t1);
    t_dev += Seconds(t1, t2);
    t_resolve += Seconds(t2, t3);
  }
  held_at[U] = held.size();
  // the weights, then every (row, draw) as one tree of its row's weight, in (row, draw) order
  const auto t_c = SteadyNow();
  LineageWeightSummary ws;
  const std::vector<double> w = LineageWeights(lw, &ws);
  ws.draws_per_row = draws_per_row;
  std::vector<int> l;
  for (std::size_t u = 0; u < U; ++u) {
    if (!std::isfinite(lw[u])) continue;
    const std::size_t len = (std::size_t)path_len[u] + 1;
    for (std::size_t d = 0; d < D; ++d) {
      const int32_t* h = held.data() + held_at[u] + d * len;
      l.assign(h, h + len);
      l.push_back(seed_id);
      tab.AddTree(l, path_len[u], w[u]);
    }
  }
  const auto t_w = SteadyNow();
  WriteLineageFiles(output_prefix, tab.Finish(seed_seq), interner.collisions(), &ws);
  {
    // per row after the burn-in: what upstream's .log subset was for.  naive_id numbers the used rows' naive sequences by
    // first appearance (-1: a skipped row)
    std::ofstream rows(output_prefix + ".rows.tsv");
    if (!rows) throw std::runtime_error("Can't write " + output_prefix + ".rows.tsv");
    rows << "row\tlh_loglik\tlog_weight\tweight\tnaive_id\tpath_len\n";
    std::unordered_map<int32_t, int32_t> naive_id;
    char buf[160];
    for (std::size_t u = 0; u < U; ++u) {
      int32_t id = -1;
      if (std::isfinite(lw[u])) id = naive_id.emplace(naive_tab[u], (int32_t)naive_id.size()).first->second;
      std::snprintf(buf, sizeof buf, "%zu\t%.17g\t%.17g\t%.17g\t%d\t%d\n", first + u, ll[u], lw[u], w[u], (int)id, (int)path_len[u]);
      rows << buf;
    }
  }
  if (timing)
    std::fprintf(stderr,
                 "[RunWeightedLineagePipeline] %zu rows x %zu draws: read %.3f s, parse+schedule+paths %.3f s, device (the chain, "
                 "copies) %.3f s, resolve+read back (%d sequences) %.3f s, count %.3f s, write %.3f s; total %.3f s\n",
                 U, D, Seconds(t_start, t_read), t_flat, t_dev, (int)interner.K(), t_resolve, Seconds(t_c, t_w),
                 Seconds(t_w, SteadyNow()), Seconds(t_start, SteadyNow()));
}

// src/PhyloHMM.cpp:461-471
void StoreGermlinePaddingXmsaIndices(const std::vector<int>& naive_bases, const std::vector<int>& site_inds,
                                     std::map<std::pair<int, int>, int>& xmsa_ids, VectorXi& xmsa_inds) {
  xmsa_inds.assign(naive_bases.size(), -1);
  for (std::size_t i = 0; i < naive_bases.size(); i++)
    StoreXmsaIndex({naive_bases[i], site_inds[i]}, xmsa_ids, xmsa_inds[i]);
}

// src/PhyloHMM.cpp:489-513
void StoreJunctionXmsaIndices(const std::vector<int>& naive_bases, const std::vector<int>& site_inds,
                              std::pair<int, int> left_flexbounds, std::pair<int, int> right_flexbounds,
                              std::map<std::pair<int, int>, int>& xmsa_ids, MatrixXi& xmsa_inds) {
  const int site_start = left_flexbounds.first, site_end = right_flexbounds.second;
  xmsa_inds.setConstant(site_end - site_start, (int)naive_bases.size(), -1);
  for (std::size_t i = 0; i < naive_bases.size(); i++) {
    if (site_inds[i] == -1) {
      for (int site_ind = site_start; site_ind < site_end; site_ind++)
        StoreXmsaIndex({naive_bases[i], site_ind}, xmsa_ids, xmsa_inds(site_ind - site_start, (int)i));
    } else {
      StoreXmsaIndex({naive_bases[i], site_inds[i]}, xmsa_ids, xmsa_inds(site_inds[i] - site_start, (int)i));
    }
  }
}

// src/PhyloHMM.cpp:523-536
void StoreXmsaIndex(std::pair<int, int> id, std::map<std::pair<int, int>, int>& xmsa_ids, int& xmsa_ind) {
  const int next = (int)xmsa_ids.size();
  auto res = xmsa_ids.emplace(id, next);
  xmsa_ind = res.first->second;
}

void PhyloHMM::SetExtendedRange(bool on) {
  // takes effect with the next InitializePhyloEmission / RunPipeline
  if (lh_family_set_extended_range(family(), on ? 1 : 0)) throw std::runtime_error(lh_last_error());
  for (lh_family* f : more_families_)
    if (lh_family_set_extended_range(f, on ? 1 : 0)) throw std::runtime_error(lh_last_error());
}

// ---- what the pipelines over a RevBayes table share ----

int PhyloHMM::BeginPipeline(const std::string& what, const std::string& kernel, double burnin_frac, const std::string* seed_seq) {
  Require(devices_.size() <= 1, "the " + what + " pipeline runs on one device: --devices may list only one");
  Require(burnin_frac >= 0.0 && burnin_frac < 1.0, "burn-in fraction must be in [0, 1)");
  const int seed_tip = seed_seq ? SeedTip(*seed_seq) : 0;
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the " + kernel + " kernel)");
  return seed_tip;
}

namespace {

// the first row after the burn-in
std::size_t FirstUsedRow(std::size_t n_rows, double burnin_frac) {
  return (std::size_t)std::floor(burnin_frac * (double)n_rows);
}

// rows per batch where LH_PIPELINE_BATCH does not say: at most 8192, and `fit` where the rows' tables bound it
std::size_t PipelineBatch(std::size_t fit) {
  return host_options().pipeline_batch > 0 ? (std::size_t)host_options().pipeline_batch : std::min<std::size_t>(8192, fit);
}

// summary.tsv's common lines; `kish_ess` as the pipeline prints its numbers
void WriteSummary(std::ostream& summary, std::size_t used, std::size_t skipped, const std::string& kish_ess) {
  summary << "key\tvalue\nrows_used\t" << used << "\nrows_skipped_nonfinite\t" << skipped << "\nkish_ess\t" << kish_ess << "\n";
}

}  // namespace

// What SumWeightedRows hands the writers: the weighted means, and per row after the burn-in its log weight
struct PhyloHMM::WeightedRows {
  WeightedSums acc;
  std::size_t skipped = 0;
  std::vector<double> lw;
  std::size_t used() const { return lw.size() - skipped; }
  double weight(std::size_t u) const { return std::isfinite(lw[u]) ? std::exp(lw[u] - acc.mx) : 0.0; }
};

// The importance-weighted mean of a table per row, over the rows from `first` on in batches of `batch_rows`:
// pack = batch(tb, off, ll) runs the C entry point on rows off .. off + tb.dev.n - 1 (ll: their log-likelihoods) and
// pack(i, row) lays row i's `width` doubles out.  The rows' tables are added up on the host in row order, each with its
// weight relative to itself: the result does not depend on the batch size.  Rows with a non-finite weight are skipped
// and counted.
template <class Batch>
PhyloHMM::WeightedRows PhyloHMM::SumWeightedRows(const std::string& what, const TsvTable& table, const std::string& input_path,
                                                 std::size_t first, std::size_t batch_rows, std::size_t width,
                                                 bool with_children, Batch&& batch) const {
  const std::size_t N = table.rows.size();
  WeightedRows r{WeightedSums(width), 0, std::vector<double>(N - first)};
  std::vector<double> row(width);
  for (std::size_t off = first; off < N; off += batch_rows) {
    const std::size_t m = std::min(batch_rows, N - off);
    const TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path, with_children);
    std::vector<double> ll(m);
    const auto pack = batch(tb, off, ll.data());
    for (std::size_t i = 0; i < m; ++i) {
      const double st[3] = {ll[i] - tb.lik[i], 1.0, 1.0};  // one row, its weight relative to itself
      r.lw[off - first + i] = st[0];
      if (!std::isfinite(st[0])) {
        ++r.skipped;
        continue;
      }
      pack(i, row.data());
      r.acc.Add(row.data(), st);
    }
  }
  Require(r.acc.s1 > 0.0, what + " pipeline: no row with a finite weight");
  r.acc.Normalise();
  return r;
}

void PhyloHMM::RunMarginalsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                    double burnin_frac) {
  BeginPipeline("marginals", "posterior", burnin_frac);
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t N = table.rows.size();
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  const std::size_t FS = (std::size_t)lh_forward_size(family_);
  constexpr std::size_t kBatch = 49152;
  // running combination of the batches' (sum w pi, max lw, sum w, sum w^2), each relative to the running max
  WeightedSums acc(FS);
  std::vector<double> wsum(FS);
  std::size_t skipped = 0;
  for (std::size_t off = first; off < N; off += kBatch) {
    const std::size_t m = std::min(kBatch, N - off);
    TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
    const DeviceBatch& b = tb.dev;
    std::vector<double> ll(m);
    double st[3];
    lh_posterior_outputs outs{tb.lik.data(), ll.data(), nullptr, wsum.data(), st};
    CheckHip(lh_eval_posterior_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                     b.pi.data(), b.alpha.data(), num_rates, &outs),
             "lh_eval_posterior_batch");
    for (std::size_t i = 0; i < m; ++i)
      if (!std::isfinite(ll[i] - tb.lik[i])) ++skipped;
    acc.Add(wsum.data(), st);
  }
  Require(acc.s1 > 0.0, "marginals pipeline: no row with a finite weight");
  acc.Normalise();
  const NaiveMarginalsResult res = MapPosterior(acc.total.data());
  std::ofstream sites(output_prefix + ".sites.tsv"), genes(output_prefix + ".genes.tsv"),
      summary(output_prefix + ".summary.tsv");
  Require(sites.good() && genes.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteSiteTable(sites, res);
  WriteGeneTable(genes, res);
  WriteSummary(summary, N - first - skipped, skipped, Fmt17(acc.KishEss()));
}


// ---- K11: exact ancestral-state marginals along a seed's lineage ----

int PhyloHMM::SeedTip(const std::string& seed_seq) const {
  Require(seed_seq != "naive", "the seed sequence cannot be 'naive': the lineage ends there");
  const int T = (int)xmsa_labels_.size();
  for (int v = 1; v < T; ++v)
    if (xmsa_labels_[v] == seed_seq) return v;
  throw std::runtime_error("the seed sequence '" + seed_seq + "' is not a sequence of this clonal family");
}

// The current tree as K11's and K12's entry points take it: its schedule and the seed's chain of ancestors
struct PhyloHMM::SeedLineage {
  int seed_tip = 0;
  std::vector<int32_t> ops, nodes;
  int32_t depth = 0;
};

PhyloHMM::SeedLineage PhyloHMM::OpenSeedLineage(const std::string& seed_seq) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  SeedLineage s;
  s.seed_tip = SeedTip(seed_seq);
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the posterior kernel)");
  const int T = tree_.n_tips;
  s.ops.resize((std::size_t)(T - 2) * 4);
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, s.ops.data(), &s.depth), "lh_schedule_tree");
  s.nodes = SeedPath(tree_.children.data(), T, tree_.root, s.seed_tip);
  Require(!s.nodes.empty(), "the seed sequence '" + seed_seq + "' does not descend from the root");
  return s;
}

PhyloHMM::AncestralMarginalsResult PhyloHMM::AncestralMarginals(const std::string& seed_seq) {
  SeedLineage s = OpenSeedLineage(seed_seq);
  const int T = tree_.n_tips, R = num_rates_;
  const std::size_t L = (std::size_t)msa_.cols();
  AncestralMarginalsResult res;
  res.nodes = std::move(s.nodes);
  const std::size_t P = res.nodes.size();
  res.n_sites = (int)L;
  res.num_rates = R;
  res.marg.assign(P * L * 4, 0.0);
  res.rate_post.assign(L * (std::size_t)R, 0.0);
  lh_ancestral_outputs outs{};
  outs.loglik = &res.loglik;
  outs.marg = res.marg.data();
  outs.rate_post = res.rate_post.data();
  CheckHip(lh_eval_ancestral_batch(family_, 1, T, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_, R,
                                   res.nodes.data(), (int32_t)P, &outs),
           "lh_eval_ancestral_batch");
  return res;
}

void PhyloHMM::WriteNodeTable(std::ostream& o, const double* table, std::size_t n_sites) {
  static const char kBases[] = "ACGT";
  o << "site\tA\tC\tG\tT\tmap_base\n";
  for (std::size_t s = 0; s < n_sites; ++s) {
    const double* p = table + s * 4;
    o << s;
    for (int c = 0; c < 4; ++c) o << '\t' << Fmt17(p[c]);
    o << '\t' << kBases[std::max_element(p, p + 4) - p] << '\n';
  }
}

void PhyloHMM::WriteRateTable(std::ostream& o, const double* rate_post, std::size_t n_sites, int num_rates) {
  o << "site";
  for (int k = 0; k < num_rates; ++k) o << "\trate" << k;
  o << '\n';
  for (std::size_t s = 0; s < n_sites; ++s) {
    o << s;
    for (int k = 0; k < num_rates; ++k) o << '\t' << Fmt17(rate_post[s * num_rates + k]);
    o << '\n';
  }
}

// The seed's chains of a batch of table rows (FlattenTable with the children), padded with -1 into path[m][P]
struct PhyloHMM::SeedChains {
  std::vector<std::vector<int32_t>> chain;
  std::size_t P = 1;
  std::vector<int32_t> path;
};

// *path_len: the lengths of the chains of rows off .. off + m - 1
PhyloHMM::SeedChains PhyloHMM::SeedChainsOf(const TableBatch& tb, std::size_t off, int seed_tip, const std::string& seed_seq,
                                            int32_t* path_len) const {
  const int T = (int)xmsa_labels_.size();
  const std::size_t m = (std::size_t)tb.dev.n;
  SeedChains c;
  c.chain.resize(m);
  for (std::size_t i = 0; i < m; ++i) {
    c.chain[i] = SeedPath(tb.children.data() + i * 2 * (std::size_t)(T - 2), T, tb.root[i], seed_tip);
    Require(!c.chain[i].empty(),
            "row " + std::to_string(off + i) + ": the seed sequence '" + seed_seq + "' does not descend from the root");
    c.P = std::max(c.P, c.chain[i].size());
    path_len[i] = (int32_t)c.chain[i].size();
  }
  c.path.assign(m * c.P, -1);
  for (std::size_t i = 0; i < m; ++i) std::copy(c.chain[i].begin(), c.chain[i].end(), c.path.begin() + i * c.P);
  return c;
}

// rows.tsv of K11's and K12's pipelines: row, weight, chain_length, and the column `extra_name` where there is one
void PhyloHMM::WriteSeedRows(std::ostream& rows, std::size_t first, const WeightedRows& w, const std::vector<int32_t>& path_len,
                             const char* extra_name, const std::vector<double>* extra) {
  rows << "row\tweight\tchain_length" << (extra ? "\t" : "") << (extra ? extra_name : "") << '\n';
  for (std::size_t u = 0; u < w.lw.size(); ++u) {
    rows << (first + u) << '\t' << Fmt17(w.weight(u)) << '\t' << path_len[u];
    if (extra) rows << '\t' << Fmt17((*extra)[u]);
    rows << '\n';
  }
}

std::vector<int32_t> PhyloHMM::WithTips(int seed_tip, const std::vector<std::string>& with) const {
  const int T = (int)xmsa_labels_.size();
  std::vector<int32_t> tips;
  for (const std::string& name : with) {
    Require(name != "naive", "--node mrca-with: the sequence cannot be 'naive': the node it shares with the seed is 'mrca'");
    int tip = 0;
    for (int v = 1; v < T && tip == 0; ++v)
      if (xmsa_labels_[v] == name) tip = v;
    Require(tip != 0, "--node mrca-with: '" + name + "' is not a sequence of this clonal family");
    Require(tip != seed_tip, "--node mrca-with: '" + name + "' is the seed sequence itself");
    tips.push_back(tip);
  }
  return tips;
}

std::vector<int32_t> PhyloHMM::CladeSlotsOf(const TableBatch& tb, int seed_tip, const std::vector<int32_t>& with_tips) const {
  const int T = (int)xmsa_labels_.size();
  std::vector<int32_t> slot;
  if (with_tips.empty()) return slot;
  slot.resize((std::size_t)tb.dev.n);
  for (std::size_t i = 0; i < slot.size(); ++i)
    slot[i] = CladeSlot(tb.children.data() + i * 2 * (std::size_t)(T - 2), T, tb.root[i], seed_tip, with_tips).slot;
  return slot;
}

namespace {

// a pipeline's node from the entry points' integer (0 or 1)
LineageNode FixedLineageNode(int node) {
  LineageNode n;
  n.node = node;
  return n;
}

// the lines a pipeline at a clade node adds to summary.tsv: the range of the slots over every row after the burn-in, the
// rows skipped for a non-finite weight included (rows.tsv lists them too); NA where no row is left
void WriteSlotSummary(std::ostream& summary, const std::vector<double>& slots) {
  if (slots.empty()) {
    summary << "slot_min\tNA\nslot_max\tNA\n";
    return;
  }
  summary << "slot_min\t" << (int)*std::min_element(slots.begin(), slots.end()) << "\nslot_max\t"
          << (int)*std::max_element(slots.begin(), slots.end()) << "\n";
}

}  // namespace

void PhyloHMM::RunAncestralMarginalsPipeline(const std::string& input_path, const std::string& seed_seq,
                                             const std::string& output_prefix, int num_rates, double burnin_frac) {
  const int seed_tip = BeginPipeline("ancestral marginals", "posterior", burnin_frac, &seed_seq);
  const int T = (int)xmsa_labels_.size(), R = num_rates;
  const std::size_t L = (std::size_t)msa_.cols();
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  // the rows' tables come back whole (32 P L bytes each, P <= T - 2): a batch is bounded by at most 512 MiB of them
  const std::size_t NE = 2 * L * 4, NR = L * (std::size_t)R;
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * ((std::size_t)(T - 2) * L * 4 + NR)));
  std::vector<double> marg, rate_post;
  std::vector<int32_t> path_len(table.rows.size() - first, 0);
  SeedChains sc;
  const WeightedRows w = SumWeightedRows(
      "ancestral marginals", table, input_path, first, PipelineBatch(fit), NE + NR, true,
      [&](const TableBatch& tb, std::size_t off, double* ll) {
        const DeviceBatch& b = tb.dev;
        sc = SeedChainsOf(tb, off, seed_tip, seed_seq, path_len.data() + (off - first));
        marg.resize((std::size_t)b.n * sc.P * L * 4);
        rate_post.resize((std::size_t)b.n * NR);
        lh_ancestral_outputs outs{};
        outs.loglik = ll;
        outs.marg = marg.data();
        outs.rate_post = rate_post.data();
        CheckHip(lh_eval_ancestral_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                         b.pi.data(), b.alpha.data(), R, sc.path.data(), (int32_t)sc.P, &outs),
                 "lh_eval_ancestral_batch");
        return [&](std::size_t i, double* row) {
          const std::size_t len = sc.chain[i].size();
          const double* mi = marg.data() + i * sc.P * L * 4;
          std::copy(mi, mi + L * 4, row);                                    // the seed's parent
          std::copy(mi + (len - 1) * L * 4, mi + len * L * 4, row + L * 4);  // the MRCA
          std::copy(rate_post.begin() + i * NR, rate_post.begin() + (i + 1) * NR, row + NE);
        };
      });
  std::ofstream parent(output_prefix + ".parent.tsv"), mrca(output_prefix + ".mrca.tsv"), rates(output_prefix + ".rates.tsv"),
      rows(output_prefix + ".rows.tsv"), summary(output_prefix + ".summary.tsv");
  Require(parent.good() && mrca.good() && rates.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteNodeTable(parent, w.acc.total.data(), L);
  WriteNodeTable(mrca, w.acc.total.data() + L * 4, L);
  WriteRateTable(rates, w.acc.total.data() + NE, L, R);
  WriteSeedRows(rows, first, w, path_len);
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
}


// ---- K12: exact substitution posteriors along the edges of a seed's lineage ----

PhyloHMM::LineageSubstitutionsResult PhyloHMM::LineageSubstitutions(const std::string& seed_seq) {
  SeedLineage lin = OpenSeedLineage(seed_seq);
  const int T = tree_.n_tips, R = num_rates_, seed_tip = lin.seed_tip;
  const std::size_t L = (std::size_t)msa_.cols();
  LineageSubstitutionsResult res;
  res.nodes = std::move(lin.nodes);
  const std::size_t P = res.nodes.size();
  res.n_sites = (int)L;
  res.edge.assign(P * L * 16, 0.0);
  res.naive_edge.assign(L * 20, 0.0);
  res.chain_counts.assign(L * 16, 0.0);
  std::vector<double> load(P + 1, 0.0);
  lh_eval_edges_outputs outs{};
  outs.loglik = &res.loglik;
  outs.edge = res.edge.data();
  outs.naive_edge = res.naive_edge.data();
  outs.chain_counts = res.chain_counts.data();
  outs.edge_load = load.data();
  CheckHip(lh_eval_edges_batch(family_, 1, T, lin.depth, lin.ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_, R,
                               res.nodes.data(), (int32_t)P, seed_tip, &outs),
           "lh_eval_edges_batch");
  res.edges.resize(P + 1);
  for (std::size_t s = 0; s <= P; ++s) {
    LineageSubstitutionsResult::Edge& e = res.edges[s];
    e.upper = s < P ? res.nodes[s] : 0;
    e.lower = s == P ? res.nodes[P - 1] : s == 0 ? seed_tip : res.nodes[s - 1];
    e.brlen = tree_.brlen[s == P ? 0 : e.lower];
    e.load = load[s];
  }
  return res;
}

void PhyloHMM::WritePairTable(std::ostream& o, const double* table, std::size_t n_sites, int n_rows, bool with_sum) {
  static const char kBases[] = "ACGTN";
  o << "site";
  for (int a = 0; a < n_rows; ++a)
    for (int c = 0; c < 4; ++c) o << '\t' << kBases[a] << kBases[c];
  if (with_sum) o << "\tsubstitutions";
  o << '\n';
  for (std::size_t s = 0; s < n_sites; ++s) {
    const double* p = table + s * (std::size_t)n_rows * 4;
    o << s;
    double off = 0.0;
    for (int a = 0; a < n_rows; ++a)
      for (int c = 0; c < 4; ++c) {
        o << '\t' << Fmt17(p[a * 4 + c]);
        if (a < 4 && a != c) off += p[a * 4 + c];
      }
    if (with_sum) o << '\t' << Fmt17(off);
    o << '\n';
  }
}

void PhyloHMM::RunLineageSubstitutionsPipeline(const std::string& input_path, const std::string& seed_seq,
                                               const std::string& output_prefix, int num_rates, double burnin_frac) {
  const int seed_tip = BeginPipeline("lineage substitutions", "posterior", burnin_frac, &seed_seq);
  const int T = (int)xmsa_labels_.size(), R = num_rates;
  const std::size_t L = (std::size_t)msa_.cols();
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  // only the rows' reductions come back (52 L + P + 1 doubles each): a batch is bounded by at most 512 MiB of them
  const std::size_t NC = L * 16, NN = L * 20, NROW = 2 * NC + NN;
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * (NROW + (std::size_t)T)));
  std::vector<double> cc, se, ne, load, subs(table.rows.size() - first, 0.0);
  std::vector<int32_t> path_len(table.rows.size() - first, 0);
  const WeightedRows w = SumWeightedRows(
      "lineage substitutions", table, input_path, first, PipelineBatch(fit), NROW, true,
      [&](const TableBatch& tb, std::size_t off, double* ll) {
        const DeviceBatch& b = tb.dev;
        const std::size_t m = (std::size_t)b.n;
        const SeedChains sc = SeedChainsOf(tb, off, seed_tip, seed_seq, path_len.data() + (off - first));
        const std::size_t P = sc.P;
        cc.resize(m * NC);
        se.resize(m * NC);
        ne.resize(m * NN);
        load.resize(m * (P + 1));
        lh_eval_edges_outputs outs{};
        outs.loglik = ll;
        outs.chain_counts = cc.data();
        outs.seed_edge = se.data();
        outs.naive_edge = ne.data();
        outs.edge_load = load.data();
        CheckHip(lh_eval_edges_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(), b.pi.data(),
                                     b.alpha.data(), R, sc.path.data(), (int32_t)P, seed_tip, &outs),
                 "lh_eval_edges_batch");
        for (std::size_t i = 0; i < m; ++i) {
          const double* li = load.data() + i * (P + 1);
          double total = li[P];  // the naive edge, then the slots from the MRCA down (padding slots hold 0)
          for (std::size_t s = sc.chain[i].size(); s-- > 0;) total += li[s];
          subs[off - first + i] = total;
        }
        return [&](std::size_t i, double* row) {
          std::copy(cc.begin() + i * NC, cc.begin() + (i + 1) * NC, row);
          std::copy(se.begin() + i * NC, se.begin() + (i + 1) * NC, row + NC);
          std::copy(ne.begin() + i * NN, ne.begin() + (i + 1) * NN, row + 2 * NC);
        };
      });
  std::ofstream counts(output_prefix + ".substitutions.tsv"), seed(output_prefix + ".seed_edge.tsv"),
      naive(output_prefix + ".naive_edge.tsv"), rows(output_prefix + ".rows.tsv"), summary(output_prefix + ".summary.tsv");
  Require(counts.good() && seed.good() && naive.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WritePairTable(counts, w.acc.total.data(), L, 4, true);
  WritePairTable(seed, w.acc.total.data() + NC, L, 4, false);
  WritePairTable(naive, w.acc.total.data() + 2 * NC, L, 5, false);
  WriteSeedRows(rows, first, w, path_len, "expected_substitutions", &subs);
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
}


// ---- K9: codon and amino-acid marginals ----

namespace {

// the layout lh_family_set_codons built
struct CodonLayout {
  int32_t n_codons = 0, n_window = 0, n_genes = 0;
  std::vector<int32_t> window_codon;
};

CodonLayout SetCodons(lh_family* fam, int frame) {
  if (lh_family_set_codons(fam, frame)) throw std::runtime_error(lh_last_error());
  CodonLayout lay;
  if (lh_codon_layout(fam, &lay.n_codons, &lay.n_window, nullptr, &lay.n_genes)) throw std::runtime_error(lh_last_error());
  lay.window_codon.resize(lay.n_window);
  if (lh_codon_layout(fam, nullptr, nullptr, lay.window_codon.data(), nullptr)) throw std::runtime_error(lh_last_error());
  return lay;
}

}  // namespace

PhyloHMM::CodonMarginalsResult PhyloHMM::ExpandCodons(int frame, const std::vector<int32_t>& window_codon,
                                                      const double* windows, const double* genes) const {
  const int L = (int)msa_.cols();
  const bool igh = locus_ == "igh";
  CodonMarginalsResult m;
  m.frame = frame;
  std::array<double, 125> zero;
  zero.fill(0.0);
  m.codons.assign(L >= frame ? (L - frame) / 3 : 0, zero);
  std::vector<char> is_window(m.codons.size(), 0);
  for (std::size_t i = 0; i < window_codon.size(); ++i) {
    const std::size_t c = (std::size_t)window_codon.at(i);
    Require(c < m.codons.size(), "ExpandCodons: window codon out of range");
    is_window[c] = 1;
    std::copy(windows + i * 125, windows + (i + 1) * 125, m.codons[c].begin());
  }
  // per region: first gene posterior, and every gene's base per site (N where it writes none)
  struct Region {
    const RegionStates* R;
    std::size_t off;
    std::vector<uint8_t> base;  // [genes][L]
  };
  std::vector<Region> regions;
  std::size_t off = 0;
  for (const RegionStates* R : {&vgerm_, igh ? &dgerm_ : nullptr, &jgerm_}) {
    if (!R) continue;
    Region r{R, off, std::vector<uint8_t>(R->ggene_ranges.size() * (std::size_t)L, 4)};
    std::size_t g = 0;
    for (const auto& kv : R->ggene_ranges) {
      for (int k = kv.second.first; k < kv.second.second; ++k) r.base[g * L + R->site_inds[k]] = (uint8_t)R->naive_bases[k];
      ++g;
    }
    off += g;
    regions.push_back(std::move(r));
  }
  const int v_end = flexbounds_.at("v_r").first;
  const int d_end = igh ? flexbounds_.at("d_r").first : v_end;
  for (std::size_t c = 0; c < m.codons.size(); ++c) {
    if (is_window[c]) continue;
    const int s0 = frame + 3 * (int)c;
    const Region& r = s0 < v_end ? regions.front() : (igh && s0 < d_end) ? regions[1] : regions.back();
    const std::size_t n = r.R->ggene_ranges.size();
    for (std::size_t g = 0; g < n; ++g) {
      const uint8_t* b = r.base.data() + g * L + s0;
      m.codons[c][25 * b[0] + 5 * b[1] + b[2]] += genes[r.off + g];
    }
  }
  return m;
}

PhyloHMM::CodonMarginalsResult PhyloHMM::NaiveCodonMarginals(int frame) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the codon kernel)");
  const CodonLayout lay = SetCodons(family_, frame);
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  std::vector<double> windows((std::size_t)lay.n_window * 125), genes(lay.n_genes);
  double ll = 0;
  lh_codon_outputs outs{nullptr, &ll, windows.data(), genes.data(), nullptr, nullptr, nullptr};
  CheckHip(lh_eval_codons_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                num_rates_, &outs),
           "lh_eval_codons_batch");
  return ExpandCodons(frame, lay.window_codon, windows.data(), genes.data());
}

void PhyloHMM::WriteCodonTable(std::ostream& o, const CodonMarginalsResult& m) {
  static const char kBases[] = "ACGTN";
  o << "codon\tfirst_site\tbases\tprobability\n";
  for (std::size_t c = 0; c < m.codons.size(); ++c)
    for (int i = 0; i < 125; ++i)
      if (m.codons[c][i] > 0.0)
        o << c << '\t' << (m.frame + 3 * c) << '\t' << kBases[i / 25] << kBases[(i / 5) % 5] << kBases[i % 5] << '\t'
          << ReprDouble(m.codons[c][i]) << '\n';
}

void PhyloHMM::WriteAminoAcidTable(std::ostream& o, const CodonMarginalsResult& m) {
  static const std::string aa_of = [] {
    static const char kBases[] = "ACGTN";
    std::string dna;
    for (int i = 0; i < 125; ++i) dna += {kBases[i / 25], kBases[(i / 5) % 5], kBases[i % 5]};
    return TranslateDna(dna);
  }();
  o << "codon\taa\tprobability\n";
  for (std::size_t c = 0; c < m.codons.size(); ++c) {
    std::map<char, double> p;
    for (int i = 0; i < 125; ++i)
      if (m.codons[c][i] > 0.0) p[aa_of[i]] += m.codons[c][i];
    for (const auto& kv : p) o << c << '\t' << kv.first << '\t' << ReprDouble(kv.second) << '\n';
  }
}

void PhyloHMM::RunCodonMarginalsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                         double burnin_frac, int frame) {
  BeginPipeline("codon marginals", "codon", burnin_frac);
  const CodonLayout lay = SetCodons(family_, frame);
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  const std::size_t NW = (std::size_t)lay.n_window * 125, NG = (std::size_t)lay.n_genes;
  // the rows' windows and genes come back whole: a batch is bounded by their size (NW + NG doubles per row)
  std::vector<double> windows, genes;
  const WeightedRows w = SumWeightedRows(
      "codon marginals", table, input_path, first, PipelineBatch(8192), NW + NG, false,
      [&](const TableBatch& tb, std::size_t, double* ll) {
        const DeviceBatch& b = tb.dev;
        windows.resize((std::size_t)b.n * NW);
        genes.resize((std::size_t)b.n * NG);
        lh_codon_outputs outs{nullptr, ll, windows.data(), genes.data(), nullptr, nullptr, nullptr};
        CheckHip(lh_eval_codons_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                      b.pi.data(), b.alpha.data(), num_rates, &outs),
                 "lh_eval_codons_batch");
        return [&](std::size_t i, double* row) {
          std::copy(windows.begin() + i * NW, windows.begin() + (i + 1) * NW, row);
          std::copy(genes.begin() + i * NG, genes.begin() + (i + 1) * NG, row + NW);
        };
      });
  const CodonMarginalsResult res = ExpandCodons(frame, lay.window_codon, w.acc.total.data(), w.acc.total.data() + NW);
  std::ofstream codons(output_prefix + ".codons.tsv"), aa(output_prefix + ".aa.tsv"), summary(output_prefix + ".summary.tsv");
  Require(codons.good() && aa.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteCodonTable(codons, res);
  WriteAminoAcidTable(aa, res);
  WriteSummary(summary, w.used(), w.skipped, ReprDouble(w.acc.KishEss()));
  summary << "frame\t" << frame << "\n";
}


// ---- K10: posteriors of deletion and insertion lengths ----

namespace {

// one junction of the events row, as the host's state space describes it
struct EventsJunctionView {
  const RegionStates *J, *GL, *GR;
  int site0, W;
  const char *left_column, *right_column, *name;
};

std::vector<EventsJunctionView> EventsJunctions(const std::string& locus, const std::map<std::string, std::pair<int, int>>& fb,
                                                const RegionStates& vgerm, const RegionStates& vd, const RegionStates& dgerm,
                                                const RegionStates& dj, const RegionStates& jgerm) {
  const int v0 = fb.at("v_r").first;
  if (locus == "igh")
    return {{&vd, &vgerm, &dgerm, v0, fb.at("d_l").second - v0, "V3pDel", "D5pDel", "VD"},
            {&dj, &dgerm, &jgerm, fb.at("d_r").first, fb.at("j_l").second - fb.at("d_r").first, "D3pDel", "J5pDel", "DJ"}};
  return {{&vd, &vgerm, &jgerm, v0, fb.at("j_l").second - v0, "V3pDel", "J5pDel", "VJ"}};
}

}  // namespace

std::size_t PhyloHMM::EventsGenes() const {
  return vgerm_.ggene_ranges.size() + (locus_ == "igh" ? dgerm_.ggene_ranges.size() : 0) + jgerm_.ggene_ranges.size();
}

std::size_t PhyloHMM::EventsSize() const {
  std::size_t size = 0;
  for (const EventsJunctionView& j : EventsJunctions(locus_, flexbounds_, vgerm_, vd_junction_, dgerm_, dj_junction_, jgerm_))
    size += (j.GL->ggene_ranges.size() + j.GR->ggene_ranges.size() + (std::size_t)j.W + 1) * ((std::size_t)j.W + 1);
  return size;
}

PhyloHMM::EventsResult PhyloHMM::MapEvents(const double* events, const double* genes) const {
  // (column, gene, length) -> probability, in the order of the files: the columns as the annotation prints them, "*"
  // (every gene) before the genes
  static const char* const kColumns[] = {"V5pDel", "V3pDel", "D5pDel", "D3pDel", "J5pDel", "J3pDel"};
  auto column_rank = [](const std::string& c) {
    for (int k = 0; k < 6; ++k)
      if (c == kColumns[k]) return k;
    throw std::runtime_error("MapEvents: unknown column " + c);
  };
  std::map<std::tuple<int, std::string, int>, double> del;
  auto add = [&](const std::string& column, const std::string& gene, int length, double p) {
    if (!(p > 0.0)) return;  // (also leaves out a NaN)
    del[{column_rank(column), gene, length}] += p;
    del[{column_rank(column), "*", length}] += p;
  };
  auto state_index = [](const RegionStates& G) {
    std::map<std::string, int> ix;
    for (std::size_t k = 0; k < G.state_strs.size(); ++k) ix[G.state_strs[k]] = (int)k;
    return ix;
  };
  EventsResult res;
  const double* t = events;
  for (const EventsJunctionView& j : EventsJunctions(locus_, flexbounds_, vgerm_, vd_junction_, dgerm_, dj_junction_, jgerm_)) {
    const int W = j.W, W1 = W + 1;
    const std::size_t nL = j.GL->ggene_ranges.size(), nR = j.GR->ggene_ranges.size();
    const double *exit_t = t, *enter_t = exit_t + nL * W1, *span = enter_t + nR * W1;
    t = span + (std::size_t)W1 * W1;
    const std::map<std::string, int> ixL = state_index(*j.GL), ixR = state_index(*j.GR);
    std::size_t l = 0;
    for (const auto& kv : j.GL->ggene_ranges) {  // (a std::map: the genes by name, the compact layout's order)
      const auto jr = j.J->ggene_ranges.find(kv.first);
      const int rows = jr == j.J->ggene_ranges.end() ? 0 : jr->second.second - jr->second.first;
      for (int a = 0; a <= W; ++a) {
        const double p = exit_t[l * W1 + a];
        if (!(p > 0.0)) continue;
        if (a == 0) {
          add(j.left_column, kv.first, j.GL->right_del[ixL.at(kv.first)], p);
          continue;
        }
        Require(a <= rows, "MapEvents: weight on a junction row the left gene " + kv.first + " has no state on");
        const int k = jr->second.first + (a - 1);
        Require(j.J->site_inds[k] - j.site0 == a - 1, "MapEvents: the left gene's junction states are not on consecutive rows");
        add(j.left_column, kv.first, j.J->del[k], p);
      }
      ++l;
    }
    std::size_t r = 0;
    for (const auto& kv : j.GR->ggene_ranges) {
      const auto jr = j.J->ggene_ranges.find(kv.first);
      Require(jr != j.J->ggene_ranges.end(), "MapEvents: the right gene " + kv.first + " has no junction states");
      const int g0 = jr->second.first + 4, g1 = jr->second.second;  // its germline states (after the four NTI states)
      const int first = g0 < g1 ? j.J->site_inds[g0] - j.site0 : W;
      for (int b = 0; b <= W; ++b) {
        const double p = enter_t[r * W1 + b];
        if (!(p > 0.0)) continue;
        if (b == W) {
          add(j.right_column, kv.first, j.GR->left_del[ixR.at(kv.first)], p);
          continue;
        }
        Require(b >= first && g0 + (b - first) < g1, "MapEvents: weight on a junction row the right gene " + kv.first + " has no state on");
        const int k = g0 + (b - first);
        Require(j.J->site_inds[k] - j.site0 == b, "MapEvents: the right gene's junction states are not on consecutive rows");
        add(j.right_column, kv.first, j.J->del[k], p);
      }
      ++r;
    }
    for (int k = 0; k <= W; ++k) {  // the k-th diagonal, from the top
      double p = 0.0;
      for (int a = 0; a + k <= W; ++a) p += span[(std::size_t)a * W1 + a + k];
      if (p > 0.0) res.insertions.push_back({j.name, k, p});
    }
    for (int a = 0; a <= W; ++a)
      for (int b = a; b <= W; ++b)
        if (span[(std::size_t)a * W1 + b] > 0.0) res.spans.push_back({j.name, a, b, span[(std::size_t)a * W1 + b]});
  }
  // the outer ends are functions of the gene alone
  {
    std::size_t g = 0;
    for (const auto& kv : vgerm_.ggene_ranges) add("V5pDel", kv.first, vgerm_.left_del[state_index(vgerm_).at(kv.first)], genes[g++]);
    g = EventsGenes() - jgerm_.ggene_ranges.size();
    for (const auto& kv : jgerm_.ggene_ranges) add("J3pDel", kv.first, jgerm_.right_del[state_index(jgerm_).at(kv.first)], genes[g++]);
  }
  for (const auto& kv : del)
    res.deletions.push_back({kColumns[std::get<0>(kv.first)], std::get<1>(kv.first), std::get<2>(kv.first), kv.second});
  return res;
}

PhyloHMM::EventsResult PhyloHMM::RearrangementEvents() {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the events kernel)");
  int64_t size = 0;
  int32_t n_genes = 0;
  CheckHip(lh_events_layout(family_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &size, &n_genes),
           "lh_events_layout");
  Require((std::size_t)size == EventsSize() && (std::size_t)n_genes == EventsGenes(),
          "the device's events layout differs from the host's state space");
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  std::vector<double> events((std::size_t)size), genes((std::size_t)n_genes);
  double ll = 0;
  lh_events_outputs outs{nullptr, &ll, events.data(), genes.data(), nullptr, nullptr, nullptr};
  CheckHip(lh_eval_events_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                num_rates_, &outs),
           "lh_eval_events_batch");
  Require(std::isfinite(ll), "RearrangementEvents: the log-likelihood is not finite");
  return MapEvents(events.data(), genes.data());
}

void PhyloHMM::WriteDeletionTable(std::ostream& o, const EventsResult& m) {
  o << "column\tgene\tlength\tprobability\n";
  for (const EventsResult::Deletion& d : m.deletions)
    o << d.column << '\t' << d.gene << '\t' << d.length << '\t' << Fmt17(d.p) << '\n';
}

void PhyloHMM::WriteInsertionTable(std::ostream& o, const EventsResult& m) {
  o << "junction\tlength\tprobability\n";
  for (const EventsResult::Insertion& d : m.insertions) o << d.junction << '\t' << d.length << '\t' << Fmt17(d.p) << '\n';
}

void PhyloHMM::WriteSpanTable(std::ostream& o, const EventsResult& m) {
  o << "junction\tleft_rows\tright_first\tprobability\n";
  for (const EventsResult::Span& d : m.spans)
    o << d.junction << '\t' << d.left_rows << '\t' << d.right_first << '\t' << Fmt17(d.p) << '\n';
}

void PhyloHMM::RunEventsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                 double burnin_frac) {
  BeginPipeline("events", "events", burnin_frac);
  const std::size_t NE = EventsSize(), NG = EventsGenes();
  {
    int64_t size = 0;
    int32_t n_genes = 0;
    CheckHip(lh_events_layout(family_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &size, &n_genes),
             "lh_events_layout");
    Require((std::size_t)size == NE && (std::size_t)n_genes == NG, "the device's events layout differs from the host's state space");
  }
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  // the rows' tables come back whole: a batch is bounded by their size (at most 512 MiB of them)
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * (NE + NG)));
  std::vector<double> events, genes;
  const WeightedRows w = SumWeightedRows(
      "events", table, input_path, first, PipelineBatch(fit), NE + NG, false,
      [&](const TableBatch& tb, std::size_t, double* ll) {
        const DeviceBatch& b = tb.dev;
        events.resize((std::size_t)b.n * NE);
        genes.resize((std::size_t)b.n * NG);
        lh_events_outputs outs{nullptr, ll, events.data(), genes.data(), nullptr, nullptr, nullptr};
        CheckHip(lh_eval_events_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                      b.pi.data(), b.alpha.data(), num_rates, &outs),
                 "lh_eval_events_batch");
        return [&](std::size_t i, double* row) {
          std::copy(events.begin() + i * NE, events.begin() + (i + 1) * NE, row);
          std::copy(genes.begin() + i * NG, genes.begin() + (i + 1) * NG, row + NE);
        };
      });
  const EventsResult res = MapEvents(w.acc.total.data(), w.acc.total.data() + NE);
  std::ofstream dels(output_prefix + ".deletions.tsv"), ins(output_prefix + ".insertions.tsv"),
      spans(output_prefix + ".spans.tsv"), summary(output_prefix + ".summary.tsv");
  Require(dels.good() && ins.good() && spans.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteDeletionTable(dels, res);
  WriteInsertionTable(ins, res);
  WriteSpanTable(spans, res);
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
}


namespace {

// ACGTN strings -> bytes 0..4 (the naive-base alphabet)
std::vector<uint8_t> EncodeSeqs(const std::vector<std::string>& seqs, const std::string& alphabet, int L) {
  std::vector<uint8_t> b(seqs.size() * (std::size_t)L);
  for (std::size_t k = 0; k < seqs.size(); ++k) {
    Require((int)seqs[k].size() == L, "candidate " + std::to_string(k) + " does not have the alignment's length");
    for (int j = 0; j < L; ++j) {
      const std::size_t a = alphabet.find(seqs[k][j]);
      Require(a != std::string::npos && a < 5, "candidate " + std::to_string(k) + " holds a character outside ACGTN");
      b[k * L + j] = (uint8_t)a;
    }
  }
  return b;
}

}  // namespace

std::vector<double> PhyloHMM::CandidatePosterior(const std::vector<std::string>& seqs, double* loglik,
                                                 std::vector<double>* log_prior) {
  Require(have_tree_, "InitializePhyloParameters must be called first");
  Require(!seqs.empty(), "CandidatePosterior: no candidates");
  CreateFamily();
  const int L = msa_.cols(), K = (int)seqs.size();
  const std::vector<uint8_t> b = EncodeSeqs(seqs, alphabet_, L);
  std::vector<double> prior(K);
  CheckHip(lh_family_set_candidates(family_, K, b.data(), prior.data()), "lh_family_set_candidates");
  const int T = tree_.n_tips;
  std::vector<int32_t> ops((std::size_t)(T - 2) * 4);
  int32_t depth = 0;
  CheckHip(lh_schedule_tree(T, tree_.children.data(), tree_.root, ops.data(), &depth), "lh_schedule_tree");
  std::vector<double> lc(K);
  double ll = 0;
  lh_candidate_outputs outs{nullptr, &ll, lc.data(), nullptr, nullptr};
  CheckHip(lh_eval_candidates_batch(family_, 1, T, depth, ops.data(), tree_.brlen.data(), er_.data(), pi_.data(), &alpha_,
                                    num_rates_, &outs),
           "lh_eval_candidates_batch");
  if (loglik) *loglik = ll;
  if (log_prior) *log_prior = prior;
  return lc;
}

// ---- K13: exact posterior probabilities of candidate ancestral sequences ----

PhyloHMM::AncestralCandidateResult PhyloHMM::AncestralCandidatePosterior(const std::string& seed_seq, int node,
                                                                         const std::vector<std::string>& candidates,
                                                                         const std::vector<std::string>& with) {
  Require(!with.empty() || node == 0 || node == 1,
          "AncestralCandidatePosterior: node must be 0 (the seed's parent) or 1 (the MRCA)");
  Require(!candidates.empty(), "AncestralCandidatePosterior: no candidates");
  const int L = msa_.cols(), K = (int)candidates.size();
  const std::vector<uint8_t> bytes = EncodeSeqs(candidates, alphabet_, L);
  const std::vector<int32_t> with_tips = with.empty() ? std::vector<int32_t>() : WithTips(SeedTip(seed_seq), with);
  SeedLineage s = OpenSeedLineage(seed_seq);
  CheckHip(lh_family_set_ancestral_candidates(family_, K, bytes.data()), "lh_family_set_ancestral_candidates");
  AncestralCandidateResult res;
  res.log_cand.assign(K, 0.0);
  lh_ancestral_candidates_outputs outs{};
  outs.loglik = &res.loglik;
  outs.log_cand = res.log_cand.data();
  if (!with_tips.empty()) {
    const int32_t slot = CladeSlot(tree_.children.data(), tree_.n_tips, tree_.root, s.seed_tip, with_tips).slot;
    res.node = s.nodes[slot];
    CheckHip(lh_eval_ancestral_candidates_at_batch(family_, 1, tree_.n_tips, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(),
                                                   pi_.data(), &alpha_, num_rates_, s.nodes.data(), (int32_t)s.nodes.size(), &slot,
                                                   &outs),
             "lh_eval_ancestral_candidates_at_batch");
    return res;
  }
  res.node = node == 0 ? s.nodes.front() : s.nodes.back();
  CheckHip(lh_eval_ancestral_candidates_batch(family_, 1, tree_.n_tips, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(),
                                              pi_.data(), &alpha_, num_rates_, s.nodes.data(), (int32_t)s.nodes.size(), node, &outs),
           "lh_eval_ancestral_candidates_batch");
  return res;
}

void PhyloHMM::RunAncestralProbsPipeline(const std::string& input_path, const std::string& seed_seq, int node,
                                         const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                         double burnin_frac) {
  Require(node == 0 || node == 1, "the ancestral-probabilities pipeline: node must be 0 (the seed's parent) or 1 (the MRCA)");
  RunAncestralProbsPipelineAt(input_path, seed_seq, FixedLineageNode(node), candidates_path, output_prefix, num_rates, burnin_frac);
}

void PhyloHMM::RunAncestralProbsPipeline(const std::string& input_path, const std::string& seed_seq, const std::string& node_text,
                                         const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                         double burnin_frac) {
  RunAncestralProbsPipelineAt(input_path, seed_seq, ParseLineageNodeText(node_text), candidates_path, output_prefix, num_rates,
                              burnin_frac);
}

void PhyloHMM::RunAncestralProbsPipelineAt(const std::string& input_path, const std::string& seed_seq, const LineageNode& at,
                                           const std::string& candidates_path, const std::string& output_prefix, int num_rates,
                                           double burnin_frac) {
  // what can be refused without a device is refused first: the node (by the callers), the candidate file, the names to join
  // the seed with, then BeginPipeline's checks
  const int node = at.node;
  const int L = msa_.cols();
  AncestralProbsTable t;
  {
    NamedCandidates c = ReadNamedCandidateFile(candidates_path, L);
    t.names = std::move(c.names);
    t.seqs = std::move(c.seqs);
  }
  const std::size_t K = t.seqs.size();
  const std::vector<uint8_t> bytes = EncodeSeqs(t.seqs, alphabet_, L);
  const std::vector<int32_t> with_tips = at.at_clade() ? WithTips(SeedTip(seed_seq), at.with) : std::vector<int32_t>();
  const int seed_tip = BeginPipeline("ancestral probabilities", "posterior", burnin_frac, &seed_seq);
  CheckHip(lh_family_set_ancestral_candidates(family_, (int32_t)K, bytes.data()), "lh_family_set_ancestral_candidates");
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  // the rows' log_cand come back whole (K doubles each): a batch is bounded by at most 512 MiB of them
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * K));
  std::vector<double> log_cand;
  std::vector<int32_t> path_len(table.rows.size() - first, 0);
  std::vector<double> slots(at.at_clade() ? table.rows.size() - first : 0);
  const WeightedRows w = SumWeightedRows(
      "ancestral probabilities", table, input_path, first, PipelineBatch(fit), K, true,
      [&](const TableBatch& tb, std::size_t off, double* ll) {
        const DeviceBatch& b = tb.dev;
        const SeedChains sc = SeedChainsOf(tb, off, seed_tip, seed_seq, path_len.data() + (off - first));
        const std::vector<int32_t> slot = CladeSlotsOf(tb, seed_tip, with_tips);
        if (!slot.empty()) std::copy(slot.begin(), slot.end(), slots.begin() + (off - first));
        log_cand.resize((std::size_t)b.n * K);
        lh_ancestral_candidates_outputs outs{};
        outs.loglik = ll;
        outs.log_cand = log_cand.data();
        if (!slot.empty())
          CheckHip(lh_eval_ancestral_candidates_at_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(),
                                                         b.er.data(), b.pi.data(), b.alpha.data(), num_rates, sc.path.data(),
                                                         (int32_t)sc.P, slot.data(), &outs),
                   "lh_eval_ancestral_candidates_at_batch");
        else
          CheckHip(lh_eval_ancestral_candidates_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(),
                                                    b.er.data(), b.pi.data(), b.alpha.data(), num_rates, sc.path.data(),
                                                    (int32_t)sc.P, node, &outs),
                 "lh_eval_ancestral_candidates_batch");
        return [&](std::size_t i, double* row) {
          for (std::size_t k = 0; k < K; ++k) row[k] = std::exp(log_cand[i * K + k]);
        };
      });
  t.prob = w.acc.total;
  std::ofstream probs(output_prefix + ".probs.tsv"), rows(output_prefix + ".rows.tsv"), summary(output_prefix + ".summary.tsv");
  Require(probs.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteAncestralProbsTable(probs, t);
  WriteSeedRows(rows, first, w, path_len, "slot", at.at_clade() ? &slots : nullptr);
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
  std::size_t constrained = 0;
  for (const std::string& q : t.seqs) constrained += q.find('N') == std::string::npos;
  summary << "candidates\t" << K << "\ncandidates_constrained\t" << constrained << "\ncovered_mass\t" << Fmt17(CoveredMass(t))
          << "\n";
  if (at.at_clade()) {
    summary << "node\t" << at.text << "\n";
    WriteSlotSummary(summary, slots);
  }
}

// ---- K14: exact codon marginals of a node of a seed's lineage ----

namespace {

void CheckNodeAndFrame(const std::string& who, int node, int frame) {
  Require(node == 0 || node == 1, who + ": node must be 0 (the seed's parent) or 1 (the MRCA)");
  Require(frame >= 0 && frame <= 2, who + ": frame must be 0, 1 or 2");
}

PhyloHMM::NodeCodonsResult UnpackNodeCodons(int frame, std::size_t C, const double* codons, const double* change) {
  PhyloHMM::NodeCodonsResult r;
  r.frame = frame;
  r.node = -1;
  r.codons.resize(C);
  r.change.resize(C);
  for (std::size_t c = 0; c < C; ++c) {
    std::copy(codons + c * 64, codons + (c + 1) * 64, r.codons[c].begin());
    std::copy(change + c * 4, change + (c + 1) * 4, r.change[c].begin());
  }
  return r;
}

}  // namespace

PhyloHMM::NodeCodonsResult PhyloHMM::NodeCodonMarginals(const std::string& seed_seq, int node, int frame,
                                                        const std::vector<std::string>& with) {
  CheckNodeAndFrame("NodeCodonMarginals", with.empty() ? node : 0, frame);
  const std::vector<int32_t> with_tips = with.empty() ? std::vector<int32_t>() : WithTips(SeedTip(seed_seq), with);
  SeedLineage s = OpenSeedLineage(seed_seq);
  const CodonLayout lay = SetCodons(family_, frame);
  const std::size_t C = (std::size_t)lay.n_codons;
  std::vector<double> codons(C * 64), change(C * 4);
  double ll = 0.0;
  lh_node_codons_outputs outs{};
  outs.loglik = &ll;
  outs.codons = codons.data();
  outs.change = change.data();
  int32_t slot = node == 0 ? 0 : (int32_t)s.nodes.size() - 1;
  if (!with_tips.empty()) {
    slot = CladeSlot(tree_.children.data(), tree_.n_tips, tree_.root, s.seed_tip, with_tips).slot;
    CheckHip(lh_eval_node_codons_at_batch(family_, 1, tree_.n_tips, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(),
                                          pi_.data(), &alpha_, num_rates_, s.nodes.data(), (int32_t)s.nodes.size(), &slot, &outs),
             "lh_eval_node_codons_at_batch");
  } else {
    CheckHip(lh_eval_node_codons_batch(family_, 1, tree_.n_tips, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(), pi_.data(),
                                       &alpha_, num_rates_, s.nodes.data(), (int32_t)s.nodes.size(), node, &outs),
             "lh_eval_node_codons_batch");
  }
  NodeCodonsResult r = UnpackNodeCodons(frame, C, codons.data(), change.data());
  r.node = s.nodes[slot];
  r.loglik = ll;
  return r;
}

void PhyloHMM::WriteNodeCodonTable(std::ostream& o, const NodeCodonsResult& m) {
  static const char kBases[] = "ACGT";
  o << "codon\tfirst_site\tbases\tprobability\n";
  for (std::size_t c = 0; c < m.codons.size(); ++c)
    for (int i = 0; i < 64; ++i)
      if (m.codons[c][i] > 0.0)
        o << c << '\t' << (m.frame + 3 * c) << '\t' << kBases[i / 16] << kBases[(i / 4) % 4] << kBases[i % 4] << '\t'
          << Fmt17(m.codons[c][i]) << '\n';
}

void PhyloHMM::WriteNodeAminoAcidTable(std::ostream& o, const NodeCodonsResult& m) {
  static const std::string aa_of = [] {
    static const char kBases[] = "ACGT";
    std::string dna;
    for (int i = 0; i < 64; ++i) dna += {kBases[i / 16], kBases[(i / 4) % 4], kBases[i % 4]};
    return TranslateDna(dna);
  }();
  o << "codon\taa\tprobability\n";
  for (std::size_t c = 0; c < m.codons.size(); ++c) {
    std::map<char, double> p;
    for (int i = 0; i < 64; ++i)
      if (m.codons[c][i] > 0.0) p[aa_of[i]] += m.codons[c][i];
    for (const auto& kv : p) o << c << '\t' << kv.first << '\t' << Fmt17(kv.second) << '\n';
  }
}

void PhyloHMM::WriteChangeTable(std::ostream& o, const NodeCodonsResult& m) {
  o << "codon\tidentical\tsynonymous\treplacement\tundetermined\n";
  for (std::size_t c = 0; c < m.change.size(); ++c) {
    o << c;
    for (int k = 0; k < 4; ++k) o << '\t' << Fmt17(m.change[c][k]);
    o << '\n';
  }
}

void PhyloHMM::RunNodeCodonsPipeline(const std::string& input_path, const std::string& seed_seq, int node,
                                     const std::string& output_prefix, int num_rates, double burnin_frac, int frame) {
  CheckNodeAndFrame("the node-codons pipeline", node, frame);
  RunNodeCodonsPipelineAt(input_path, seed_seq, FixedLineageNode(node), output_prefix, num_rates, burnin_frac, frame);
}

void PhyloHMM::RunNodeCodonsPipeline(const std::string& input_path, const std::string& seed_seq, const std::string& node_text,
                                     const std::string& output_prefix, int num_rates, double burnin_frac, int frame) {
  RunNodeCodonsPipelineAt(input_path, seed_seq, ParseLineageNodeText(node_text), output_prefix, num_rates, burnin_frac, frame);
}

void PhyloHMM::RunNodeCodonsPipelineAt(const std::string& input_path, const std::string& seed_seq, const LineageNode& at,
                                       const std::string& output_prefix, int num_rates, double burnin_frac, int frame) {
  // what can be refused without a device is refused first: the node (by the callers) and the frame, the names to join the
  // seed with, then BeginPipeline's checks
  const int node = at.node;
  CheckNodeAndFrame("the node-codons pipeline", at.at_clade() ? 0 : node, frame);
  const std::vector<int32_t> with_tips = at.at_clade() ? WithTips(SeedTip(seed_seq), at.with) : std::vector<int32_t>();
  const int seed_tip = BeginPipeline("node codons", "codon", burnin_frac, &seed_seq);
  const CodonLayout lay = SetCodons(family_, frame);
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  const std::size_t C = (std::size_t)lay.n_codons, NC = C * 64, NH = C * 4;
  // the rows' tables come back whole (68 C doubles each): a batch is bounded by at most 512 MiB of them
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * std::max<std::size_t>(NC + NH, 1)));
  std::vector<double> codons, change;
  std::vector<int32_t> path_len(table.rows.size() - first, 0);
  std::vector<double> slots(at.at_clade() ? table.rows.size() - first : 0);
  const WeightedRows w = SumWeightedRows(
      "node codons", table, input_path, first, PipelineBatch(fit), NC + NH, true,
      [&](const TableBatch& tb, std::size_t off, double* ll) {
        const DeviceBatch& b = tb.dev;
        const SeedChains sc = SeedChainsOf(tb, off, seed_tip, seed_seq, path_len.data() + (off - first));
        const std::vector<int32_t> slot = CladeSlotsOf(tb, seed_tip, with_tips);
        if (!slot.empty()) std::copy(slot.begin(), slot.end(), slots.begin() + (off - first));
        codons.resize((std::size_t)b.n * NC);
        change.resize((std::size_t)b.n * NH);
        lh_node_codons_outputs outs{};
        outs.loglik = ll;
        outs.codons = codons.data();
        outs.change = change.data();
        if (!slot.empty())
          CheckHip(lh_eval_node_codons_at_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                                b.pi.data(), b.alpha.data(), num_rates, sc.path.data(), (int32_t)sc.P,
                                                slot.data(), &outs),
                   "lh_eval_node_codons_at_batch");
        else
          CheckHip(lh_eval_node_codons_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                           b.pi.data(), b.alpha.data(), num_rates, sc.path.data(), (int32_t)sc.P, node, &outs),
                 "lh_eval_node_codons_batch");
        return [&](std::size_t i, double* row) {
          std::copy(codons.begin() + i * NC, codons.begin() + (i + 1) * NC, row);
          std::copy(change.begin() + i * NH, change.begin() + (i + 1) * NH, row + NC);
        };
      });
  const NodeCodonsResult res = UnpackNodeCodons(frame, C, w.acc.total.data(), w.acc.total.data() + NC);
  std::ofstream cod(output_prefix + ".codons.tsv"), aa(output_prefix + ".aa.tsv"), chg(output_prefix + ".changes.tsv"),
      rows(output_prefix + ".rows.tsv"), summary(output_prefix + ".summary.tsv");
  Require(cod.good() && aa.good() && chg.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteNodeCodonTable(cod, res);
  WriteNodeAminoAcidTable(aa, res);
  WriteChangeTable(chg, res);
  WriteSeedRows(rows, first, w, path_len, "slot", at.at_clade() ? &slots : nullptr);
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
  double syn = 0.0, repl = 0.0;
  for (const auto& h : res.change) {
    syn += h[1];
    repl += h[2];
  }
  summary << "frame\t" << frame << "\nnode\t" << (at.at_clade() ? at.text : node == 0 ? "parent" : "mrca")
          << "\nexpected_synonymous\t" << Fmt17(syn) << "\nexpected_replacement\t" << Fmt17(repl) << "\n";
  if (at.at_clade()) WriteSlotSummary(summary, slots);
}

// ---- K15: exact amino-acid replacement posteriors along the edges of a seed's lineage ----

namespace {

void CheckFrame(const std::string& who, int frame) { Require(frame >= 0 && frame <= 2, who + ": frame must be 0, 1 or 2"); }

PhyloHMM::LineageReplacementsResult UnpackReplacements(int frame, std::size_t C, const double* cc, const double* aa, const double* sc) {
  PhyloHMM::LineageReplacementsResult r;
  r.frame = frame;
  r.codon_counts.resize(C);
  r.aa_counts.resize(C);
  r.seed_change.resize(C);
  for (std::size_t c = 0; c < C; ++c) {
    std::copy(cc + c * 4, cc + (c + 1) * 4, r.codon_counts[c].begin());
    std::copy(aa + c * 441, aa + (c + 1) * 441, r.aa_counts[c].begin());
    std::copy(sc + c * 3, sc + (c + 1) * 3, r.seed_change[c].begin());
  }
  return r;
}

}  // namespace

PhyloHMM::LineageReplacementsResult PhyloHMM::LineageReplacements(const std::string& seed_seq, int frame) {
  CheckFrame("LineageReplacements", frame);
  SeedLineage s = OpenSeedLineage(seed_seq);
  const CodonLayout lay = SetCodons(family_, frame);
  const std::size_t C = (std::size_t)lay.n_codons, P = s.nodes.size();
  std::vector<double> cc(C * 4), aa(C * 441), sc(C * 3), ec((P + 1) * C * 3), el((P + 1) * 2);
  double ll = 0.0;
  lh_codon_edges_outputs outs{};
  outs.loglik = &ll;
  outs.codon_counts = cc.data();
  outs.aa_counts = aa.data();
  outs.seed_change = sc.data();
  outs.edge_change = ec.data();
  outs.edge_load = el.data();
  CheckHip(lh_eval_codon_edges_batch(family_, 1, tree_.n_tips, s.depth, s.ops.data(), tree_.brlen.data(), er_.data(), pi_.data(),
                                     &alpha_, num_rates_, s.nodes.data(), (int32_t)P, s.seed_tip, &outs),
           "lh_eval_codon_edges_batch");
  LineageReplacementsResult r = UnpackReplacements(frame, C, cc.data(), aa.data(), sc.data());
  r.nodes = std::move(s.nodes);
  r.loglik = ll;
  r.edge_change = std::move(ec);
  r.edge_load.resize(P + 1);
  for (std::size_t e = 0; e <= P; ++e) r.edge_load[e] = {el[2 * e], el[2 * e + 1]};
  return r;
}

void PhyloHMM::WriteReplacementTable(std::ostream& o, const LineageReplacementsResult& m) {
  o << "codon\tfirst_site\tfrom\tto\texpected_edges\n";
  for (std::size_t c = 0; c < m.aa_counts.size(); ++c)
    for (int x = 0; x < 21; ++x)
      for (int y = 0; y < 21; ++y)
        if (x != y && m.aa_counts[c][x * 21 + y] > 0.0)
          o << c << '\t' << (m.frame + 3 * c) << '\t' << kAaSymbols[x] << '\t' << kAaSymbols[y] << '\t'
            << Fmt17(m.aa_counts[c][x * 21 + y]) << '\n';
}

void PhyloHMM::WriteCodonChangeTable(std::ostream& o, const LineageReplacementsResult& m) {
  o << "codon\tunchanged\tsynonymous\treplacement\tundetermined\n";
  for (std::size_t c = 0; c < m.codon_counts.size(); ++c) {
    o << c;
    for (int k = 0; k < 4; ++k) o << '\t' << Fmt17(m.codon_counts[c][k]);
    o << '\n';
  }
}

void PhyloHMM::WriteSeedChangeTable(std::ostream& o, const LineageReplacementsResult& m) {
  o << "codon\tunchanged\tsynonymous\treplacement\n";
  for (std::size_t c = 0; c < m.seed_change.size(); ++c) {
    o << c;
    for (int k = 0; k < 3; ++k) o << '\t' << Fmt17(m.seed_change[c][k]);
    o << '\n';
  }
}

void PhyloHMM::RunLineageReplacementsPipeline(const std::string& input_path, const std::string& seed_seq,
                                              const std::string& output_prefix, int num_rates, double burnin_frac, int frame) {
  // what can be refused without a device is refused first: the frame, then BeginPipeline's checks (burn-in, seed)
  CheckFrame("the lineage-replacements pipeline", frame);
  const int seed_tip = BeginPipeline("lineage replacements", "codon", burnin_frac, &seed_seq);
  const CodonLayout lay = SetCodons(family_, frame);
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t first = FirstUsedRow(table.rows.size(), burnin_frac);
  const std::size_t C = (std::size_t)lay.n_codons, NC = C * 4, NA = C * 441, NS = C * 3, NROW = NC + NA + NS;
  // the rows' tables come back whole (448 C doubles each): a batch is bounded by at most 512 MiB of them
  const std::size_t fit = std::max<std::size_t>(1, ((std::size_t)512 << 20) / (sizeof(double) * std::max<std::size_t>(NROW, 1)));
  std::vector<double> cc, aa, sc, syn(table.rows.size() - first, 0.0), repl(table.rows.size() - first, 0.0);
  std::vector<int32_t> path_len(table.rows.size() - first, 0);
  const WeightedRows w = SumWeightedRows(
      "lineage replacements", table, input_path, first, PipelineBatch(fit), NROW, true,
      [&](const TableBatch& tb, std::size_t off, double* ll) {
        const DeviceBatch& b = tb.dev;
        const std::size_t m = (std::size_t)b.n;
        const SeedChains chains = SeedChainsOf(tb, off, seed_tip, seed_seq, path_len.data() + (off - first));
        cc.resize(m * NC);
        aa.resize(m * NA);
        sc.resize(m * NS);
        lh_codon_edges_outputs outs{};
        outs.loglik = ll;
        outs.codon_counts = cc.data();
        outs.aa_counts = aa.data();
        outs.seed_change = sc.data();
        CheckHip(lh_eval_codon_edges_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                           b.pi.data(), b.alpha.data(), num_rates, chains.path.data(), (int32_t)chains.P, seed_tip,
                                           &outs),
                 "lh_eval_codon_edges_batch");
        for (std::size_t i = 0; i < m; ++i) {  // the row's expected changes over its lineage, the codons in order
          double s1 = 0.0, s2 = 0.0;
          for (std::size_t c = 0; c < C; ++c) {
            s1 += cc[i * NC + c * 4 + 1];
            s2 += cc[i * NC + c * 4 + 2];
          }
          syn[off - first + i] = s1;
          repl[off - first + i] = s2;
        }
        return [&](std::size_t i, double* row) {
          std::copy(cc.begin() + i * NC, cc.begin() + (i + 1) * NC, row);
          std::copy(aa.begin() + i * NA, aa.begin() + (i + 1) * NA, row + NC);
          std::copy(sc.begin() + i * NS, sc.begin() + (i + 1) * NS, row + NC + NA);
        };
      });
  const double* t = w.acc.total.data();
  const LineageReplacementsResult res = UnpackReplacements(frame, C, t, t + NC, t + NC + NA);
  std::ofstream rep(output_prefix + ".replacements.tsv"), chg(output_prefix + ".codon_changes.tsv"),
      seed(output_prefix + ".seed_edge.tsv"), rows(output_prefix + ".rows.tsv"), summary(output_prefix + ".summary.tsv");
  Require(rep.good() && chg.good() && seed.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  WriteReplacementTable(rep, res);
  WriteCodonChangeTable(chg, res);
  WriteSeedChangeTable(seed, res);
  rows << "row\tweight\tchain_length\texpected_synonymous\texpected_replacement\n";
  for (std::size_t u = 0; u < w.lw.size(); ++u)
    rows << (first + u) << '\t' << Fmt17(w.weight(u)) << '\t' << path_len[u] << '\t' << Fmt17(syn[u]) << '\t' << Fmt17(repl[u])
         << '\n';
  WriteSummary(summary, w.used(), w.skipped, Fmt17(w.acc.KishEss()));
  double s1 = 0.0, s2 = 0.0;
  for (const auto& h : res.codon_counts) {
    s1 += h[1];
    s2 += h[2];
  }
  summary << "frame\t" << frame << "\nexpected_synonymous\t" << Fmt17(s1) << "\nexpected_replacement\t" << Fmt17(s2) << "\n";
}

// Pass 1 draws every used row's naive sequence with the std::mt19937 words RunPipeline gives that row (row r: words
// r * RawDrawsPerSample() on), on the device where the family has its sampler tables: K4's states become bytes and a
// hash there (K6c), the host maps hashes to candidate ids in row order and the device checks every row's bytes against
// its candidate's (lh_draws_resolve); rows whose hash collides with another sequence's are resolved by their bytes.
// Candidates are numbered by first appearance at the end, so both paths, every batch size and every hash width give
// the same ids.  Pass 2 scores the candidates exactly (K6b) and combines the batches as RunMarginalsPipeline does.
void PhyloHMM::RunNaiveProbsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                     double burnin_frac, const std::string& candidates_path, int max_candidates) {
  Require(devices_.size() <= 1, "the naive-probabilities pipeline runs on one device: --devices may list only one");
  Require(burnin_frac >= 0.0 && burnin_frac < 1.0, "burn-in fraction must be in [0, 1)");
  Require(max_candidates >= 1 && max_candidates <= 65536, "max-candidates must be in 1 .. 65536");
  CreateFamily();
  // stage times on stderr (LH_PIPELINE_TIMING): table parsing, device calls, host collection, per pass
  const bool timing = host_options().pipeline_timing;
  double p1_parse = 0, p1_dev = 0, p1_collect = 0, p1_total = 0, p2_prior = 0, p2_parse = 0, p2_dev = 0, p2_total = 0;
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t N = table.rows.size();
  const std::size_t first = (std::size_t)std::floor(burnin_frac * (double)N);
  const std::size_t U = N - first;  // rows after the burn-in
  const int L = msa_.cols();
  const std::size_t kBatch = host_options().pipeline_batch > 0 ? (std::size_t)host_options().pipeline_batch : 49152;
  NaiveProbsTable t;
  std::vector<int32_t> row_id;  // pass 1: candidate of every row after the burn-in (-1: non-finite row or dropped)
  std::vector<double> ll1;
  int64_t draws_distinct = -1, dropped = 0;
  const auto t_p1 = SteadyNow();
  if (candidates_path.empty()) {
    const int raw = RawDrawsPerSample();
    row_id.assign(U, -1);
    ll1.assign(U, 0.0);
    std::vector<std::string> distinct;  // by pass-1 id
    if (device_sampler_) {
      CheckHip(lh_draws_reset(family_), "lh_draws_reset");
      SeqInterner interner(family_, lh_draws_resolve, lh_draws_rows_read, L, "naive-probabilities pipeline");
      std::mt19937 word_rng = rng_;
      word_rng.discard((unsigned long long)first * (unsigned long long)raw);
      for (std::size_t off = first; off < N; off += kBatch) {
        const std::size_t m = std::min(kBatch, N - off);
        const auto t0 = SteadyNow();
        TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
        const DeviceBatch& b = tb.dev;
        const auto t1 = SteadyNow();
        p1_parse += Seconds(t0, t1);
        std::vector<uint32_t> words(m * (std::size_t)raw);
        for (uint32_t& x : words) x = (uint32_t)word_rng();
        std::vector<uint64_t> hash(m);
        double* ll = ll1.data() + (off - first);
        CheckHip(lh_eval_draw_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                    b.pi.data(), b.alpha.data(), num_rates, words.data(), ll, hash.data(), nullptr),
                 "lh_eval_draw_batch");
        const auto t2 = SteadyNow();
        p1_dev += Seconds(t1, t2);
        std::vector<uint8_t> finite(m);
        for (std::size_t i = 0; i < m; ++i) finite[i] = std::isfinite(ll[i] - tb.lik[i]);
        interner.Assign(m, hash.data(), finite.data(), row_id.data() + (off - first));
        p1_collect += Seconds(t2, SteadyNow());
      }
      int32_t Ks = 0;
      CheckHip(lh_draws_candidates_read(family_, &Ks, nullptr), "lh_draws_candidates_read");
      std::vector<uint8_t> store((std::size_t)Ks * L);
      CheckHip(lh_draws_candidates_read(family_, &Ks, store.data()), "lh_draws_candidates_read");
      // renumber by first appearance
      std::vector<int32_t> remap(Ks, -1);
      for (int32_t& id : row_id) {
        if (id < 0) continue;
        if (remap[id] < 0) {
          remap[id] = (int32_t)distinct.size();
          distinct.push_back(DecodeBases(store.data() + (std::size_t)id * L, (std::size_t)L, alphabet_));
        }
        id = remap[id];
      }
    } else {
      // the host sampler (LH_HOST_SAMPLING, or no device sampler tables): forward arrays to the host, HMM::SampleRow
      EnsureSamplingLists();
      std::mt19937 rng = rng_;
      rng.discard((unsigned long long)first * (unsigned long long)raw);
      std::unordered_map<std::string, int32_t> ids;
      const std::size_t FS = lh_forward_size(family_), SS = lh_scaler_size(family_);
      const std::size_t kSub = std::min<std::size_t>(kBatch, 1024);
      std::vector<double> fwd(kSub * FS);
      std::vector<int32_t> sco(kSub * SS);
      RowSampler s;
      for (std::size_t off = first; off < N; off += kSub) {
        const std::size_t m = std::min(kSub, N - off);
        const auto t0 = SteadyNow();
        TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
        const DeviceBatch& b = tb.dev;
        const auto t1 = SteadyNow();
        p1_parse += Seconds(t0, t1);
        double* ll = ll1.data() + (off - first);
        lh_eval_outputs outs{nullptr, nullptr, fwd.data(), sco.data()};
        CheckHip(lh_eval_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(), b.pi.data(),
                               b.alpha.data(), num_rates, ll, &outs),
                 "lh_eval_batch");
        const auto t2 = SteadyNow();
        p1_dev += Seconds(t1, t2);
        for (std::size_t i = 0; i < m; ++i) {
          if (!std::isfinite(ll[i] - tb.lik[i])) {
            rng.discard((unsigned long long)raw);
            continue;
          }
          SampleRow(s, fwd.data() + i * FS, rng);
          const auto r = ids.emplace(s.naive_seq, (int32_t)distinct.size());
          if (r.second) distinct.push_back(s.naive_seq);
          row_id[off - first + i] = r.first->second;
        }
        p1_collect += Seconds(t2, SteadyNow());
      }
    }
    // counts, and the limit: the most drawn, ties by first appearance, kept in first-appearance order
    std::vector<int64_t> count(distinct.size(), 0);
    for (int32_t id : row_id)
      if (id >= 0) ++count[id];
    draws_distinct = (int64_t)distinct.size();
    Require(!distinct.empty(), "naive-probabilities pipeline: no row with a finite weight");
    std::vector<int32_t> keep(distinct.size());
    for (std::size_t k = 0; k < keep.size(); ++k) keep[k] = (int32_t)k;
    if ((int64_t)distinct.size() > max_candidates) {
      std::stable_sort(keep.begin(), keep.end(), [&](int32_t a, int32_t b) { return count[a] > count[b]; });
      keep.resize(max_candidates);
      std::sort(keep.begin(), keep.end());
      dropped = draws_distinct - max_candidates;
    }
    std::vector<int32_t> new_id(distinct.size(), -1);
    for (std::size_t k = 0; k < keep.size(); ++k) {
      new_id[keep[k]] = (int32_t)k;
      t.seqs.push_back(distinct[keep[k]]);
      t.count.push_back(count[keep[k]]);
    }
    for (int32_t& id : row_id)
      if (id >= 0) id = new_id[id];
    t.sampled = true;
  } else {
    t.seqs = ReadCandidateFile(candidates_path, L);
  }

  p1_total = Seconds(t_p1, SteadyNow());
  // pass 2: exact probabilities
  const auto t_p2 = SteadyNow();
  const int K = (int)t.seqs.size();
  const std::vector<uint8_t> bytes = EncodeSeqs(t.seqs, alphabet_, L);
  t.log_prior.assign(K, 0.0);
  CheckHip(lh_family_set_candidates(family_, K, bytes.data(), t.log_prior.data()), "lh_family_set_candidates");
  p2_prior = Seconds(t_p2, SteadyNow());
  WeightedSums acc((std::size_t)K);
  std::vector<double> wsum(K), lw(U);
  std::size_t skipped = 0;
  for (std::size_t off = first; off < N; off += kBatch) {
    const std::size_t m = std::min(kBatch, N - off);
    const auto t0 = SteadyNow();
    TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
    const DeviceBatch& b = tb.dev;
    const auto t1 = SteadyNow();
    p2_parse += Seconds(t0, t1);
    std::vector<double> ll(m);
    double st[3];
    lh_candidate_outputs outs{tb.lik.data(), ll.data(), nullptr, wsum.data(), st};
    CheckHip(lh_eval_candidates_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                      b.pi.data(), b.alpha.data(), num_rates, &outs),
             "lh_eval_candidates_batch");
    p2_dev += Seconds(t1, SteadyNow());
    for (std::size_t i = 0; i < m; ++i) {
      lw[off - first + i] = ll[i] - tb.lik[i];
      if (!std::isfinite(lw[off - first + i])) ++skipped;
      if (!ll1.empty() && std::memcmp(&ll[i], &ll1[off - first + i], sizeof(double)) != 0)
        throw std::runtime_error("naive-probabilities pipeline: the two passes' log-likelihoods differ at row " +
                                 std::to_string(off + i));
    }
    acc.Add(wsum.data(), st);
  }
  Require(acc.s1 > 0.0, "naive-probabilities pipeline: no row with a finite weight");
  acc.Normalise();
  p2_total = Seconds(t_p2, SteadyNow());
  if (timing)
    std::fprintf(stderr,
                 "[RunNaiveProbsPipeline] %zu rows; pass 1 (%s): parse %.4f s, device %.4f s, collect %.4f s, total %.4f s; "
                 "pass 2 (%d candidates): priors %.4f s, parse %.4f s, device %.4f s, total %.4f s\n",
                 U, !candidates_path.empty() ? "skipped" : device_sampler_ ? "device draws" : "host draws", p1_parse, p1_dev,
                 p1_collect, p1_total, K, p2_prior, p2_parse, p2_dev, p2_total);
  t.prob = acc.total;
  double covered = 0.0;
  for (int k = 0; k < K; ++k) covered += t.prob[k];
  if (t.sampled) {  // self-normalised sampled frequencies, weights as K5 / K6b form them, summed in row order
    double lmax = -INFINITY;
    for (double x : lw)
      if (std::isfinite(x)) lmax = std::max(lmax, x);
    std::vector<double> f(K, 0.0);
    double W = 0.0;
    for (std::size_t i = 0; i < U; ++i) {
      if (!std::isfinite(lw[i])) continue;
      const double w = std::exp(lw[i] - lmax);
      W += w;
      if (row_id[i] >= 0) f[row_id[i]] += w;
    }
    t.freq.resize(K);
    for (int k = 0; k < K; ++k) t.freq[k] = f[k] / W;
  }
  std::ofstream naive(output_prefix + ".naive.tsv"), aa(output_prefix + ".aa.fasta"), dnamap(output_prefix + ".dnamap"),
      summary(output_prefix + ".summary.tsv");
  Require(naive.good() && aa.good() && dnamap.good() && summary.good(), "Can't write " + output_prefix + ".*");
  WriteNaiveTable(naive, t);
  WriteAaFasta(aa, t);
  WriteDnaMap(dnamap, t);
  char buf[64], cov[64];
  std::snprintf(buf, sizeof buf, "%.17g", acc.KishEss());
  std::snprintf(cov, sizeof cov, "%.17g", covered);
  summary << "key\tvalue\nrows_used\t" << (U - skipped) << "\nrows_skipped_nonfinite\t" << skipped << "\nkish_ess\t" << buf
          << "\ndraws_distinct\t" << (draws_distinct < 0 ? std::string("NA") : std::to_string(draws_distinct))
          << "\ncandidates\t" << K << "\ncandidates_dropped\t" << dropped << "\ncovered_mass\t" << cov << "\n";
}

// Pass 1: K8 per batch; the host interns the rows' state vectors.  Pass 2: the kept paths are registered as candidates
// with their path priors and scored on every row by K6b; the host adds w_i exp(log_cand[i][k]) up in row order against the
// largest log-weight of the whole table (known from pass 1), so no sum depends on how the table was cut into batches.
void PhyloHMM::RunAnnotationsPipeline(const std::string& input_path, const std::string& output_prefix, int num_rates,
                                      double burnin_frac, int max_candidates) {
  Require(devices_.size() <= 1, "the annotations pipeline runs on one device: --devices may list only one");
  Require(burnin_frac >= 0.0 && burnin_frac < 1.0, "burn-in fraction must be in [0, 1)");
  Require(max_candidates >= 1 && max_candidates <= 65536, "max-candidates must be in 1 .. 65536");
  CreateFamily();
  Require(device_sampler_, "the family has no device sampler tables (needed by the Viterbi kernel)");
  TsvTable table = TsvTable::OpenRevBayesTable(input_path);
  const std::size_t N = table.rows.size();
  const std::size_t first = (std::size_t)std::floor(burnin_frac * (double)N);
  const std::size_t U = N - first;  // rows after the burn-in
  const std::size_t S = (std::size_t)lh_sample_states(family_);
  const std::size_t kBatch = host_options().pipeline_batch > 0 ? (std::size_t)host_options().pipeline_batch : 49152;

  // pass 1
  std::vector<double> ll1(U), lw(U), post(U);
  std::vector<int32_t> row_path(U, -1);            // the row's MAP path by first appearance (-1: skipped row)
  std::vector<std::vector<int32_t>> paths;         // distinct paths in first-appearance order
  std::unordered_map<std::string, int32_t> ids;    // by the bytes of the state vector
  std::size_t skipped = 0;
  for (std::size_t off = first; off < N; off += kBatch) {
    const std::size_t m = std::min(kBatch, N - off);
    TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
    const DeviceBatch& b = tb.dev;
    std::vector<int32_t> states(m * S);
    std::vector<double> lp(m);
    lh_viterbi_outputs outs{nullptr, ll1.data() + (off - first), states.data(), lp.data(), nullptr};
    CheckHip(lh_eval_viterbi_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                   b.pi.data(), b.alpha.data(), num_rates, &outs),
             "lh_eval_viterbi_batch");
    for (std::size_t i = 0; i < m; ++i) {
      const std::size_t u = off - first + i;
      lw[u] = ll1[u] - tb.lik[i];
      post[u] = lp[i] - ll1[u];
      if (!std::isfinite(lw[u]) || states[i * S] < 0) {  // (no path without a finite log-likelihood, and the reverse)
        ++skipped;
        continue;
      }
      const std::string key(reinterpret_cast<const char*>(states.data() + i * S), S * sizeof(int32_t));
      const auto r = ids.emplace(key, (int32_t)paths.size());
      if (r.second) paths.emplace_back(states.begin() + i * S, states.begin() + (i + 1) * S);
      row_path[u] = r.first->second;
    }
  }
  Require(!paths.empty(), "annotations pipeline: no row with a finite weight");
  double lmax = -INFINITY;
  for (std::size_t u = 0; u < U; ++u)
    if (row_path[u] >= 0) lmax = std::max(lmax, lw[u]);
  std::vector<double> w(U, 0.0), map_weight(paths.size(), 0.0);
  std::vector<int64_t> map_rows(paths.size(), 0);
  double s1 = 0.0, s2 = 0.0;
  for (std::size_t u = 0; u < U; ++u) {
    if (row_path[u] < 0) continue;
    w[u] = std::exp(lw[u] - lmax);
    s1 += w[u];
    s2 += w[u] * w[u];
    map_weight[row_path[u]] += w[u];
    ++map_rows[row_path[u]];
  }
  // the paths of largest MAP weight, ties by first appearance, kept in first-appearance order
  std::vector<int32_t> keep(paths.size());
  for (std::size_t k = 0; k < keep.size(); ++k) keep[k] = (int32_t)k;
  if ((int64_t)paths.size() > max_candidates) {
    std::stable_sort(keep.begin(), keep.end(), [&](int32_t a, int32_t b) { return map_weight[a] > map_weight[b]; });
    keep.resize(max_candidates);
    std::sort(keep.begin(), keep.end());
  }
  const int K = (int)keep.size();
  std::vector<int32_t> cand_of_path(paths.size(), -1), cand_states((std::size_t)K * S);
  for (int k = 0; k < K; ++k) {
    cand_of_path[keep[k]] = k;
    std::copy(paths[keep[k]].begin(), paths[keep[k]].end(), cand_states.begin() + (std::size_t)k * S);
  }

  // pass 2
  std::vector<double> log_prior(K), prob(K, 0.0);
  CheckHip(lh_family_set_candidate_paths(family_, K, cand_states.data(), log_prior.data()), "lh_family_set_candidate_paths");
  const std::size_t kScore = std::max<std::size_t>(1, std::min(kBatch, ((std::size_t)32 << 20) / (std::size_t)K));  // rows per call: 256 MB of log_cand
  std::vector<double> lc;
  for (std::size_t off = first; off < N; off += kScore) {
    const std::size_t m = std::min(kScore, N - off);
    TableBatch tb = FlattenTable(table, off, off + m, false, true, input_path);
    const DeviceBatch& b = tb.dev;
    std::vector<double> ll(m);
    lc.resize(m * (std::size_t)K);
    lh_candidate_outputs outs{nullptr, ll.data(), lc.data(), nullptr, nullptr};
    CheckHip(lh_eval_candidates_batch(family_, b.n, b.n_tips, b.max_depth, b.ops.data(), b.brlen.data(), b.er.data(),
                                      b.pi.data(), b.alpha.data(), num_rates, &outs),
             "lh_eval_candidates_batch");
    for (std::size_t i = 0; i < m; ++i) {
      const std::size_t u = off - first + i;
      if (std::memcmp(&ll[i], &ll1[u], sizeof(double)) != 0)
        throw std::runtime_error("annotations pipeline: the two passes' log-likelihoods differ at row " + std::to_string(off + i));
      if (row_path[u] < 0) continue;
      const double* row = lc.data() + i * (std::size_t)K;
      for (int k = 0; k < K; ++k) prob[k] += w[u] * std::exp(row[k]);
    }
  }
  for (double& v : prob) v /= s1;

  // paths whose annotation columns format alike are one annotation
  struct Annotation {
    std::string columns;
    double prob = 0.0, prior = 0.0, weight = 0.0;
    int64_t rows = 0;
  };
  std::vector<Annotation> ann;
  std::unordered_map<std::string, int32_t> ann_ids;
  std::vector<int32_t> ann_of_cand(K);
  RowSampler rs;
  for (int k = 0; k < K; ++k) {
    ApplySampledStates(rs, cand_states.data() + (std::size_t)k * S);
    std::string cols;
    AppendAnnotationColumns(cols, rs);
    const auto r = ann_ids.emplace(cols, (int32_t)ann.size());
    if (r.second) {
      ann.emplace_back();
      ann.back().columns = cols;
    }
    Annotation& a = ann[r.first->second];
    a.prob += prob[k];
    a.prior += std::exp(log_prior[k]);
    a.weight += map_weight[keep[k]];
    a.rows += map_rows[keep[k]];
    ann_of_cand[k] = r.first->second;
  }
  std::vector<int32_t> order(ann.size()), rank_of(ann.size());
  for (std::size_t k = 0; k < order.size(); ++k) order[k] = (int32_t)k;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return ann[a].prob > ann[b].prob; });
  for (std::size_t r = 0; r < order.size(); ++r) rank_of[order[r]] = (int32_t)r + 1;
  char buf[64];
  auto num = [&](double v) {
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return std::string(buf);
  };
  std::ofstream all(output_prefix + ".annotations.tsv"), best(output_prefix + ".best.tsv"), rows(output_prefix + ".rows.tsv"),
      summary(output_prefix + ".summary.tsv");
  Require(all.good() && best.good() && rows.good() && summary.good(), "Can't write " + output_prefix + ".*.tsv");
  const std::string head = "rank\tprobability\tlog_probability\tlog_prior\tmap_rows\tmap_weight_share\t" + AnnotationHeader() + "\n";
  all << head;
  best << head;
  double covered = 0.0;
  for (std::size_t r = 0; r < order.size(); ++r) {
    const Annotation& a = ann[order[r]];
    covered += a.prob;
    const std::string line = std::to_string(r + 1) + '\t' + num(a.prob) + '\t' + num(std::log(a.prob)) + '\t' +
                             num(std::log(a.prior)) + '\t' + std::to_string(a.rows) + '\t' + num(a.weight / s1) + '\t' +
                             a.columns + '\n';
    all << line;
    if (r == 0) best << line;
  }
  rows << "row\tlh_loglik\tlog_weight\tlog_path_posterior\tannotation\n";
  for (std::size_t u = 0; u < U; ++u) {
    const int32_t c = row_path[u] >= 0 ? cand_of_path[row_path[u]] : -1;
    rows << (first + u) << '\t' << num(ll1[u]) << '\t' << num(lw[u]) << '\t' << num(post[u]) << '\t'
         << (c >= 0 ? std::to_string(rank_of[ann_of_cand[c]]) : std::string("NA")) << '\n';
  }
  summary << "key\tvalue\nrows_used\t" << (U - skipped) << "\nrows_skipped_nonfinite\t" << skipped << "\ndistinct_paths\t"
          << paths.size() << "\npaths_scored\t" << K << "\nannotations\t" << ann.size() << "\ncovered_mass\t" << num(covered)
          << "\nkish_ess\t" << num(s1 * s1 / s2) << "\n";
}

}  // namespace linearham
