// C ABI of liblinearham_hip.so (see include/linearham_amd.h): family upload, tree scheduling,
// batched evaluation.  Host-side code only; the kernels live in lh_model/lh_prune/lh_forward.hip.
#include <algorithm>
#include <array>
#include <map>
#include <cstdio>
#include <cstring>
#include <functional>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "lh_device.h"

namespace lh {
const DebugOptions& debug_options() {
  static const DebugOptions opts = [] {
    DebugOptions o;
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    auto num = [](const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    o.chunk = std::max(256, num("LH_CHUNK", o.chunk));
    o.host_sub = std::max(256, num("LH_HOST_SUB", o.host_sub));
    o.eval_split = std::min(8, std::max(0, num("LH_EVAL_SPLIT", o.eval_split)));
    o.k0_serial = set("LH_K0_SERIAL");
    o.eval_fwd_priority = std::min(1, num("LH_EVAL_FWD_PRIORITY", o.eval_fwd_priority));
    o.k2b_no_pair = set("LH_K2B_NO_PAIR");
    o.k2b_vd_single = set("LH_K2B_VD_SINGLE");
    o.k2b_dj_pair = set("LH_K2B_DJ_PAIR");
    o.sample_timing = set("LH_SAMPLE_TIMING");
    o.k4_no_save = set("LH_K4_NO_SAVE");
    o.k1_tile_cap = num("LH_K1_TILE_CAP", 0);
    o.k1_cxx_walk = set("LH_K1_CXX_WALK");
    o.k1_tables = set("LH_K1_TABLES");
    o.k1_stack = set("LH_K1_STACK");
    o.k1_no_tables = set("LH_K1_NO_TABLES");
    o.k1_segments = set("LH_K1_SEGMENTS");
    o.k1_seg_waves = num("LH_K1_SEG_WAVES", o.k1_seg_waves);
    o.k1_no_fuse = set("LH_K1_NO_FUSE");
    o.codon_blocks = std::max(1, num("LH_CODON_BLOCKS", o.codon_blocks));
    o.events_blocks = std::max(1, num("LH_EVENTS_BLOCKS", o.events_blocks));
    o.anc_out_mb = std::max(1, num("LH_ANC_OUT_MB", o.anc_out_mb));
    o.edge_out_mb = std::max(1, num("LH_EDGE_OUT_MB", o.edge_out_mb));
    o.anc_pairs = std::max(0, num("LH_ANC_PAIRS", o.anc_pairs));
    o.codon_edges_mb = std::max(0, num("LH_CODON_EDGES_MB", o.codon_edges_mb));
    o.collect_hash_bits = std::min(64, std::max(1, num("LH_COLLECT_HASH_BITS", o.collect_hash_bits)));
    return o;
  }();
  return opts;
}
}  // namespace lh

namespace {

thread_local std::string g_error;

int fail(const std::string& msg) {
  g_error = msg;
  return 1;
}

#define LH_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

// A grow-only buffer of device memory or (Pinned) page-locked host memory.  ensure() leaves at least 64 bytes, so that an
// empty request still gets an address.  Growing first waits for the device: queued work may still read the old allocation.
// Buffers only grow, so the steady state neither allocates nor waits.
template <bool Pinned>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { release(); }
  int ensure(size_t bytes) {
    bytes = std::max<size_t>(bytes, 64);
    if (bytes <= cap_) return 0;
    if (p_) {
      LH_HIP(hipDeviceSynchronize());
      release();
    }
    LH_HIP(Pinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes));
    cap_ = bytes;
    return 0;
  }
  template <typename T = void>
  T* get() const { return static_cast<T*>(p_); }

 private:
  void release() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    cap_ = 0;
  }
  void* p_ = nullptr;
  size_t cap_ = 0;
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// lh_profile_enable's kernel times: HIP events at the Stages + 1 boundaries of every profiled launch group, summed and
// reset by a read.  A launch group that runs in sub-batches on several streams (eval_group_split) is recorded as spans
// instead: a pair of events around every piece of a stage, on the stream that piece runs on; a stage's time is then the
// sum of its spans, and the stages' times overlap.
template <int Stages>
class KernelTimer {
 public:
  KernelTimer() = default;
  KernelTimer(const KernelTimer&) = delete;
  KernelTimer& operator=(const KernelTimer&) = delete;
  ~KernelTimer() {
    for (Events& es : done_) destroy(es);
    destroy(open_);
    destroy(done_spans_);
    destroy(open_spans_);
  }
  // begin() records boundary 0 on `s`, mark(k) boundary k, end() the last one
  int begin(hipStream_t s) {
    destroy(open_);  // (a launch group that failed leaves its set open)
    for (hipEvent_t& e : open_) LH_HIP(hipEventCreate(&e));
    return mark(0, s);
  }
  int mark(int k, hipStream_t s) {
    LH_HIP(hipEventRecord(open_[k], s));
    return 0;
  }
  int end(hipStream_t s) {
    if (mark(Stages, s)) return 1;
    done_.push_back(std::exchange(open_, Events{}));
    return 0;
  }
  // The span form of one launch group: begin_spans(), then span_begin(stage, s) ... span_end(s) around every piece,
  // end_spans().
  void begin_spans() {
    destroy(open_);
    destroy(open_spans_);
  }
  int span_begin(int stage, hipStream_t s) {
    Span sp{stage, nullptr, nullptr};
    LH_HIP(hipEventCreate(&sp.a));
    open_spans_.push_back(sp);
    LH_HIP(hipEventCreate(&open_spans_.back().b));
    LH_HIP(hipEventRecord(sp.a, s));
    return 0;
  }
  int span_end(hipStream_t s) {
    LH_HIP(hipEventRecord(open_spans_.back().b, s));
    return 0;
  }
  void end_spans() {
    done_spans_.insert(done_spans_.end(), open_spans_.begin(), open_spans_.end());
    open_spans_.clear();
    ++span_groups_;
  }
  // Waits for the launch groups recorded since the last read and hands out their times per stage (ms[Stages]) and their
  // number; either may be null.
  int read(double* ms, int64_t* launches) {
    double sum[Stages] = {};
    hipError_t e = hipSuccess;
    for (Span& sp : done_spans_) {
      if (e == hipSuccess) e = hipEventSynchronize(sp.b);
      float t = 0;
      if (e == hipSuccess) e = hipEventElapsedTime(&t, sp.a, sp.b);
      sum[sp.stage] += t;
    }
    destroy(done_spans_);
    for (Events& es : done_) {
      if (e == hipSuccess) e = hipEventSynchronize(es[Stages]);
      for (int k = 0; k < Stages && e == hipSuccess; ++k) {
        float t = 0;
        e = hipEventElapsedTime(&t, es[k], es[k + 1]);
        sum[k] += t;
      }
      destroy(es);
    }
    const int64_t n = (int64_t)done_.size() + std::exchange(span_groups_, 0);
    done_.clear();
    LH_HIP(e);
    if (ms) std::copy(sum, sum + Stages, ms);
    if (launches) *launches = n;
    return 0;
  }

 private:
  using Events = std::array<hipEvent_t, Stages + 1>;
  static void destroy(Events& es) {
    for (hipEvent_t& e : es)
      if (e) (void)hipEventDestroy(std::exchange(e, nullptr));
  }
  struct Span {
    int stage;
    hipEvent_t a, b;
  };
  static void destroy(std::vector<Span>& v) {
    for (Span& sp : v) {
      if (sp.a) (void)hipEventDestroy(sp.a);
      if (sp.b) (void)hipEventDestroy(sp.b);
    }
    v.clear();
  }
  std::vector<Events> done_;
  Events open_{};
  std::vector<Span> done_spans_, open_spans_;
  int64_t span_groups_ = 0;
};

struct Workspace {  // K0-K2's scratch (ensure_workspace)
  DevBuf rates, eig, site_lik, site_scal;
  DevBuf scratch, wops, wlen, tabs, hdr;  // K0c's checked / rewritten schedules and K1's scratch area
  lh::PruneWs prune{};                    // the same five as launch_prune takes them; err_flag is the family's
};

struct ForwardWs {  // K2a -> K2b hand-off (run_forward)
  DevBuf gem, jem, dxf, gcnt, jrs, dxc;
};

struct AsrWs {  // K3's scratch
  DevBuf clv;
  DevBuf rates;   // lh_eval_lineage_batch: K0a's rates of the whole batch when the caller does not ask for them
  DevBuf choice;  // K3a -> K3b when the caller does not ask for the rate categories
  DevBuf desc;    // K3s -> K3b schedule descriptors
};

struct AncestralWs {  // K11's scratch (lh::AncWs) and the arrays its callers do not hand in
  DevBuf clv, part, tvec, rho, chain, plen, desc;
  DevBuf naive_prob, path, slot;  // the host-pointer forms' device copies
  DevBuf marg, rate_post;
  // lh_eval_ancestral_batch: K11a's table (built by the first call), its output, and the reduction's arrays
  bool have_table = false;
  DevBuf sb_off, sb_idx, site_base;
  DevBuf loglik, rates, ends, ll_used, weights, stats, partial_e, partial_r;
  DevBuf out_wsum, out_wrate;
};

struct EdgesWs {  // K12's scratch beside K11's (lh::SubWs) and the outputs its callers do not take
  DevBuf cc, ne, se, el, edge;
  DevBuf out_edge, out_ne, out_cc, out_se, out_el, out_wcc, out_wse, out_wne;
  DevBuf partial_c, partial_s, partial_n;  // the weighted reduction's slabs
};

struct AncProbsWs {  // K13 (lh_ancestral_probs.hip)
  int32_t K = 0;               // 0: lh_family_set_ancestral_candidates has not been called (or its last call failed)
  DevBuf seqs;                 // [K][L]
  DevBuf part, table;          // K13b's partial tables and K13m's tables of a launch group
  DevBuf em;                   // the group's emissions in caller columns, K2a's em_out
  DevBuf pair_em, pair_ll, open_ll;  // a group of pairs: its emissions and sweeps; the rows' own sweeps
  DevBuf prob, partial;        // exp(log_cand) of the batch and the weighted reduction's slabs
  DevBuf out_cond, out_log_cand, out_wsum;  // the host-pointer form's device copies
};

struct NodeCodonsWs {  // K14 (lh_node_codon.hip)
  bool have = false;  // the tables are built: by the first call after lh_family_set_codons
  lh::NodeCodonTables tab{};
  DevBuf codon_src, germ, codes;
  DevBuf windows, genes, naive;  // a launch group's K9 outputs and the naive codon posteriors of every codon
  DevBuf zero;                   // the given-rates form: the all-zero naive_prob K11r is handed (its output is not read)
  DevBuf codons, change, partial_c, partial_h;  // the batch's rows where the caller does not take them; the reduction's slabs
  DevBuf out_codons, out_change, out_wcodons, out_wchange;  // the host-pointer form's device copies
};

struct CodonEdgesWs {  // K15 (lh_codon_edges.hip); K9's outputs and the naive codon posteriors live in NodeCodonsWs
  DevBuf part, table;  // K15b's partials and K15m's tables of a launch group
  DevBuf ec_tmp;       // a launch group's edge_change where only edge_load is taken
  DevBuf cc, aa, sc, partial_c, partial_a, partial_s;  // the batch's rows where the caller does not take them; the slabs
  DevBuf out_cc, out_aa, out_sc, out_ec, out_el, out_cond, out_wcc, out_waa, out_wsc;  // the host-pointer form's device copies
};

struct PosteriorWs {  // K5's arrays that the caller of lh_eval_posterior_batch_device does not hand in
  DevBuf loglik, weights, stats, partial;
};

// K6 (lh_naive_probs.hip).  The prior P_HMM(s) of a candidate is the forward sweep over indicator emissions, one per
// caller column: `twin` is the family created once more without its alignment (lh_family_create), whose columns are
// the caller's one to one; col_site / col_base are the caller's column -> (site, naive base) map.
struct ViterbiWs {  // K8 (lh_viterbi.hip): the back-pointers, and the arrays the caller does not hand in
  DevBuf bp, loglik, states, log_path, weights, stats;
  DevBuf paths, first_bad;  // lh_family_set_candidate_paths
};

// K9 (lh_codon.hip).  CodonSource: what lh_family_set_codons needs of the caller's descriptor (the bases and sites the
// states write), kept on the host by lh_family_create.
struct CodonSegments {
  std::vector<int32_t> offsets, inds;
};
struct CodonSourceJunction {
  std::vector<int32_t> left_xmsa, right_xmsa, nti_xmsa;  // [W][nL], [W][nR], [W][nR][4] caller columns
};
struct CodonSource {
  bool have = false;
  std::vector<int32_t> site;  // [n_xmsa]
  std::vector<uint8_t> base;  // [n_xmsa]
  CodonSegments v, d, j;
  CodonSourceJunction vd, dj;
};
// What K9's and K10's entry points share: a table per row (K9: the windows, K10: the events), the gene posteriors, and the
// weighted sums of both.
struct TableWs {
  DevBuf loglik, table, genes;               // the arrays the caller does not hand in
  DevBuf weights, stats, partial_t, partial_g;
  DevBuf out_tsum, out_gsum;                 // the host-pointer form's device copies of the weighted sums
};
struct CodonWs : TableWs {
  int32_t frame = -1;  // -1: lh_family_set_codons has not been called (or its last call failed)
  int32_t n_codons = 0;
  std::vector<int32_t> window_codon;
  lh::CodonTables tab{};
  DevBuf win, codes;  // the tables
  DevBuf scratch;
  // what K14's tables are built from (host): the chain position of every site, the positions of the D and the J genes, and
  // per region (V, D, J) the base every gene writes on every site (N where it writes none)
  std::vector<int32_t> site_pos;
  int32_t q_d = 0, q_j = 0;
  std::vector<uint8_t> gene_base[3];
};

// K10 (lh_events.hip)
struct EventsWs : TableWs {
  DevBuf post, scratch;  // K5's copy of the forward arrays, the per-slot normaliser tables
};

struct CandidateWs {
  lh_family* twin = nullptr;
  std::string twin_error;  // why there is no twin
  const int32_t* col_site = nullptr;  // [n_xmsa] (arena)
  const uint8_t* col_base = nullptr;  // [n_xmsa] (arena)
  lh::CandidateTables tab{};          // K == 0: lh_family_set_candidates has not been called
  DevBuf seqs, em, prior, idx, agree, lem_cols;  // the candidates and their tables
  DevBuf loglik, weights, stats, partial, lem, base;  // K6b's arrays the caller does not hand in
};

// The sequence store (lh_device.h) on a handle: store[cur] holds K distinct sequences and room for cap, and grows by
// copying into the other buffer.  The rest is the scratch of store_resolve and store_rows_read.
struct SeqStore {
  DevBuf ids, flag, pairs;
  DevBuf gather_slots, gather_out;
  DevBuf store[2];
  int cur = 0;
  int32_t K = 0;
  size_t cap = 0;  // sequences store[cur] holds room for
};

// K6c (lh_collect.hip): the naive sequences of the last lh_eval_draw_batch / lh_naive_sequences batch, and the
// candidate store lh_draws_resolve appends to.
struct CollectWs {
  DevBuf seqs, hash, states;
  int32_t n_last = -1;
  SeqStore store;
};

// K7 (lh_lineage.hip): the last lineage batch (its arrays belong to the caller, or to the handle after lh_lineage_batch)
// and the lineage store lh_lineage_resolve appends to.
struct LineageWs {
  DevBuf naive, path, nt_hash, aa_hash;  // lh_lineage_batch's device copies
  lh::LineageBatch last{};  // last.n < 0: no batch
  SeqStore store;
  LineageWs() { last.n = -1; }
};

// Device copies of the host-pointer entry points' arrays.  The entry points share them on purpose: each waits for the device
// before it fills them and before it returns, and a handle is driven by one thread at a time.
struct HostInputs {
  DevBuf ops, brlen, er, pi, alpha;
  DevBuf rates, naive;  // lh_asr_batch
  DevBuf words;         // lh_eval_sample_batch
  DevBuf log_offset;    // lh_eval_posterior_batch
  DevBuf em;            // lh_forward_batch
};
struct HostOutputs {
  DevBuf loglik, rates, xmsa_emission, forward, scaler_counts;
  DevBuf states;                     // lh_eval_sample_batch
  DevBuf anc, rate_choice;           // lh_asr_batch
  DevBuf weighted_sum, weight_stats;  // lh_eval_posterior_batch, lh_eval_candidates_batch
  DevBuf log_cand, log_prior;         // lh_eval_candidates_batch, lh_family_set_candidates
  DevBuf log_path;                    // lh_eval_viterbi_batch, lh_viterbi_forward_batch
};

// lh_eval_batch's host -> device pipeline: two pinned staging slots, a copy stream and a compute stream
struct HostPipe {
  PinnedBuf pinned[2];
  hipStream_t copy = nullptr, comp = nullptr;
  hipEvent_t staged[2] = {nullptr, nullptr};
  ~HostPipe() {
    for (hipEvent_t e : staged)
      if (e) (void)hipEventDestroy(e);
    if (copy) (void)hipStreamDestroy(copy);
    if (comp) (void)hipStreamDestroy(comp);
  }
};

// An evaluation's launch group in sub-batches (eval_group_split): K0a and every sub-batch's K0c + K1 on `prune`, every
// sub-batch's K2 on `fwd`; the events order the two against each other and against the caller's stream.  Created by the
// handle's first evaluation; an event is recorded again by every group (a wait holds the record that was the last
// one when the wait was enqueued).
// The same streams run K0a beside K0c in front of every launch group's K1 (eval_device: K0a on `prune` behind `fork`,
// joined by `join_prune` into the caller's stream, where K0c and K1 run; eval_group_split: K0a on `fwd` beside the first
// sub-batch's K0c on `prune`, whose K1 waits for `k0a`).
struct OverlapPipe {
  static constexpr int kMaxSplit = 8;  // LH_EVAL_SPLIT's range
  hipStream_t prune = nullptr, fwd = nullptr;
  hipEvent_t fork = nullptr, join_prune = nullptr, join_fwd = nullptr, k0a = nullptr;
  hipEvent_t pruned[kMaxSplit] = {};
  bool ready = false;
  int ensure(bool fwd_high) {
    if (ready) return 0;
    int least = 0, greatest = 0;
    LH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (!prune) LH_HIP(hipStreamCreateWithFlags(&prune, hipStreamNonBlocking));
    if (!fwd) LH_HIP(hipStreamCreateWithPriority(&fwd, hipStreamNonBlocking, fwd_high ? greatest : 0));
    for (hipEvent_t* e : {&fork, &join_prune, &join_fwd, &k0a})
      if (!*e) LH_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (hipEvent_t& e : pruned)
      if (!e) LH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ready = true;
    return 0;
  }
  ~OverlapPipe() {
    for (hipEvent_t e : {fork, join_prune, join_fwd, k0a})
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : pruned)
      if (e) (void)hipEventDestroy(e);
    if (prune) (void)hipStreamDestroy(prune);
    if (fwd) (void)hipStreamDestroy(fwd);
  }
};

}  // namespace

// Everything a handle owns.  Its buffers, events and streams release themselves; lh_family_destroy deletes the handle with
// its device current.
struct lh_family {
  int device = 0;
  lh::DevFamily host{};            // device pointers inside
  lh::DevFamily* dev = nullptr;    // device copy of `host`
  std::vector<void*> allocs;
  char* arena_ptr = nullptr;
  size_t arena_left = 0;
  Workspace ws;
  ForwardWs fws;
  AsrWs asr;
  PosteriorWs post;
  CandidateWs cand;
  ViterbiWs vit;
  CodonSource codon_src;
  CodonWs codon;
  EventsWs events;
  CollectWs collect;
  LineageWs lineage;
  AncestralWs anc;
  EdgesWs edges;
  AncProbsWs probs;
  NodeCodonsWs node_codons;
  CodonEdgesWs codon_edges;
  // forward arrays that stay on the device, shared by K4 and K5 in both their forms: K4 draws from them, K5 overwrites
  // them with the posteriors (calls on a handle do not overlap: they also share the workspace)
  DevBuf forward_dev;
  HostInputs in;
  HostOutputs out;
  PinnedBuf staging;  // stage_inputs' page-locked slot
  HostPipe pipe;
  OverlapPipe overlap;
  bool profile = false;
  KernelTimer<3> eval_timer;  // model, prune, forward
  KernelTimer<1> asr_timer, post_timer;
  KernelTimer<1> prior_timer, cand_timer;  // K6a, K6b
  KernelTimer<1> collect_timer;             // K6c
  KernelTimer<1> vit_timer;                 // K8
  KernelTimer<1> codon_timer;               // K9
  KernelTimer<2> events_timer;              // K10: K5's pass on the copy, K10 and its reduction
  KernelTimer<1> lineage_timer;             // K7
  KernelTimer<3> anc_timer;                 // K11: K11a, K11b (with K11r, K11c, K11m), the weighted reduction
  KernelTimer<3> edges_timer;               // K12: K11a, K12b (with K11r, K11c, K12c, K12m), the weighted reduction
  KernelTimer<3> probs_timer;               // K13's skeleton: K11a, K13b + K13e with their sweeps, the weighted reduction
  KernelTimer<2> probs_stage_timer;         // inside its second stage: the tables (K11r, K11c, K13b, K13m), the pairs (K13e, K2)
  KernelTimer<3> node_codons_timer;         // K14's skeleton: K11a, the tables + the contraction, the weighted reduction
  KernelTimer<2> node_codons_stage_timer;   // inside its second stage: the tables (K13's, the naive codons), the contraction
  KernelTimer<1> node_codons_k9_timer;      // K9, in front of K5
  KernelTimer<3> codon_edges_timer;         // K15's skeleton: K11a, the tables + the contraction, the weighted reduction
  KernelTimer<2> codon_edges_stage_timer;   // inside its second stage: the tables (K15b, K15m, the naive codons), the contraction
  KernelTimer<1> codon_edges_k9_timer;      // K9, in front of K5
  KernelTimer<5> chain_timer;               // lh_eval_lineage_batch: K0, K1, K2 + K4 + K6c, K3, K7
  bool extended = false;  // lh_family_set_extended_range
  bool have_sampler = false;
  lh::DevSampler sampler{};  // device pointers inside (arena)
  const lh::DevSampler* sampler_dev = nullptr;  // its device copy (K4 reads the tables' addresses from memory)
  int32_t n_ucol_used = 0;  // (naive base, pattern) pairs some xMSA column has (lh_family_info)
  // two device words (arena).  [0]: bit 0, K0c met a malformed schedule; bit 1, K11c / K12c a bad path or seed; bit 2, a slot
  // outside its path, and [1] = 0x7fffffff - the first such row of its call (lh_family_status reads and clears both)
  int32_t* err_flag = nullptr;
  std::string k1_form;          // the K1 kernel form of the last evaluation (lh_family_prune_form)
  std::string k2_form;          // the K2 kernels of the last forward sweep (lh_family_forward_form)
  int k2_dj_samples = 0;        // samples per wave of its D-J kernel (lh_family_forward_dj_samples)
  int k2_dj_waves = 0;          // waves per workgroup of that kernel (lh_family_forward_dj_waves)
};

namespace {

// A handle belongs to the device that was current when lh_family_create ran; every entry point makes that device
// current for its duration, so handles of different GPUs can be driven from any thread (one thread per handle).
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(const lh_family* f) {
    if (f && hipGetDevice(&prev) == hipSuccess && prev != f->device) switched = hipSetDevice(f->device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// All family tables are sub-allocated from a few large device chunks: the forward kernel touches ~45
// small tables per junction row, and one allocation (and page) per table costs TLB reach.
int arena_alloc(lh_family* f, size_t bytes, void** out) {
  bytes = (bytes + 255) & ~(size_t)255;
  if (bytes == 0) bytes = 256;
  if (f->arena_left < bytes) {
    const size_t chunk = std::max(bytes, (size_t)8 << 20);
    void* p = nullptr;
    LH_HIP(hipMalloc(&p, chunk));
    f->allocs.push_back(p);
    f->arena_ptr = static_cast<char*>(p);
    f->arena_left = chunk;
  }
  *out = f->arena_ptr;
  f->arena_ptr += bytes;
  f->arena_left -= bytes;
  return 0;
}

template <typename T>
int upload(lh_family* f, const T* src, size_t count, const T** dst) {
  *dst = nullptr;
  void* p = nullptr;
  if (arena_alloc(f, count * sizeof(T), &p)) return 1;  // count == 0: a valid dummy address
  if (count > 0) {
    if (!src) return fail("lh_family_create: null array in descriptor");
    LH_HIP(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  }
  *dst = static_cast<const T*>(p);
  return 0;
}

// `ucol` translates the caller's xMSA column indices into u-columns (lh_device.h); the sentinel column
// whose emission is 1.0 sits at position n_ucol.
template <typename T>
int upload_vec(lh_family* f, const std::vector<T>& v, const T** out);

// Consensus form of a segment set (DevSegments): only when every gene's factors sit on consecutive alignment
// sites (xmsa_site known), the set spans at most 510 sites, and the form at least halves the factor count.
int upload_consensus(lh_family* f, const lh_segments& s, const std::vector<int32_t>& ucol, int n_ucol,
                     const int32_t* xmsa_site, int scale, lh::DevSegments* d) {
  // test hook: always the factor-by-factor walk (a property of the family being created: read here, so that a test can
  // build both forms in one process)
  const bool off = std::getenv("LH_K2A_DIRECT") != nullptr;
  if (off || !xmsa_site || s.n_genes < 1) return 0;
  const int n = s.n_genes;
  int lo = INT32_MAX, hi = -1;
  long long total = 0;
  for (int g = 0; g < n; ++g) {
    const int a = s.offsets[g], b = s.offsets[g + 1];
    if (a == b) continue;
    for (int j = a + 1; j < b; ++j)
      if (xmsa_site[s.xmsa_inds[j]] != xmsa_site[s.xmsa_inds[j - 1]] + 1) return 0;  // not site-aligned
    lo = std::min(lo, xmsa_site[s.xmsa_inds[a]]);
    hi = std::max(hi, xmsa_site[s.xmsa_inds[b - 1]] + 1);
    total += b - a;
  }
  if (hi < 0 || total < 4096) return 0;  // nothing to gain on a small set: the scan and its barriers cost more
  const int ns = hi - lo;
  if (ns > 510) return 0;
  // consensus column per site: the most frequent u-column among the genes covering it (ties: smallest)
  std::vector<std::map<int32_t, int>> votes(ns);
  for (int g = 0; g < n; ++g)
    for (int j = s.offsets[g]; j < s.offsets[g + 1]; ++j) ++votes[xmsa_site[s.xmsa_inds[j]] - lo][ucol[s.xmsa_inds[j]]];
  std::vector<int32_t> cons(ns, n_ucol);  // uncovered sites (gaps between genes): the sentinel, emission 1
  for (int p = 0; p < ns; ++p) {
    int best = 0;
    for (const auto& kv : votes[p])
      if (kv.second > best) {
        best = kv.second;
        cons[p] = kv.first;
      }
  }
  std::vector<std::vector<uint32_t>> diffs(n);
  std::vector<uint32_t> rng(n, 0);
  size_t max_diff = 0;
  for (int g = 0; g < n; ++g) {
    const int a = s.offsets[g], b = s.offsets[g + 1];
    if (a == b) continue;
    const int first = xmsa_site[s.xmsa_inds[a]] - lo;
    rng[g] = (uint32_t)first | ((uint32_t)(first + (b - a)) << 16);
    for (int j = a; j < b; ++j) {
      const int p = first + (j - a);
      const int32_t u = ucol[s.xmsa_inds[j]];
      if (u != cons[p]) diffs[g].push_back((uint32_t)p | ((uint32_t)(u * scale) << 16));
    }
    max_diff = std::max(max_diff, diffs[g].size());
    rng[g] |= (uint32_t)((diffs[g].size() + 7) / 8) << 25;  // rounds of eight departures (<= 64: at most 510 sites)
  }
  max_diff = (max_diff + 7) & ~(size_t)7;  // the kernel takes the departures eight at a time
  // worth it?  work of the consensus form (scan + per gene a division and its diffs) against the plain walk
  if ((long long)ns + (long long)n * (long long)(max_diff + 8) > total / 2) return 0;
  std::vector<uint16_t> col(ns);
  for (int p = 0; p < ns; ++p) col[p] = (uint16_t)(cons[p] * scale);
  const uint32_t pad = (uint32_t)ns | ((uint32_t)(n_ucol * scale) << 16);
  std::vector<uint32_t> dif(std::max<size_t>(max_diff, 8) * n, pad);
  for (int g = 0; g < n; ++g)
    for (size_t k = 0; k < diffs[g].size(); ++k) dif[k * n + g] = diffs[g][k];
  if (upload_vec(f, col, &d->cons_col)) return 1;
  if (upload_vec(f, rng, &d->cons_rng)) return 1;
  if (upload_vec(f, dif, &d->cons_dif)) return 1;
  d->cons_sites = ns;
  d->cons_diffs = (int32_t)max_diff;
  return 0;
}

int upload_segments(lh_family* f, const lh_segments& s, int n_xmsa, const std::vector<int32_t>& ucol, int n_ucol,
                    const int32_t* xmsa_site, lh::DevSegments* d) {
  const int scale = f->host.idx_byte_offsets ? 8 : 1;  // byte offsets into the LDS emission vector
  if (s.n_genes < 0) return fail("segments: negative gene count");
  d->n_genes = s.n_genes;
  d->cons_sites = 0;
  d->cons_diffs = 0;
  d->cons_col = nullptr;
  d->cons_rng = nullptr;
  d->cons_dif = nullptr;
  if (s.n_genes > 0) {
    if (!s.offsets) return fail("segments: null offsets");
    if (s.offsets[0] != 0) return fail("segments: offsets[0] != 0");
    for (int g = 0; g < s.n_genes; ++g)
      if (s.offsets[g + 1] < s.offsets[g]) return fail("segments: offsets not monotone");
    const int total = s.offsets[s.n_genes];
    for (int j = 0; j < total; ++j)
      if (s.xmsa_inds[j] < 0 || s.xmsa_inds[j] >= n_xmsa) return fail("segments: xMSA index out of range");
    int longest = 0;
    for (int g = 0; g < s.n_genes; ++g) longest = std::max(longest, s.offsets[g + 1] - s.offsets[g]);
    d->n_chunks = (longest + 7) / 8;
    if (n_ucol > 0xfffe) return fail("segments: more than 65534 distinct xMSA columns");
    // [chunk][gene][8] 16-bit indices, sentinel = column n_ucol (em = 1)
    std::vector<uint16_t> t((size_t)d->n_chunks * s.n_genes * 8, (uint16_t)(n_ucol * scale));
    for (int g = 0; g < s.n_genes; ++g)
      for (int j = s.offsets[g]; j < s.offsets[g + 1]; ++j) {
        const int k = j - s.offsets[g];
        t[((size_t)(k / 8) * s.n_genes + g) * 8 + (k % 8)] = (uint16_t)(ucol[s.xmsa_inds[j]] * scale);
      }
    const uint16_t* dev = nullptr;
    if (upload(f, t.data(), t.size(), &dev)) return 1;
    d->inds_c = reinterpret_cast<const uint4*>(dev);
    if (upload_consensus(f, s, ucol, n_ucol, xmsa_site, scale, d)) return 1;
  } else {
    d->n_chunks = 0;
    const uint16_t* dev = nullptr;
    if (upload<uint16_t>(f, nullptr, 0, &dev)) return 1;
    d->inds_c = reinterpret_cast<const uint4*>(dev);
  }
  return 0;
}

int check_idx(const int32_t* a, size_t n, int n_xmsa, bool allow_neg, const char* what) {
  for (size_t i = 0; i < n; ++i)
    if (a[i] >= n_xmsa || (a[i] < 0 && !(allow_neg && a[i] == -1)))
      return fail(std::string("junction: xMSA index out of range in ") + what);
  return 0;
}

// Validates a junction's emission-column indices and marks the columns it uses.
int collect_junction_cols(const lh_junction& j, int n_xmsa, std::vector<int32_t>* used) {
  const size_t W = j.n_rows, nL = j.n_left, nR = j.n_right;
  if (j.n_rows < 1 || j.n_left < 1 || j.n_right < 1) return fail("junction: bad dimensions");
  if (!j.left_xmsa || !j.right_xmsa || !j.nti_xmsa) return fail("lh_family_create: null array in junction descriptor");
  if (check_idx(j.left_xmsa, W * nL, n_xmsa, true, "left_xmsa")) return 1;
  if (check_idx(j.right_xmsa, W * nR, n_xmsa, true, "right_xmsa")) return 1;
  if (check_idx(j.nti_xmsa, W * nR * 4, n_xmsa, false, "nti_xmsa")) return 1;
  auto mark = [&](const int32_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
      if (p[i] >= 0) (*used)[p[i]] = 1;
  };
  mark(j.left_xmsa, W * nL);
  mark(j.right_xmsa, W * nR);
  mark(j.nti_xmsa, W * nR * 4);
  return 0;
}

// Copies a [rows][n][inner] table into [rows][n_pad][inner], filling the padding with `fill`.
template <typename T>
std::vector<T> pad_genes(const T* src, size_t rows, size_t n, size_t n_pad, size_t inner, T fill) {
  std::vector<T> t(rows * n_pad * inner, fill);
  for (size_t i = 0; i < rows; ++i)
    for (size_t g = 0; g < n; ++g)
      for (size_t u = 0; u < inner; ++u) t[(i * n_pad + g) * inner + u] = src[(i * n + g) * inner + u];
  return t;
}

template <typename T>
int upload_vec(lh_family* f, const std::vector<T>& v, const T** out) {
  return upload(f, v.data(), v.size(), out);
}

// `remap` translates xMSA column indices into positions of the compact junction-column list; -1 (the
// state does not emit at this site) and padding become the zero sentinel at position n_jcols.
// left_chunks / right_chunks: the 64-gene register chunks K2b's kernel template gives each side of THIS junction
// (lh_forward.hip launch_forward: the V side 1 / 2 / 4 / 8 / 16 by the V alleles, every D or J side 1 / 2 / 4 by the LARGER of
// the D and J sets).  The tables are padded to that width, not to the side's own gene count rounded up: a lane reads
// entry lane + 64 q of a row for every q of its template (round 4: with 65 D and 30 J alleles the D-J junction's J side was
// padded to 64 and read two chunks wide -- the second chunk was the NEXT row's entries, behind the last row whatever
// followed the table; such lanes feed no result, but their values entered the row's ScaleMatrix key, and a tiny one
// scaled the row's real entries to inf; found by tests/dev_tools/random_sweep_pipeline.py --many).
int upload_junction(lh_family* f, const lh_junction& j, const std::vector<int32_t>& remap, int n_jcols,
                    const int32_t* xmsa_site, const std::vector<int32_t>& pat_of_site, int left_chunks, int right_chunks,
                    lh::DevJunction* d) {
  const size_t W = j.n_rows, nL = j.n_left, nR = j.n_right;
  const size_t pL = std::max<size_t>((nL + 63) / 64, (size_t)left_chunks) * 64,
               pR = std::max<size_t>((nR + 63) / 64, (size_t)right_chunks) * 64;
  d->n_rows = j.n_rows;
  d->n_left = j.n_left;
  d->n_right = j.n_right;
  d->left_pad = (int32_t)pL;
  d->right_pad = (int32_t)pR;
  if (!j.enter_trans || !j.enter_lo || !j.left_trans || !j.left_lo || !j.right_gp_nli || !j.right_ntt ||
      !j.right_nlo || !j.right_trans || !j.right_gp_li || !j.exit_nlo || !j.exit_trans || !j.exit_gp_li)
    return fail("lh_family_create: null array in junction descriptor");
  auto cols = [&](const int32_t* src, size_t rows, size_t n, size_t n_pad, size_t inner) {
    std::vector<int32_t> t = pad_genes<int32_t>(src, rows, n, n_pad, inner, -1);
    for (int32_t& x : t) x = x >= 0 ? remap[x] : n_jcols;
    return t;
  };
  std::vector<double> ltr = pad_genes<double>(j.left_trans, W, nL, pL, 1, 0.0);
  for (size_t l = 0; l < nL; ++l) ltr[l] = j.enter_trans[l];  // row 0 is entered from the germline region
  std::vector<double> ntt(pR * 16, 0.0);
  for (size_t r = 0; r < nR; ++r)
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) ntt[r * 16 + b * 4 + a] = j.right_ntt[r * 16 + a * 4 + b];
  if (upload_vec(f, pad_genes<double>(j.enter_lo, 1, nL, pL, 1, 0.0), &d->enter_lo)) return 1;
  if (upload_vec(f, ltr, &d->left_trans)) return 1;
  if (upload_vec(f, pad_genes<double>(j.left_lo, W, nL, pL, 1, 0.0), &d->left_lo)) return 1;
  if (upload_vec(f, cols(j.left_xmsa, W, nL, pL, 1), &d->left_xmsa)) return 1;
  if (upload_vec(f, pad_genes<double>(j.right_gp_nli, 1, nR, pR, 4, 0.0), &d->right_gp_nli)) return 1;
  if (upload_vec(f, ntt, &d->right_ntt)) return 1;
  if (upload_vec(f, pad_genes<double>(j.right_nlo, W, nR, pR, 4, 0.0), &d->right_nlo)) return 1;
  if (upload_vec(f, pad_genes<double>(j.right_trans, W, nR, pR, 1, 0.0), &d->right_trans)) return 1;
  if (upload_vec(f, pad_genes<double>(j.right_gp_li, W, nR, pR, 1, 0.0), &d->right_gp_li)) return 1;
  if (upload_vec(f, cols(j.right_xmsa, W, nR, pR, 1), &d->right_xmsa)) return 1;
  if (upload_vec(f, cols(j.nti_xmsa, W, nR, pR, 4), &d->nti_xmsa)) return 1;
  if (upload_vec(f, pad_genes<double>(j.exit_nlo, 1, nR, pR, 4, 0.0), &d->exit_nlo)) return 1;
  if (upload_vec(f, pad_genes<double>(j.exit_trans, 1, nR, pR, 1, 0.0), &d->exit_trans)) return 1;
  if (upload_vec(f, pad_genes<double>(j.exit_gp_li, 1, nR, pR, 1, 0.0), &d->exit_gp_li)) return 1;
  // pattern of each row's alignment site, through the NTI emission column of the row (always present)
  std::vector<int32_t> row_pat(W, f->host.n_prune);
  if (xmsa_site)
    for (size_t i = 0; i < W; ++i) row_pat[i] = pat_of_site[xmsa_site[j.nti_xmsa[i * nR * 4]]];
  if (upload_vec(f, row_pat, &d->row_pat)) return 1;
  return 0;
}

// bytes of K1 workspace per sample: scratch area (P-matrices, cherry tables) and K0c's schedule arrays
size_t k1_bytes_per_sample(const lh_family* f, int T, int R) {
  const lh::PruneWsSizes z = lh::prune_ws_sizes(T, f->host.msa_mixed_n != 0);
  const size_t n_ops = (size_t)std::max(T - 2, 1);
  return sizeof(double) * R * z.scratch_doubles_per_rate + n_ops * (sizeof(int2) + sizeof(double)) +
         z.tabs_per_sample * sizeof(int4) + sizeof(int4);
}

// Sizes the workspace for launch groups of n samples (buffers only grow: a smaller R or T reuses them).
int ensure_workspace(lh_family* f, int n, int R, int T) {
  Workspace& w = f->ws;
  const size_t L = std::max<size_t>(f->host.n_prune, 1), cap = std::max(n, 1);
  // K1's scratch area per (sample, rate): the walk's P-matrices and cherry tables; K0c's per-sample schedule arrays
  const lh::PruneWsSizes z = lh::prune_ws_sizes(T, f->host.msa_mixed_n != 0);
  const size_t n_ops = (size_t)std::max(T - 2, 1);
  if (w.rates.ensure(sizeof(double) * cap * R) || w.eig.ensure(sizeof(double) * cap * 36) ||
      w.scratch.ensure(sizeof(double) * cap * R * z.scratch_doubles_per_rate) || w.wops.ensure(sizeof(int2) * cap * n_ops) ||
      w.wlen.ensure(sizeof(double) * cap * n_ops) || w.tabs.ensure(sizeof(int4) * cap * z.tabs_per_sample) ||
      w.hdr.ensure(sizeof(int4) * cap) || w.site_lik.ensure(sizeof(double) * cap * R * 5 * L) ||
      w.site_scal.ensure(sizeof(int32_t) * cap * R * L))
    return 1;
  w.prune = {w.scratch.get<double>(), w.wops.get<int2>(), w.wlen.get<double>(), w.tabs.get<int4>(), w.hdr.get<int4>(),
             f->err_flag};
  return 0;
}

// samples per launch group (bounds the workspace: ~150 KB per sample for a 100-tip tree; a multiple of 6144 = whole
// rounds of all three kernels on 256 CUs for configs[2]-like shapes); LH_CHUNK: test hook
static const int kChunk = lh::debug_options().chunk;

int run_forward(lh_family* f, int n, int R, const double* site_lik, const int32_t* site_scal, const double* pi,
                const double* em_in, double* em_out, double* loglik_dev, const lh_eval_outputs* outs,
                size_t sample_offset, hipStream_t stream, const lh::LogEmRequest& lem = lh::LogEmRequest{}, size_t row0 = 0,
                size_t rows = 0) {
  double* fwd = (outs && outs->forward) ? outs->forward + sample_offset * f->host.forward_size : nullptr;
  int32_t* sco =
      (outs && outs->scaler_counts) ? outs->scaler_counts + sample_offset * f->host.scaler_size : nullptr;
  ForwardWs& w = f->fws;
  // A sub-batch (eval_group_split) is rows row0 .. row0 + n of a launch group of `rows` samples: the hand-off buffers are
  // sized for the group (growing one would wait for the device and drop the other sub-batches' rows), and every one of
  // them is indexed by sample alone (lh_forward.hip: gem [gem_size], gcnt [3], jem [n_jcols], jrs [junction rows],
  // dxf [32], dxc [1] per sample), so the sub-batch works on its own rows of them.
  const size_t m = std::max(rows, row0 + (size_t)n);
  const size_t jrows = f->host.vd.n_rows + (f->host.has_d ? f->host.dj.n_rows : 0);
  if (w.jrs.ensure(sizeof(int32_t) * m * std::max(f->host.vd.n_rows + f->host.dj.n_rows, 1)) ||
      w.dxf.ensure(sizeof(double) * m * 32) || w.dxc.ensure(sizeof(int32_t) * m) ||
      w.gem.ensure(sizeof(double) * m * std::max<int64_t>(f->host.gem_size, 1)) ||
      w.jem.ensure(sizeof(double) * m * std::max(f->host.n_jcols, 1)) || w.gcnt.ensure(sizeof(int32_t) * m * 3))
    return 1;
  lh::launch_forward(f->host, f->dev, n, R, site_lik, site_scal, pi, em_in, em_out, w.gem.get<double>() + row0 * f->host.gem_size,
                     w.gcnt.get<int32_t>() + row0 * 3, w.jem.get<double>() + row0 * f->host.n_jcols,
                     w.jrs.get<int32_t>() + row0 * jrows, w.dxf.get<double>() + row0 * 32, w.dxc.get<int32_t>() + row0, loglik_dev,
                     fwd, sco, f->extended, stream, lem);
  f->k2_form = lh::forward_last_form();
  f->k2_dj_samples = lh::forward_last_dj_samples();
  f->k2_dj_waves = lh::forward_last_dj_waves();
  LH_HIP(hipGetLastError());
  return 0;
}

// Reads (and clears) the handle's asynchronous error word after synchronising its device.
int check_async_error(lh_family* f, const char* who) {
  int32_t word[2] = {0, 0};
  LH_HIP(hipDeviceSynchronize());
  LH_HIP(hipMemcpy(word, f->err_flag, sizeof(word), hipMemcpyDeviceToHost));
  const int32_t flag = word[0];
  if (flag) {
    LH_HIP(hipMemset(f->err_flag, 0, sizeof(word)));
    if ((flag & 4) && !(flag & 1))  // (K13b's slot check; it takes the place of the path's message)
      return fail(std::string(who) + ": slot of sample " + std::to_string(0x7fffffff - word[1]) +
                  " lies outside the sample's lineage path (0 .. its length - 1); the affected samples' results are NaN");
    if (flag == 2)  // (K11c's and K12c's bit alone)
      return fail(std::string(who) + ": lineage path that is not a chain up to the root, or (edge tables) a seed tip that is not a "
                                     "child of its first node; the affected samples' results are NaN");
    return fail(std::string(who) + ": malformed schedule op (use lh_schedule_tree); the affected samples' results are NaN");
  }
  return 0;
}

// A batch of trees as every evaluating entry point takes it, in the order of their signatures: n samples of T tips, each
// with its schedule, branch lengths and model.  `model` is alpha[n], or (per_rate) rates[n][R].  The arrays are the
// host's or the device's; only this struct knows their strides.
struct TreeBatch {
  int32_t n, T, max_depth;
  const int32_t* ops;   // [n][T - 2][4]
  const double* brlen;  // [n][2 T - 2]
  const double* er;     // [n][6]
  const double* pi;     // [n][4]
  const double* model;
  int32_t R;
  bool per_rate = false;
  size_t nodes() const { return 2 * (size_t)T - 2; }
  size_t n_ops() const { return (size_t)T - 2; }
  size_t model_stride() const { return per_rate ? (size_t)R : 1; }
  bool has_arrays() const { return ops && brlen && er && pi && model; }
  const int32_t* schedule(size_t i) const { return ops + i * n_ops() * 4; }
  // samples off .. off + m
  TreeBatch slice(size_t off, int32_t m) const {
    return {m, T, max_depth, schedule(off), brlen + off * nodes(), er + off * 6, pi + off * 4, model + off * model_stride(),
            R, per_rate};
  }
  // bytes per sample of ops, brlen, er, pi and model
  std::array<size_t, 5> sample_bytes() const {
    return {sizeof(int32_t) * 4 * n_ops(), sizeof(double) * nodes(), sizeof(double) * 6, sizeof(double) * 4,
            sizeof(double) * model_stride()};
  }
};

// The argument checks of every entry point that evaluates trees, `w` naming it in the messages.  Returns 1 (error set) for
// a malformed call, -1 for an empty batch and 0 otherwise: `if (int rc = check_batch(...)) return rc > 0;`
int check_batch(const lh_family* f, const std::string& w, const TreeBatch& b, bool needs_sampler = false) {
  const int n = b.n, T = b.T, R = b.R, max_depth = b.max_depth;
  if (!f) return fail(w + ": null family");
  if (needs_sampler && !f->have_sampler) return fail(w + ": lh_family_set_sampler has not been called");
  if (n < 0) return fail(w + ": negative batch size");
  if (n == 0) return -1;
  if (f->host.n_seqs < 1) return fail(w + ": family was created without an MSA (forward-only)");
  if (T != f->host.n_seqs + 1) return fail(w + ": n_tips must equal n_seqs + 1 (naive)");
  if (T < 3) return fail(w + ": need at least 3 tips");
  if (R < 1 || R > 64) return fail(w + ": num_rates out of range");
  if (max_depth < 0 || max_depth > 16) return fail(w + ": max_depth out of range");
  // (launch_prune checks the LDS need of the form it takes -- trees this large with a stack deeper than four slots do not fit)
  if ((size_t)T * 128 > 160 * 1024) return fail(w + ": too many tips for the LDS tip table");
  return 0;
}

// bytes per sample of an evaluation's launch group: K1's workspace and its planes
size_t eval_bytes_per_sample(const lh_family* f, int T, int R) {
  return k1_bytes_per_sample(f, T, R) + sizeof(double) * R * 6 * (size_t)std::max(f->host.n_prune, 1);
}

// launch groups of an evaluation: at most kChunk samples and at most ~16 GB of per-sample workspace
size_t eval_group(const lh_family* f, int T, int R) {
  return std::min<size_t>(kChunk, std::max<size_t>(1024, ((size_t)16 << 30) / eval_bytes_per_sample(f, T, R)));
}

// launch groups of the sampling kernel: at most ~8 GB of CLV area (clv_per_sample: 32 B per inner node and site) plus K1's
// workspace
size_t asr_group(const lh_family* f, int T, int R, size_t clv_per_sample) {
  return std::min<size_t>(8192, std::max<size_t>(64, ((size_t)8 << 30) / (clv_per_sample + eval_bytes_per_sample(f, T, R))));
}

// K1 for the launch group g with the given rates, into the workspace's planes (ensure_workspace has sized them), and what
// every caller makes of its outcome.  mix == false: per-rate planes, K1 must not mix the categories.  The walk that tests
// for rescaling after every op (launch_prune, test_every_op) for a handle in the extended-range mode and for the unmixed
// planes: K3 draws a site's rate category from them, and a category the assembly walk has zeroed between two of its tests
// leaves the draw to the dead ones (tests/test_gpu_rescaling_cadence.py).
// row0 > 0: g is a sub-batch (eval_group_split) that starts at row row0 of its launch group, and works on its own rows of
// the workspace -- every array is indexed by sample alone (lh_prune.hip: eig [36], the scratch area [R][rate_stride], wops and
// wlen [T - 2], tabs [tabs_stride], hdr [1], the planes [planes][5 | 1][n_prune] per sample); `rates` is the sub-batch's.
// The planes' stride needs the plane count, which the shape and not the batch size decides: row0_planes is what the
// group's first sub-batch got.  fork: the schedule kernel on another stream, joined in front of K1 (lh::PruneFork).
int prune_group(lh_family* f, const std::string& who, const TreeBatch& g, const double* rates, bool mix, hipStream_t stream,
                int* planes, size_t row0 = 0, int row0_planes = 0, const lh::PruneFork* fork = nullptr) {
  Workspace& w = f->ws;
  const lh::PruneWsSizes z = lh::prune_ws_sizes(g.T, f->host.msa_mixed_n != 0);
  const size_t L = (size_t)std::max(f->host.n_prune, 0), pl = (size_t)row0_planes;
  lh::PruneWs p = w.prune;
  p.scratch += row0 * g.R * z.scratch_doubles_per_rate;
  p.wops += row0 * g.n_ops();
  p.wlen += row0 * g.n_ops();
  p.tabs += row0 * z.tabs_per_sample;
  p.hdr += row0;
  *planes = lh::launch_prune(f->host, g.n, g.R, g.T, g.max_depth, g.ops, g.brlen, rates, w.eig.get<double>() + row0 * 36, p, g.pi,
                             w.site_lik.get<double>() + row0 * pl * 5 * L, w.site_scal.get<int32_t>() + row0 * pl * L, stream,
                             mix, f->extended || !mix, fork);
  if (*planes < 0) return fail(who + ": " + lh::prune_last_error());
  f->k1_form = lh::prune_last_form();
  if (!mix && *planes != g.R && f->host.n_prune > 0) return fail(who + ": internal error (rate planes were mixed)");
  if (row0 > 0 && *planes != row0_planes) return fail(who + ": internal error (sub-batches with different rate planes)");
  return 0;
}

// One schedule op as lh_schedule_tree writes it (a malformed op would index out of bounds on the device).
bool valid_op(const int32_t* op, int T, int nodes, int max_depth) {
  const int kind = op[0] & 15;
  const bool push = op[0] & lh::OP_PUSH_FLAG;
  const int rank = op[0] >> lh::OP_RANK_SHIFT;  // bits 5-7 unused
  bool ok = (op[0] & 0xe0) == 0 && op[0] >= 0 && kind <= 2 && rank <= T - 3;
  if (kind == lh::OP_CHERRY) ok = ok && op[1] >= 1 && op[1] < T && op[2] >= 1 && op[2] < T;
  if (kind == lh::OP_TIP_ACC) ok = ok && !push && op[1] >= 1 && op[1] < T && op[2] >= T && op[2] < nodes;
  if (kind == lh::OP_POP_ACC) ok = ok && !push && op[1] >= T && op[1] < nodes && op[2] >= T && op[2] < nodes;
  if (push || kind == lh::OP_POP_ACC) ok = ok && op[3] >= 0 && op[3] < max_depth;
  return ok;
}

// One sample's schedule: every op well-formed, and the rank field of each op the running count of inner-branch matrices
// lh_schedule_tree leaves there (a tip-accumulate op takes one, a pop-accumulate op two, a cherry none; T - 3 in all) --
// the fused K1 prologue files its matrices by that number.  (The kernels check the same thing again on the device:
// schedules may also arrive in device memory.)
// And the stack discipline: a push goes to slot = the number of pending siblings, a pop takes the last one, none is left at
// the end (a schedule that breaks it within the slot range computes a finite, wrong likelihood; the device checks repeat this).
bool valid_schedule(const int32_t* ops, int T, int nodes, int max_depth) {
  int count = 0, depth = 0;
  for (int k = 0; k < T - 2; ++k) {
    const int32_t* op = ops + (size_t)k * 4;
    if (!valid_op(op, T, nodes, max_depth)) return false;
    const int kind = op[0] & 15, rank = op[0] >> lh::OP_RANK_SHIFT;
    if (kind == lh::OP_CHERRY) {
      if (rank != 0 && rank != count) return false;
      if (((op[0] & lh::OP_PUSH_FLAG) != 0) != (k != 0)) return false;  // the first op has no accumulator to set aside, every later cherry does
      if (k != 0 && op[3] != depth++) return false;
    } else {
      if (rank != count) return false;
      count += kind == lh::OP_POP_ACC ? 2 : 1;
      if (kind == lh::OP_POP_ACC && op[3] != --depth) return false;
    }
  }
  return count == T - 3 && depth == 0;
}

// fn(lo, hi) on nw threads that split [0, n) between them (on the calling thread when nw is 1)
template <typename Fn>
void in_threads(size_t n, int nw, Fn&& fn) {
  if (nw <= 1) return fn((size_t)0, n);
  std::vector<std::thread> pool;
  for (int t = 0; t < nw; ++t) pool.emplace_back(fn, n * t / nw, n * (t + 1) / nw);
  for (std::thread& th : pool) th.join();
}

// All schedules of a batch; a few threads when the batch is large (0.19 us per op on one core: 0.4 ms per 2048 samples of
// a 101-tip tree, as much as the device then needs for K0-K2).
bool valid_schedules(const TreeBatch& b) {
  const size_t n = b.n;
  const int nw = (int)std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), (size_t)8, n * b.n_ops() / 65536}));
  std::atomic<bool> bad{false};
  in_threads(n, nw, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi && !bad; ++i)
      if (!valid_schedule(b.schedule(i), b.T, (int)b.nodes(), b.max_depth)) bad = true;
  });
  return !bad;
}

// Every row of the batch's path[n][P]: inner nodes, then -1 padding, and not empty
int valid_paths(const std::string& W, const int32_t* path, int P, const TreeBatch& b) {
  for (size_t i = 0; i < (size_t)b.n; ++i) {
    bool ended = false;
    for (int s = 0; s < P; ++s) {
      const int32_t v = path[i * P + s];
      if (v == -1) ended = true;
      else if (ended || v < b.T || v >= (int32_t)b.nodes()) return fail(W + ": path entries are inner nodes, then -1 padding");
    }
    if (path[i * P] == -1) return fail(W + ": empty path");
  }
  return 0;
}

int valid_naive(const std::string& W, const uint8_t* naive, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (naive[k] > 4) return fail(W + ": naive base out of range");
  return 0;
}

struct HostIn { const void* src; size_t bytes; DevBuf* dst; };  // a host array to copy in (src null: none)
struct HostOut { void* dst; const void* src; size_t bytes; };    // a device result to copy back (dst null: not wanted)

// Host inputs of a host-pointer entry point -> their device buffers.  The caller's arrays are ordinary pageable memory:
// copied from there, every transfer has the driver lock and unlock their pages, which stalls for milliseconds whenever
// other threads of the process are busy allocating (RunPipeline's formatting workers are).  One memcpy each into the
// handle's page-locked slot (64-byte aligned) costs a fraction of that; the copies go on the default stream.
int stage_inputs(lh_family* f, const std::vector<HostIn>& in) {
  auto padded = [](size_t b) { return (b + 63) & ~(size_t)63; };
  size_t total = 0;
  for (const HostIn& a : in)
    if (a.src) {
      if (a.dst->ensure(a.bytes)) return 1;
      total += padded(a.bytes);
    }
  if (f->staging.ensure(total)) return 1;
  LH_HIP(hipDeviceSynchronize());  // earlier calls may still be using the buffers
  char* slot = f->staging.get<char>();
  for (const HostIn& a : in)
    if (a.src) {
      memcpy(slot, a.src, a.bytes);
      LH_HIP(hipMemcpyAsync(a.dst->get(), slot, a.bytes, hipMemcpyHostToDevice, nullptr));
      slot += padded(a.bytes);
    }
  return 0;
}

// stage_inputs for a batch of trees on the host and the entry point's further arrays: *dev is the batch over the handle's
// device copies (f->in), as the _device forms take it.
int stage_batch(lh_family* f, const TreeBatch& host, std::initializer_list<HostIn> extras, TreeBatch* dev) {
  HostInputs& in = f->in;
  DevBuf& model = host.per_rate ? in.rates : in.alpha;
  const std::array<size_t, 5> bytes = host.sample_bytes();
  const size_t n = host.n;
  std::vector<HostIn> all{{host.ops, bytes[0] * n, &in.ops},
                          {host.brlen, bytes[1] * n, &in.brlen},
                          {host.er, bytes[2] * n, &in.er},
                          {host.pi, bytes[3] * n, &in.pi},
                          {host.model, bytes[4] * n, &model}};
  all.insert(all.end(), extras);
  if (stage_inputs(f, all)) return 1;
  *dev = host;
  dev->ops = in.ops.get<const int32_t>();
  dev->brlen = in.brlen.get<const double>();
  dev->er = in.er.get<const double>();
  dev->pi = in.pi.get<const double>();
  dev->model = model.get<const double>();
  return 0;
}

// what the caller does not hand in comes from the handle's buffers
int own(double*& p, DevBuf& b, size_t bytes) {
  if (!p && b.ensure(bytes)) return 1;
  if (!p) p = b.get<double>();
  return 0;
}

// The importance weights of a batch, w_i = exp(lw_i - max lw) with lw = loglik - log_offset, and their statistics (max lw,
// sum w, sum w^2).  prepare() takes the buffers before the evaluation is enqueued (one that grows waits for the device):
// the weights from the handle's, the statistics from the handle's unless the caller hands an array in.  launch() enqueues
// the reduction behind the evaluation.
struct WeightReduce {
  double *w = nullptr, *stats = nullptr;
  int prepare(size_t n, DevBuf& weights, DevBuf& stats_buf, double* caller_stats) {
    stats = caller_stats;
    return own(w, weights, sizeof(double) * n) || own(stats, stats_buf, sizeof(double) * 3);
  }
  void launch(int n, const double* loglik, const double* log_offset, hipStream_t stream) const {
    lh::launch_posterior_reduce(n, 0, nullptr, loglik, log_offset, w, nullptr, nullptr, stats, stream);
  }
};

// `want` (a host output the caller asked for) gets device buffer b, `bytes` long, as *d; else *d is null.
template <typename T>
int out_buf(const T* want, DevBuf& b, size_t bytes, T** d) {
  if (want && b.ensure(bytes)) return 1;
  *d = want ? b.get<T>() : nullptr;
  return 0;
}

// The host-pointer calls check their schedules on the host WHILE the device works on them: the kernels make the same checks
// themselves (a malformed op costs that sample a NaN and the handle an error code, never an out-of-bounds access), so
// nothing is risked by the order.  A batch the host check refuses hands nothing back:
int refuse_schedules(lh_family* f, const char* who) {
  (void)hipDeviceSynchronize();
  (void)check_async_error(f, who);  // (the device found it too: one report is enough)
  return fail(std::string(who) + ": malformed schedule op (use lh_schedule_tree)");
}

// The end of a host-pointer call: waits for the device, reads K0c's verdict on the schedules as the device saw them (`who`
// null: the call ran none), and copies the results back.
int copy_back(lh_family* f, const char* who, const std::vector<HostOut>& out) {
  if (!who) LH_HIP(hipDeviceSynchronize());
  if (who && check_async_error(f, who)) return 1;
  for (const HostOut& o : out)
    if (o.dst) LH_HIP(hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The end of a host-pointer call that evaluated `host`: its schedules checked beside the device, then copy_back.
int finish_batch(lh_family* f, const char* who, const TreeBatch& host, const std::vector<HostOut>& out) {
  if (!valid_schedules(host)) return refuse_schedules(f, who);
  return copy_back(f, who, out);
}

// lh_*_profile_read: the times of one of the handle's timers since the last read
template <int Stages>
int profile_read(lh_family* f, KernelTimer<Stages> lh_family::*timer, double* ms, int64_t* launches) {
  if (!f) return fail("null family");
  DeviceGuard guard(f);
  return (f->*timer).read(ms, launches);
}

}  // namespace

extern "C" {

const char* lh_last_error(void) { return g_error.c_str(); }

int lh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int lh_set_device(int32_t device) {
  if (device < 0 || device >= lh_device_count()) return fail("lh_set_device: no such device");
  LH_HIP(hipSetDevice(device));
  return 0;
}

int lh_warmup(void) {
  if (lh_device_count() < 1) return fail("lh_warmup: no HIP device available");
  LH_HIP(hipFree(nullptr));  // creates the primary context of the current device
  return 0;
}

void* lh_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    fail("lh_host_alloc: hipHostMalloc failed");
    return nullptr;
  }
  return p;
}

void lh_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int lh_family_create(const lh_family_desc* desc, lh_family** out) {
  if (!desc || !out) return fail("lh_family_create: null argument");
  *out = nullptr;
  if (desc->abi_version != LH_ABI_VERSION) return fail("lh_family_create: ABI version mismatch");
  if (lh_device_count() < 1)
    return fail("lh_family_create: no HIP device available (this library has no CPU path)");
  if (desc->n_xmsa < 1) return fail("lh_family_create: n_xmsa must be >= 1");
  if (desc->n_seqs < 0 || desc->n_sites < 0) return fail("lh_family_create: negative dimension");
  if ((int64_t)desc->n_seqs * desc->n_sites >= ((int64_t)1 << 31))
    return fail("lh_family_create: MSA larger than 2^31 bytes (K1 addresses it with 32-bit offsets)");
  lh_family* f = new lh_family();
  if (hipGetDevice(&f->device) != hipSuccess) {
    delete f;
    return fail("hipGetDevice failed");
  }
  {
    void* p = nullptr;
    if (arena_alloc(f, 2 * sizeof(int32_t), &p) || hipMemset(p, 0, 2 * sizeof(int32_t)) != hipSuccess) {
      lh_family_destroy(f);
      return fail("lh_family_create: device allocation failed");
    }
    f->err_flag = static_cast<int32_t*>(p);
  }
  lh::DevFamily& h = f->host;
  h.has_d = desc->has_d ? 1 : 0;
  h.n_seqs = desc->n_seqs;
  h.n_sites = desc->n_sites;
  h.n_xmsa = desc->n_xmsa;
  int rc = 0;
  const size_t C = desc->n_xmsa;
  std::vector<int32_t> ucol(C);  // caller's column -> u-column
  std::vector<int32_t> pat_of_site_all;  // alignment site -> K1 pattern (families with an alignment)
  if (desc->n_seqs > 0) {
    if (!desc->msa || !desc->xmsa_site || !desc->xmsa_naive_base) rc = fail("lh_family_create: null array in descriptor");
    const size_t N = desc->n_seqs, L = desc->n_sites;
    for (size_t i = 0; i < N * L && !rc; ++i)
      if (desc->msa[i] > 4) rc = fail("lh_family_create: msa value out of range");
    for (size_t c = 0; c < C && !rc; ++c)
      if (desc->xmsa_site[c] < 0 || desc->xmsa_site[c] >= desc->n_sites || desc->xmsa_naive_base[c] > 4)
        rc = fail("lh_family_create: xMSA column descriptor out of range");
    if (!rc) {
      // site patterns: identical alignment columns are pruned once (first-appearance order)
      std::map<std::string, int32_t> seen;
      std::vector<int32_t> pat_of_site(L);
      std::vector<size_t> first_site;
      std::string key(N, '\0');
      for (size_t j = 0; j < L; ++j) {
        for (size_t i = 0; i < N; ++i) key[i] = (char)desc->msa[i * L + j];
        auto it = seen.emplace(key, (int32_t)first_site.size());
        if (it.second) first_site.push_back(j);
        pat_of_site[j] = it.first->second;
      }
      // Order: patterns without an N, then patterns with some N, then (at most one) the all-N pattern.
      // The all-N column -- alignment padding -- has likelihood pi_b for naive base b whatever the tree,
      // i.e. emission 1 (sum of pi for naive base N): K1 never sees it (its site dimension is n_prune),
      // K2a writes the constant.
      // If no pattern mixes N with bases, K1 runs the instantiation without N handling.
      const size_t NP = first_site.size();
      std::vector<int> cls(NP, 0);  // 0 clean, 1 mixed, 2 all-N
      for (size_t p = 0; p < NP; ++p) {
        size_t n_n = 0;
        for (size_t i = 0; i < N; ++i) n_n += desc->msa[i * L + first_site[p]] == 4;
        cls[p] = n_n == 0 ? 0 : n_n == N ? 2 : 1;
      }
      std::vector<int32_t> order(NP), new_id(NP);
      for (size_t p = 0; p < NP; ++p) order[p] = (int32_t)p;
      std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return cls[a] < cls[b]; });
      for (size_t q = 0; q < NP; ++q) new_id[order[q]] = (int32_t)q;
      for (size_t j = 0; j < L; ++j) pat_of_site[j] = new_id[pat_of_site[j]];
      {
        std::vector<size_t> fs(NP);
        for (size_t q = 0; q < NP; ++q) fs[q] = first_site[order[q]];
        first_site.swap(fs);
      }
      const bool has_all_n = NP > 0 && cls[order[NP - 1]] == 2;
      h.n_pat = (int32_t)NP;
      h.n_prune = (int32_t)(NP - (has_all_n ? 1 : 0));
      h.msa_mixed_n = 0;
      for (int c : cls) h.msa_mixed_n |= c == 1;
      std::vector<uint8_t> pmsa(N * std::max<size_t>(h.n_prune, 1));
      for (size_t i = 0; i < N; ++i)
        for (size_t p = 0; p < (size_t)h.n_prune; ++p) pmsa[i * h.n_prune + p] = desc->msa[i * L + first_site[p]];
      // u-columns: the (naive base, pattern) pairs, numbered by their place in K1's output planes --
      // base * n_prune + pattern, then the five bases of the all-N pattern -- so that K2a fills its emission vector
      // with one pass over the planes and no look-up (lh_device.h).  Pairs no xMSA column has keep u_base = 0xff.
      const int32_t NPr = h.n_prune;
      const size_t n_u = 5 * (size_t)NPr + 5;
      std::vector<int32_t> u_pat(n_u), col_of_ucol(n_u, -1);
      std::vector<uint8_t> u_base(n_u, 0xff);
      for (size_t u = 0; u < n_u; ++u) u_pat[u] = u < 5 * (size_t)NPr ? (int32_t)(u % NPr) : NPr;
      int32_t n_used = 0;
      for (size_t c = 0; c < C; ++c) {
        const int b = desc->xmsa_naive_base[c];
        const int32_t pat = pat_of_site[desc->xmsa_site[c]];
        const int32_t u = pat < NPr ? b * NPr + pat : 5 * NPr + b;
        ucol[c] = u;
        if (col_of_ucol[u] < 0) {
          col_of_ucol[u] = (int32_t)c;
          u_base[u] = (uint8_t)b;
          ++n_used;
        }
      }
      f->n_ucol_used = n_used;
      h.n_ucol = (int32_t)u_pat.size();
      pat_of_site_all = pat_of_site;
      rc = rc || upload(f, pmsa.data(), pmsa.size(), &h.msa);
      h.msa_planes = nullptr;
      if (h.n_prune > 0) {
        // two state bits per pattern, and for alignments that mix N with bases a third plane flagging N (state bits 0 there)
        const size_t np = h.n_prune, nb = (np + 127) / 128, nm = h.msa_mixed_n ? 3 : 2;
        std::vector<uint64_t> planes(N * nb * 2 * nm, 0);
        for (size_t i = 0; i < N; ++i)
          for (size_t b = 0; b < nb; ++b)
            for (size_t s2 = 0; s2 < 2; ++s2)
              for (size_t l = 0; l < 64; ++l) {
                const uint8_t st = pmsa[i * np + std::min(128 * b + 64 * s2 + l, np - 1)];
                uint64_t* m = &planes[((i * nb + b) * 2 + s2) * nm];
                if (st < 4) {
                  m[0] |= (uint64_t)(st & 1) << l;
                  m[1] |= (uint64_t)((st >> 1) & 1) << l;
                } else {
                  m[2] |= (uint64_t)1 << l;  // (reached only when msa_mixed_n: a clean alignment holds no 4)
                }
              }
        rc = rc || upload(f, planes.data(), planes.size(), &h.msa_planes);
      }
      rc = rc || upload(f, pat_of_site.data(), pat_of_site.size(), &h.site_pat);
      rc = rc || upload(f, u_pat.data(), u_pat.size(), &h.u_pat);
      rc = rc || upload(f, u_base.data(), u_base.size(), &h.u_base);
      rc = rc || upload(f, ucol.data(), C, &h.ucol_of_col);
      rc = rc || upload(f, col_of_ucol.data(), col_of_ucol.size(), &h.col_of_ucol);
    }
  } else {
    for (size_t c = 0; c < C; ++c) ucol[c] = (int32_t)c;
    h.n_pat = 0;
    h.n_prune = 0;
    h.msa_mixed_n = 0;
    h.n_ucol = (int32_t)C;
    f->n_ucol_used = (int32_t)C;
    rc = rc || upload<uint8_t>(f, nullptr, 0, &h.msa);
    h.msa_planes = nullptr;
    rc = rc || upload<int32_t>(f, nullptr, 0, &h.site_pat);
    rc = rc || upload<int32_t>(f, nullptr, 0, &h.u_pat);
    rc = rc || upload<uint8_t>(f, nullptr, 0, &h.u_base);
    rc = rc || upload(f, ucol.data(), C, &h.ucol_of_col);
    rc = rc || upload(f, ucol.data(), C, &h.col_of_ucol);
  }
  h.idx_byte_offsets = ((int64_t)h.n_ucol + 1) * 8 <= 0xffff ? 1 : 0;
  const int32_t* seg_site = (desc->n_seqs > 0 && !rc) ? desc->xmsa_site : nullptr;  // alignment site of a column
  rc = rc || upload_segments(f, desc->vpadding, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.vpadding);
  rc = rc || upload_segments(f, desc->vgerm, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.vgerm);
  rc = rc || upload_segments(f, desc->jgerm, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.jgerm);
  rc = rc || upload_segments(f, desc->jpadding, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.jpadding);
  const size_t nV = desc->vgerm.n_genes, nJ = desc->jgerm.n_genes;
  if (!rc && (desc->vpadding.n_genes != (int)nV || desc->jpadding.n_genes != (int)nJ))
    rc = fail("lh_family_create: padding/germline gene counts differ");
  rc = rc || upload(f, desc->vgerm_gene_prob, nV, &h.vgerm_gene_prob);
  rc = rc || upload(f, desc->vpadding_transition, nV, &h.vpadding_transition);
  rc = rc || upload(f, desc->vgerm_trans_prod, nV, &h.vgerm_trans_prod);
  rc = rc || upload(f, desc->jpadding_transition, nJ, &h.jpadding_transition);
  std::vector<int32_t> remap(desc->n_xmsa, 0);  // first "used" flags, then positions in the compact junction list
  rc = rc || collect_junction_cols(desc->vd, desc->n_xmsa, &remap);
  if (h.has_d) rc = rc || collect_junction_cols(desc->dj, desc->n_xmsa, &remap);
  if (!rc) {
    std::vector<int32_t> jpos(h.n_ucol, -1), jcols;  // junction list = the u-columns the junction rows touch
    std::vector<char> used_u(h.n_ucol, 0);
    for (int c = 0; c < desc->n_xmsa; ++c)
      if (remap[c]) used_u[ucol[c]] = 1;
    for (int u = 0; u < h.n_ucol; ++u)
      if (used_u[u]) {
        jpos[u] = (int32_t)jcols.size();
        jcols.push_back(u);
      }
    for (int c = 0; c < desc->n_xmsa; ++c) remap[c] = remap[c] ? jpos[ucol[c]] : -1;
    h.n_jcols = (int32_t)jcols.size();
    rc = upload(f, jcols.data(), jcols.size(), &h.jcols);
  }
  // the chunk counts of K2b's templates (launch_forward): GA for the V side, GB for every D / J side
  auto round_to = [](int c, std::initializer_list<int> steps) {
    for (int s : steps)
      if (c <= s) return s;
    return c;
  };
  const int ga_t = round_to(((int)nV + 63) / 64, {1, 2, 4, 8, 16});
  const int gb_t = round_to((std::max((int)desc->dgerm.n_genes * (h.has_d ? 1 : 0), (int)nJ) + 63) / 64, {1, 2, 4});
  rc = rc || upload_junction(f, desc->vd, remap, h.n_jcols, seg_site, pat_of_site_all, ga_t, gb_t, &h.vd);
  if (!rc && desc->vd.n_left != (int)nV) rc = fail("lh_family_create: vd.n_left != number of V genes");
  if (h.has_d) {
    rc = rc || upload_segments(f, desc->dgerm, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.dgerm);
    rc = rc || upload_junction(f, desc->dj, remap, h.n_jcols, seg_site, pat_of_site_all, gb_t, gb_t, &h.dj);
    if (!rc && (desc->vd.n_right != desc->dgerm.n_genes || desc->dj.n_left != desc->dgerm.n_genes ||
                desc->dj.n_right != (int)nJ))
      rc = fail("lh_family_create: junction gene counts do not match the germline regions");
  } else {
    lh_segments empty{0, nullptr, nullptr};
    rc = rc || upload_segments(f, empty, desc->n_xmsa, ucol, h.n_ucol, seg_site, &h.dgerm);
    memset(&h.dj, 0, sizeof(h.dj));
    if (!rc && desc->vd.n_right != (int)nJ) rc = fail("lh_family_create: vd.n_right != number of J genes");
  }
  if (!rc) {
    h.max_genes = std::max({(int)nV, (int)nJ, h.dgerm.n_genes, 1});
    h.forward_size = (int64_t)nV + (int64_t)h.vd.n_rows * (h.vd.n_left + 5 * (int64_t)h.vd.n_right) + nJ;
    h.scaler_size = 1 + h.vd.n_rows + 1;
    if (h.has_d) {
      h.forward_size += h.dgerm.n_genes + (int64_t)h.dj.n_rows * (h.dj.n_left + 5 * (int64_t)h.dj.n_right);
      h.scaler_size += h.dj.n_rows + 1;
    }
    h.gem_size = 2 * (int64_t)nV + h.dgerm.n_genes + 2 * (int64_t)nJ;
    if (lh::forward_lds_bytes(h) > 160 * 1024)
      rc = fail("lh_family_create: family too large for the forward kernels' LDS working set");
    else if (nV > 1024 || h.dgerm.n_genes > 256 || nJ > 256)
      rc = fail("lh_family_create: more than 1024 V genes or 256 D/J genes");
  }
  if (!rc) {
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(lh::DevFamily)) != hipSuccess ||
        hipMemcpy(p, &h, sizeof(lh::DevFamily), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail("lh_family_create: device allocation failed");
    else {
      f->dev = static_cast<lh::DevFamily*>(p);
      f->allocs.push_back(p);
    }
  }
  if (!rc && desc->n_seqs > 0) {
    // K9's source tables (lh_family_set_codons)
    CodonSource& cs = f->codon_src;
    cs.site.assign(desc->xmsa_site, desc->xmsa_site + C);
    cs.base.assign(desc->xmsa_naive_base, desc->xmsa_naive_base + C);
    auto seg = [](const lh_segments& s, CodonSegments* o) {
      o->offsets.assign(s.offsets, s.offsets + s.n_genes + 1);
      o->inds.assign(s.xmsa_inds, s.xmsa_inds + s.offsets[s.n_genes]);
    };
    auto junc = [](const lh_junction& j, CodonSourceJunction* o) {
      const size_t W = j.n_rows, nL = j.n_left, nR = j.n_right;
      o->left_xmsa.assign(j.left_xmsa, j.left_xmsa + W * nL);
      o->right_xmsa.assign(j.right_xmsa, j.right_xmsa + W * nR);
      o->nti_xmsa.assign(j.nti_xmsa, j.nti_xmsa + W * nR * 4);
    };
    seg(desc->vgerm, &cs.v);
    seg(desc->jgerm, &cs.j);
    junc(desc->vd, &cs.vd);
    if (h.has_d) {
      seg(desc->dgerm, &cs.d);
      junc(desc->dj, &cs.dj);
    }
    cs.have = true;
  }
  if (!rc && desc->n_seqs > 0) {
    // K6a's twin (CandidateWs); a family it cannot be made for still evaluates, and lh_family_set_candidates says why
    rc = upload(f, desc->xmsa_site, C, &f->cand.col_site) || upload(f, desc->xmsa_naive_base, C, &f->cand.col_base);
    lh_family_desc d2 = *desc;
    d2.n_seqs = 0;
    d2.msa = nullptr;
    const std::string keep = g_error;
    if (!rc && lh_family_create(&d2, &f->cand.twin)) f->cand.twin_error = g_error;
    g_error = keep;
  }
  if (rc) {
    std::string keep = g_error;
    lh_family_destroy(f);
    g_error = keep;
    return 1;
  }
  *out = f;
  return 0;
}

void lh_family_destroy(lh_family* f) {
  if (!f) return;
  DeviceGuard guard(f);
  lh_family_destroy(std::exchange(f->cand.twin, nullptr));
  for (void* p : f->allocs) (void)hipFree(p);
  delete f;  // the members release their buffers, events and streams while the guard keeps the family's device current
}

int64_t lh_forward_size(const lh_family* f) { return f ? f->host.forward_size : 0; }

const char* lh_family_prune_form(const lh_family* f) { return f ? f->k1_form.c_str() : ""; }

const char* lh_family_forward_form(const lh_family* f) { return f ? f->k2_form.c_str() : ""; }
int lh_family_forward_dj_samples(const lh_family* f) { return f ? f->k2_dj_samples : 0; }
int lh_family_forward_dj_waves(const lh_family* f) { return f ? f->k2_dj_waves : 0; }

int lh_family_consensus_sets(const lh_family* f) {
  if (!f) return 0;
  const lh::DevFamily& h = f->host;
  return (h.vpadding.cons_sites > 0) | (h.vgerm.cons_sites > 0) << 1 | (h.dgerm.cons_sites > 0) << 2 |
         (h.jgerm.cons_sites > 0) << 3 | (h.jpadding.cons_sites > 0) << 4;
}

int lh_family_info(const lh_family* f, int32_t* n_patterns, int32_t* n_unique_columns) {
  if (!f) return fail("lh_family_info: null family");
  if (n_patterns) *n_patterns = f->host.n_prune;  // the all-N padding pattern, if any, costs nothing
  if (n_unique_columns) *n_unique_columns = f->n_ucol_used;
  return 0;
}
int64_t lh_scaler_size(const lh_family* f) { return f ? f->host.scaler_size : 0; }

int lh_schedule_tree(int32_t T, const int32_t* children, int32_t root, int32_t* ops, int32_t* max_depth) {
  if (T < 3) return fail("lh_schedule_tree: need at least 3 tips (naive + 2 sequences)");
  const int n_nodes = 2 * T - 2, I = T - 2;
  if (!children || !ops) return fail("lh_schedule_tree: null argument");
  if (root < T || root >= n_nodes) return fail("lh_schedule_tree: root must be an inner node");
  // validate: every node except root and tip 0 (naive) appears exactly once as a child
  std::vector<int> seen(n_nodes, 0);
  for (int i = 0; i < 2 * I; ++i) {
    const int c = children[i];
    if (c < 1 || c >= n_nodes) return fail("lh_schedule_tree: child id out of range");
    if (seen[c]++) return fail("lh_schedule_tree: node appears twice as a child");
  }
  if (seen[root]) return fail("lh_schedule_tree: root appears as a child");
  for (int v = 1; v < n_nodes; ++v)
    if (v != root && !seen[v]) return fail("lh_schedule_tree: node is not attached to the tree");
  // subtree tip counts + acyclicity (iterative post-order from root)
  std::vector<int> size(n_nodes, 0), order;
  order.reserve(I);
  {
    std::vector<int> stack{root};
    std::vector<char> visited(n_nodes, 0);
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      if (visited[v]) return fail("lh_schedule_tree: cycle in children array");
      visited[v] = 1;
      if (v >= T) {
        order.push_back(v);
        stack.push_back(children[2 * (v - T)]);
        stack.push_back(children[2 * (v - T) + 1]);
      }
    }
    if ((int)order.size() != I) return fail("lh_schedule_tree: tree does not span all inner nodes");
    for (int k = I - 1; k >= 0; --k) {
      const int v = order[k];
      const int a = children[2 * (v - T)], b = children[2 * (v - T) + 1];
      size[v] = (a < T ? 1 : size[a]) + (b < T ? 1 : size[b]);
    }
  }
  // emit ops: explicit stack of (node, phase)
  struct Frame {
    int v, phase, first, second;
  };
  std::vector<Frame> fs;
  fs.push_back({root, 0, 0, 0});
  int n_out = 0, depth = 0, maxd = 0;
  int n_inner_mats = 0;       // inner-branch P-matrices needed by the ops written so far (K1 packs its prologue by it)
  bool acc_live = false;      // accumulator holds a result that a later op still needs
  bool push_pending = false;  // the next cherry must push the accumulator first
  while (!fs.empty()) {
    Frame& fr = fs.back();
    const int v = fr.v;
    const int a = children[2 * (v - T)], b = children[2 * (v - T) + 1];
    const bool ta = a < T, tb = b < T;
    int32_t* op = ops + 4 * (size_t)n_out;
    if (ta && tb) {
      op[0] = lh::OP_CHERRY;
      op[1] = a;
      op[2] = b;
      op[3] = 0;
      if (push_pending) {
        op[0] |= lh::OP_PUSH_FLAG;
        op[3] = depth++;
        maxd = std::max(maxd, depth);
        push_pending = false;
      }
      ++n_out;
      acc_live = true;
      fs.pop_back();
    } else if (ta != tb) {
      const int tip = ta ? a : b, inner = ta ? b : a;
      if (fr.phase == 0) {
        fr.phase = 1;
        fs.push_back({inner, 0, 0, 0});
      } else {
        op[0] = lh::OP_TIP_ACC | (n_inner_mats << lh::OP_RANK_SHIFT);
        n_inner_mats += 1;
        op[1] = tip;
        op[2] = inner;
        op[3] = 0;
        ++n_out;
        fs.pop_back();
      }
    } else {
      if (fr.phase == 0) {
        fr.first = size[a] >= size[b] ? a : b;  // larger subtree first bounds the stack by log2(T)
        fr.second = size[a] >= size[b] ? b : a;
        fr.phase = 1;
        const int first = fr.first;
        fs.push_back({first, 0, 0, 0});
      } else if (fr.phase == 1) {
        fr.phase = 2;
        push_pending = true;  // first op of the second subtree is a cherry: it pushes `first`
        const int second = fr.second;
        fs.push_back({second, 0, 0, 0});
      } else {
        op[0] = lh::OP_POP_ACC | (n_inner_mats << lh::OP_RANK_SHIFT);
        n_inner_mats += 2;
        op[1] = fr.first;
        op[2] = fr.second;
        op[3] = --depth;
        ++n_out;
        fs.pop_back();
      }
    }
  }
  (void)acc_live;
  if (n_out != I || depth != 0) return fail("lh_schedule_tree: internal scheduling error");
  if (maxd > 16) return fail("lh_schedule_tree: tree needs more than 16 stack slots");
  if (max_depth) *max_depth = maxd;
  return 0;
}

int lh_family_set_extended_range(lh_family* f, int enable) {
  if (!f) return fail("null family");
  f->extended = enable != 0;
  return 0;
}

static int upload_sampler_junction(lh_family* f, const lh_sampler_junction& j, lh::DevSampleJunction* d) {
  const size_t W = j.n_rows, nL = j.n_left, nR = j.n_right;
  if (j.n_rows < 1 || j.n_left < 1 || j.n_right < 1 || j.n_states < 2) return fail("lh_family_set_sampler: bad dimensions");
  if (!j.left_rows || !j.left_dense || !j.left_lo || !j.left_trans || !j.enter_lo || !j.right_dense || !j.right_first ||
      !j.gene_prob || !j.nti_landing_in || !j.nti_transition || !j.nti_landing_out || !j.landing_in || !j.right_trans ||
      !j.exit_nlo || !j.exit_trans || !j.exit_li || !j.prod)
    return fail("lh_family_set_sampler: null array in descriptor");
  // the genes must form two blocks of the dense state vector, each in gene order, with consistent lengths
  int lo_l = INT32_MAX, hi_l = -1, lo_r = INT32_MAX, hi_r = -1;
  for (size_t l = 0; l < nL; ++l) {
    if (j.left_rows[l] < 0 || j.left_rows[l] > j.n_rows || j.left_dense[l] < 0) return fail("lh_family_set_sampler: bad left gene");
    if (l > 0 && j.left_dense[l] < j.left_dense[l - 1] + j.left_rows[l - 1]) return fail("lh_family_set_sampler: left genes out of order");
    lo_l = std::min(lo_l, j.left_dense[l]);
    hi_l = std::max(hi_l, j.left_dense[l] + j.left_rows[l]);
  }
  for (size_t r = 0; r < nR; ++r) {
    if (j.right_first[r] < 0 || j.right_first[r] > j.n_rows || j.right_dense[r] < 0) return fail("lh_family_set_sampler: bad right gene");
    const int len = 4 + (j.n_rows - j.right_first[r]);
    if (r > 0 && j.right_dense[r] < j.right_dense[r - 1] + 4) return fail("lh_family_set_sampler: right genes out of order");
    lo_r = std::min(lo_r, j.right_dense[r]);
    hi_r = std::max(hi_r, j.right_dense[r] + len);
  }
  if (!(hi_r <= lo_l || hi_l <= lo_r) || std::max(hi_l, hi_r) > j.n_states)
    return fail("lh_family_set_sampler: the junction's genes do not form two blocks of its state vector");
  d->n_rows = j.n_rows;
  d->n_left = j.n_left;
  d->n_right = j.n_right;
  d->n_states = j.n_states;
  d->right_first_block = hi_r <= lo_l ? 1 : 0;
  std::vector<int32_t> cls((size_t)j.n_states, 0);
  for (size_t l = 0; l < nL; ++l)
    for (int i = 0; i < j.left_rows[l]; ++i) cls[(size_t)j.left_dense[l] + i] = 0 | (int32_t)(l << 4);
  for (size_t r = 0; r < nR; ++r) {
    for (int b = 0; b < 4; ++b) cls[(size_t)j.right_dense[r] + b] = 1 | (b << 2) | (int32_t)(r << 4);
    for (int i = j.right_first[r]; i < j.n_rows; ++i) cls[(size_t)j.right_dense[r] + 4 + (i - j.right_first[r])] = 2 | (int32_t)(r << 4);
  }
  if (upload(f, cls.data(), cls.size(), &d->state_class)) return 1;
  if (upload(f, j.left_rows, nL, &d->left_rows) || upload(f, j.left_dense, nL, &d->left_dense) ||
      upload(f, j.left_lo, W * nL, &d->left_lo) || upload(f, j.left_trans, W * nL, &d->left_trans) ||
      upload(f, j.enter_lo, nL, &d->enter_lo) || upload(f, j.right_dense, nR, &d->right_dense) ||
      upload(f, j.right_first, nR, &d->right_first) || upload(f, j.gene_prob, nR, &d->gp) ||
      upload(f, j.nti_landing_in, nR * 4, &d->nli) || upload(f, j.nti_transition, nR * 16, &d->ntt) ||
      upload(f, j.nti_landing_out, W * nR * 4, &d->nlo) || upload(f, j.landing_in, W * nR, &d->li) ||
      upload(f, j.right_trans, W * nR, &d->rtrans) || upload(f, j.exit_nlo, nR * 4, &d->exit_nlo) ||
      upload(f, j.exit_trans, nR, &d->exit_trans) || upload(f, j.exit_li, nR, &d->exit_li) ||
      upload(f, j.prod, nR, &d->prod))
    return 1;
  return 0;
}

int lh_family_set_sampler(lh_family* f, const lh_sampler_desc* desc) {
  if (!f || !desc) return fail("lh_family_set_sampler: null argument");
  DeviceGuard guard(f);
  const lh::DevFamily& h = f->host;
  lh::DevSampler s{};
  s.has_d = h.has_d;
  s.n_v = h.vgerm.n_genes;
  s.n_d = h.dgerm.n_genes;
  s.n_j = h.jgerm.n_genes;
  if (desc->vd.n_rows != h.vd.n_rows || desc->vd.n_left != h.vd.n_left || desc->vd.n_right != h.vd.n_right)
    return fail("lh_family_set_sampler: V-D junction dimensions differ from the family's");
  if (upload_sampler_junction(f, desc->vd, &s.vd)) return 1;
  int draws = (s.n_j >= 2) + (s.n_v >= 2) + s.vd.n_rows;
  s.states_per_sample = 2 + s.vd.n_rows;
  if (h.has_d) {
    if (desc->dj.n_rows != h.dj.n_rows || desc->dj.n_left != h.dj.n_left || desc->dj.n_right != h.dj.n_right)
      return fail("lh_family_set_sampler: D-J junction dimensions differ from the family's");
    if (upload_sampler_junction(f, desc->dj, &s.dj)) return 1;
    draws += (s.n_d >= 2) + s.dj.n_rows;
    s.states_per_sample += 1 + s.dj.n_rows;
  }
  s.words_per_sample = 2 * draws;
  f->sampler = s;
  if (upload(f, &s, 1, &f->sampler_dev)) return 1;
  f->have_sampler = true;
  return 0;
}

int32_t lh_sample_words(const lh_family* f) { return f && f->have_sampler ? f->sampler.words_per_sample : 0; }
int32_t lh_sample_states(const lh_family* f) { return f && f->have_sampler ? f->sampler.states_per_sample : 0; }

int lh_family_status(lh_family* f) {
  if (!f) return fail("lh_family_status: null family");
  DeviceGuard guard(f);
  return check_async_error(f, "lh_family_status");
}

int lh_profile_enable(lh_family* f, int enable) {
  if (!f) return fail("null family");
  f->profile = enable != 0;
  return 0;
}

int lh_profile_read(lh_family* f, double* ms_model, double* ms_prune, double* ms_forward, int64_t* n_launches) {
  double ms[3];
  if (profile_read(f, &lh_family::eval_timer, ms, n_launches)) return 1;
  if (ms_model) *ms_model = ms[0];
  if (ms_prune) *ms_prune = ms[1];
  if (ms_forward) *ms_forward = ms[2];
  return 0;
}

int lh_asr_profile_read(lh_family* f, double* ms_sampling, int64_t* n_launches) {
  return profile_read(f, &lh_family::asr_timer, ms_sampling, n_launches);
}

namespace {

// Samples per sub-batch of a launch group of m samples (m or more: the group runs whole, on the caller's stream).
// LH_EVAL_SPLIT=S forces S equal sub-batches, however small (tests, measurements).  The product's choice is kEvalSplit = 1,
// no split: on configs[2] every split measured at or below the single stream (profiles/r12_k1_k2_overlap.txt -- 56 to 79 %
// of K2's time ran inside a K1 interval, and K1 paid more for the company than K2's hidden time returned: three K1
// workgroups fill a CU's LDS and registers, so a K2 workgroup takes the place of a K1 workgroup instead of the idle issue
// slots beside it).  A kEvalSplit above 1 would cut whole blocks of 6144 samples (whole rounds of K1 and of all three K2
// kernels on 256 CUs for configs[2]-like shapes, as the launch group's own size) and leave a group too small for two such
// blocks whole: a K1 that no longer fills the chip loses more to its tail than an overlap could return.
constexpr int kEvalSplit = 1;
constexpr bool kEvalFwdHigh = false;
static_assert(kEvalSplit >= 1 && kEvalSplit <= OverlapPipe::kMaxSplit, "one `pruned` event per sub-batch");
int eval_sub_batch(int m) {
  const int forced = lh::debug_options().eval_split;
  if (forced > 0) return (m + forced - 1) / forced;
  constexpr int kBlock = 6144;
  if (kEvalSplit <= 1 || m < 2 * kBlock) return m;
  return ((m + kEvalSplit - 1) / kEvalSplit + kBlock - 1) / kBlock * kBlock;
}

// the handle's two internal streams and their events, created by the first evaluation
int ensure_overlap(lh_family* f) {
  const int fwd_priority = lh::debug_options().eval_fwd_priority;
  return f->overlap.ensure(fwd_priority < 0 ? kEvalFwdHigh : fwd_priority > 0);
}

// One launch group of eval_device (samples off .. off + g.n of the call) in sub-batches of `per` samples: K2 of sub-batch i
// runs on the handle's forward stream while K1 of sub-batch i + 1 runs on its pruning stream -- neither kernel fills the
// vector units by itself.  A sub-batch is its own rows of the group's workspace (prune_group, run_forward): no second
// workspace, no copies.  Both streams fork from the caller's stream and join it again before this returns, whatever
// the outcome, so everything the caller enqueues next -- the next group, K8 on the hand-off buffers, the next call --
// finds the group complete in stream order.
int eval_group_split(lh_family* f, const TreeBatch& g, int off, int per, double* rates, double* em_out, double* loglik,
                     const lh_eval_outputs* outs, const lh::LogEmRequest& lem, hipStream_t stream) {
  OverlapPipe& op = f->overlap;
  if (ensure_overlap(f)) return 1;
  Workspace& w = f->ws;
  const int m = g.n, R = g.R;
  const size_t C = f->host.n_xmsa, L = (size_t)std::max(f->host.n_prune, 0);
  KernelTimer<3>* timer = f->profile ? &f->eval_timer : nullptr;
  LH_HIP(hipEventRecord(op.fork, stream));
  LH_HIP(hipStreamWaitEvent(op.prune, op.fork, 0));
  LH_HIP(hipStreamWaitEvent(op.fwd, op.fork, 0));
  // K0a runs once, beside the first sub-batch's K0c: K0a on the forward stream (idle until the first K2), K0c where it was,
  // and that sub-batch's K1 behind both.  The K0 span then runs from K0a's start to that join and holds the first K0c;
  // the later sub-batches' K0c stay in their K1 spans.  (LH_K0_SERIAL: K0a -> K0c -> K1 in a row on the pruning stream.)
  const bool beside = !lh::debug_options().k0_serial;
  hipStream_t k0a_stream = beside ? op.fwd : op.prune;
  const lh::PruneFork k0_fork{op.prune, [&]() -> int {
                                LH_HIP(hipStreamWaitEvent(op.prune, op.k0a, 0));
                                if (timer && (timer->span_end(op.prune) || timer->span_begin(1, op.prune))) return 1;
                                return 0;
                              }};
  auto enqueue = [&]() -> int {
    if (timer) timer->begin_spans();
    if (timer && timer->span_begin(0, k0a_stream)) return 1;
    lh::launch_model_setup(m, R, g.er, g.pi, g.model, rates, w.eig.get<double>(), k0a_stream);
    if (beside) LH_HIP(hipEventRecord(op.k0a, op.fwd));
    if (!beside && timer && timer->span_end(op.prune)) return 1;
    int planes = 0;
    for (int r0 = 0, j = 0; r0 < m; r0 += per, ++j) {
      const int k = std::min(per, m - r0);
      const TreeBatch sub = g.slice(r0, k);
      const bool forked = beside && r0 == 0;  // (its join opens the K1 span)
      if (!forked && timer && timer->span_begin(1, op.prune)) return 1;
      if (prune_group(f, "lh_eval_batch", sub, rates + (size_t)r0 * R, true, op.prune, &planes, r0, planes, forked ? &k0_fork : nullptr))
        return 1;
      if (timer && timer->span_end(op.prune)) return 1;
      LH_HIP(hipEventRecord(op.pruned[j], op.prune));
      LH_HIP(hipStreamWaitEvent(op.fwd, op.pruned[j], 0));
      if (timer && timer->span_begin(2, op.fwd)) return 1;
      const size_t s0 = (size_t)off + r0;
      const lh::LogEmRequest lem_k{lem.cols, lem.n, lem.out ? lem.out + s0 * lem.n : nullptr};
      if (run_forward(f, k, planes, w.site_lik.get<double>() + (size_t)r0 * planes * 5 * L,
                      w.site_scal.get<int32_t>() + (size_t)r0 * planes * L, sub.pi, nullptr,
                      em_out ? em_out + (size_t)r0 * C : nullptr, loglik + s0, outs, s0, op.fwd, lem_k, r0, m))
        return 1;
      if (timer && timer->span_end(op.fwd)) return 1;
    }
    if (timer) timer->end_spans();
    return 0;
  };
  const int rc = enqueue();
  LH_HIP(hipEventRecord(op.join_prune, op.prune));
  LH_HIP(hipEventRecord(op.join_fwd, op.fwd));
  LH_HIP(hipStreamWaitEvent(stream, op.join_prune, 0));
  LH_HIP(hipStreamWaitEvent(stream, op.join_fwd, 0));
  return rc;
}

// lh_eval_batch_device's body; lem: K6b's log emissions of every sample (lem.out[n][lem.n]), or none.
// after(off, m): enqueued behind the forward sweep of every launch group (samples off .. off + m), while K2a's hand-off
// buffers still hold that group (K8 reads them); nonzero fails the call.
int eval_device(lh_family* f, const TreeBatch& b, double* loglik, const lh_eval_outputs* outs, void* hip_stream,
                const lh::LogEmRequest& lem = lh::LogEmRequest{}, const std::function<int(int, int)>* after = nullptr) {
  if (int rc = check_batch(f, "lh_eval_batch", b)) return rc > 0;
  DeviceGuard guard(f);
  if (!b.has_arrays() || !loglik) return fail("lh_eval_batch: null array");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int n = b.n, R = b.R;
  const int chunk = (int)std::min<size_t>(n, eval_group(f, b.T, R));
  if (ensure_workspace(f, chunk, R, b.T)) return 1;
  Workspace& w = f->ws;
  double *eig = w.eig.get<double>(), *site_lik = w.site_lik.get<double>();
  int32_t* site_scal = w.site_scal.get<int32_t>();
  const size_t C = f->host.n_xmsa;
  const bool serial_k0 = lh::debug_options().k0_serial;  // LH_K0_SERIAL: K0a -> K0c -> K1 in a row on the caller's stream
  if (!serial_k0 && ensure_overlap(f)) return 1;
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const TreeBatch g = b.slice(off, m);
    double* rates = (outs && outs->rates) ? outs->rates + (size_t)off * R : w.rates.get<double>();
    double* em_out = (outs && outs->xmsa_emission) ? outs->xmsa_emission + (size_t)off * C : nullptr;
    if (const int per = eval_sub_batch(m); per < m) {
      if (eval_group_split(f, g, off, per, rates, em_out, loglik, outs, lem, stream)) return 1;
      LH_HIP(hipGetLastError());
      if (after && (*after)(off, m)) return 1;
      continue;
    }
    if (f->profile && f->eval_timer.begin(stream)) return 1;
    int planes = 0;
    if (serial_k0) {
      lh::launch_model_setup(m, R, g.er, g.pi, g.model, rates, eig, stream);
      if (f->profile && f->eval_timer.mark(1, stream)) return 1;
      if (prune_group(f, "lh_eval_batch", g, rates, true, stream, &planes)) return 1;
    } else {
      // K0a (er / pi / alpha -> rates / eig) beside K0c (ops / brlen -> wops / wlen / tabs / hdr): neither reads what the
      // other writes, and a thread respectively a wave per sample leaves both bound by latency, so the step pays the
      // longer one instead of their sum (as far as they leave each other room: side by side K0a takes 119 instead of 65 us
      // on configs[2] and K0c 130 instead of 96; profiles/r17_outside_k1.txt).  The K0 pair of events spans fork to join,
      // K1's starts behind the join.
      // K0c stays on the caller's stream, where K1 follows it without a wait between two queues (such a wait measured
      // 20 us between K0c's end and K1's start, most of what running the two side by side saves); K0a, the shorter one,
      // goes to the handle's pruning stream and has ended when K0c does.
      OverlapPipe& op = f->overlap;
      LH_HIP(hipEventRecord(op.fork, stream));
      LH_HIP(hipStreamWaitEvent(op.prune, op.fork, 0));
      lh::launch_model_setup(m, R, g.er, g.pi, g.model, rates, eig, op.prune);
      LH_HIP(hipEventRecord(op.join_prune, op.prune));
      bool joined = false;
      const lh::PruneFork k0_fork{stream, [&]() -> int {
                                    joined = true;
                                    LH_HIP(hipStreamWaitEvent(stream, op.join_prune, 0));
                                    return f->profile ? f->eval_timer.mark(1, stream) : 0;
                                  }};
      const int rc = prune_group(f, "lh_eval_batch", g, rates, true, stream, &planes, 0, 0, &k0_fork);
      if (!joined) LH_HIP(hipStreamWaitEvent(stream, op.join_prune, 0));  // (K1 was refused before K0c went out)
      if (rc) return 1;
    }
    if (f->profile && f->eval_timer.mark(2, stream)) return 1;
    const lh::LogEmRequest lem_m{lem.cols, lem.n, lem.out ? lem.out + (size_t)off * lem.n : nullptr};
    if (run_forward(f, m, planes, site_lik, site_scal, g.pi, nullptr, em_out, loglik + off, outs, off, stream, lem_m))
      return 1;
    if (f->profile && f->eval_timer.end(stream)) return 1;
    LH_HIP(hipGetLastError());
    if (after && (*after)(off, m)) return 1;
  }
  return 0;
}

}  // namespace

int lh_eval_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                         const double* brlen, const double* er, const double* pi, const double* alpha,
                         int32_t R, double* loglik, const lh_eval_outputs* outs, void* hip_stream) {
  return eval_device(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, loglik, outs, hip_stream);
}

// Host pointers in, host pointers out.  The batch moves in sub-chunks through two pinned staging slots:
// while the kernels of one sub-chunk run on the compute stream, a few host threads validate the next
// sub-chunk's schedules and gather its inputs into the other slot, and the copy stream ships it.
int lh_eval_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                  const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                  double* loglik, const lh_eval_outputs* outs) {
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, "lh_eval_batch", host)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays() || !loglik) return fail("lh_eval_batch: null array");
  const size_t C = f->host.n_xmsa, FS = f->host.forward_size, SS = f->host.scaler_size;
  const lh_eval_outputs none{};
  const lh_eval_outputs& o = outs ? *outs : none;
  HostOutputs& out = f->out;
  lh_eval_outputs d_outs{};
  if (out.loglik.ensure(sizeof(double) * n) || out_buf(o.rates, out.rates, sizeof(double) * R * n, &d_outs.rates) ||
      out_buf(o.xmsa_emission, out.xmsa_emission, sizeof(double) * C * n, &d_outs.xmsa_emission) ||
      out_buf(o.forward, out.forward, sizeof(double) * FS * n, &d_outs.forward) ||
      out_buf(o.scaler_counts, out.scaler_counts, sizeof(int32_t) * SS * n, &d_outs.scaler_counts))
    return 1;
  double* d_ll = out.loglik.get<double>();

  // per-sample bytes of the five input arrays, in the order they sit in a staging slot
  const std::array<size_t, 5> bytes = host.sample_bytes();
  const char* src[5] = {(const char*)ops, (const char*)brlen, (const char*)er, (const char*)pi, (const char*)alpha};
  DevBuf* in[5] = {&f->in.ops, &f->in.brlen, &f->in.er, &f->in.pi, &f->in.alpha};
  char* dst[5];
  size_t per_sample = 0;
  for (int a = 0; a < 5; ++a) {
    if (in[a]->ensure(bytes[a] * n)) return 1;
    dst[a] = in[a]->get<char>();
    per_sample += bytes[a];
  }
  const TreeBatch dev{n, T, max_depth, (const int32_t*)dst[0], (const double*)dst[1], (const double*)dst[2],
                      (const double*)dst[3], (const double*)dst[4], R};
  const int kSub = lh::debug_options().host_sub;  // (default 12 288: whole rounds of all kernels for configs[2]-like shapes)
  const int sub = std::min<int>(n, kSub);
  HostPipe& hp = f->pipe;
  if (!hp.copy) {
    LH_HIP(hipStreamCreateWithFlags(&hp.copy, hipStreamNonBlocking));
    LH_HIP(hipStreamCreateWithFlags(&hp.comp, hipStreamNonBlocking));
    for (hipEvent_t& e : hp.staged) LH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (hp.pinned[0].ensure(per_sample * sub) || hp.pinned[1].ensure(per_sample * sub)) return 1;
  LH_HIP(hipDeviceSynchronize());  // the staging buffers may still be in use by an earlier device-pointer call

  const int n_workers = (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 8u));
  int rc = 0;
  int slot = 0;
  bool slot_used[2] = {false, false};
  for (int off = 0; off < n && !rc; off += sub, slot ^= 1) {
    const int m = std::min(sub, n - off);
    if (slot_used[slot]) LH_HIP(hipEventSynchronize(hp.staged[slot]));  // its last copy has left the slot
    char* part[5] = {hp.pinned[slot].get<char>()};
    for (int a = 1; a < 5; ++a) part[a] = part[a - 1] + bytes[a - 1] * m;
    std::atomic<bool> bad{false};
    const int nw = std::max(1, std::min(n_workers, m / 256));
    // the sub-chunk's inputs into the pinned slot ...
    in_threads(m, nw, [&](size_t lo, size_t hi) {
      for (int a = 0; a < 5; ++a) memcpy(part[a] + bytes[a] * lo, src[a] + bytes[a] * (off + lo), bytes[a] * (hi - lo));
    });
    for (int a = 0; a < 5; ++a)
      if (hipMemcpyAsync(dst[a] + bytes[a] * off, part[a], bytes[a] * m, hipMemcpyHostToDevice, hp.copy) !=
          hipSuccess)
        rc = fail("lh_eval_batch: hipMemcpyAsync failed");
    if (rc) break;
    LH_HIP(hipEventRecord(hp.staged[slot], hp.copy));
    slot_used[slot] = true;
    LH_HIP(hipStreamWaitEvent(hp.comp, hp.staged[slot], 0));
    lh_eval_outputs sub_outs{d_outs.rates ? d_outs.rates + (size_t)off * R : nullptr,
                             d_outs.xmsa_emission ? d_outs.xmsa_emission + (size_t)off * C : nullptr,
                             d_outs.forward ? d_outs.forward + (size_t)off * FS : nullptr,
                             d_outs.scaler_counts ? d_outs.scaler_counts + (size_t)off * SS : nullptr};
    rc = eval_device(f, dev.slice(off, m), d_ll + off, &sub_outs, hp.comp);
    if (rc) break;
    // ... and its schedules checked on the host while the device works on them
    in_threads(m, nw, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi && !bad; ++i)
        if (!valid_schedule(host.schedule(off + i), T, (int)host.nodes(), max_depth)) bad = true;
    });
    if (bad) rc = refuse_schedules(f, "lh_eval_batch");
  }
  if (hipDeviceSynchronize() != hipSuccess && !rc) rc = fail("lh_eval_batch: device synchronisation failed");
  if (rc) return 1;
  return copy_back(f, "lh_eval_batch",  // (K0c's verdict on the schedules as the device saw them)
                   {{loglik, d_ll, sizeof(double) * n},
                    {o.rates, d_outs.rates, sizeof(double) * R * n},
                    {o.xmsa_emission, d_outs.xmsa_emission, sizeof(double) * C * n},
                    {o.forward, d_outs.forward, sizeof(double) * FS * n},
                    {o.scaler_counts, d_outs.scaler_counts, sizeof(int32_t) * SS * n}});
}

int lh_eval_sample_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                const uint32_t* words, double* loglik, double* rates, int32_t* states, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, "lh_eval_sample_batch_device", b, true)) return rc > 0;
  DeviceGuard guard(f);
  if (!words || !states) return fail("lh_eval_sample_batch_device: null array");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const size_t FS = f->host.forward_size;
  if (f->forward_dev.ensure(sizeof(double) * FS * n)) return 1;
  double* fwd = f->forward_dev.get<double>();
  lh_eval_outputs outs{rates, nullptr, fwd, nullptr};
  if (eval_device(f, b, loglik, &outs, hip_stream)) return 1;
  lh::launch_sample(f->sampler, f->sampler_dev, n, fwd, FS, words, f->sampler.words_per_sample, states, stream);
  LH_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

namespace {

// What lh_eval_sample_batch and lh_eval_draw_batch share: the host arrays staged, K0-K2 with the forward arrays kept on
// the device (rates into out.rates when want_rates), K4's draws into out.states, loglik into out.loglik.  With `sync` the
// device is waited for after the evaluation and after the sampling; stamps[4] receive the times after the buffers, the
// copies in, the evaluation and the sampling.
int sample_host_batch(lh_family* f, const TreeBatch& host, const uint32_t* words, bool want_rates, bool sync,
                      std::chrono::steady_clock::time_point* stamps) {
  const size_t n = host.n, FS = f->host.forward_size;
  const lh::DevSampler& smp = f->sampler;
  HostOutputs& out = f->out;
  if (out.loglik.ensure(sizeof(double) * n) || (want_rates && out.rates.ensure(sizeof(double) * host.R * n)) ||
      out.states.ensure(sizeof(int32_t) * smp.states_per_sample * n) || f->forward_dev.ensure(sizeof(double) * FS * n))
    return 1;
  stamps[0] = std::chrono::steady_clock::now();
  TreeBatch dev;
  if (stage_batch(f, host, {{words, sizeof(uint32_t) * smp.words_per_sample * n, &f->in.words}}, &dev)) return 1;
  stamps[1] = std::chrono::steady_clock::now();
  double* fwd = f->forward_dev.get<double>();
  lh_eval_outputs outs{want_rates ? out.rates.get<double>() : nullptr, nullptr, fwd, nullptr};
  if (eval_device(f, dev, out.loglik.get<double>(), &outs, nullptr)) return 1;
  if (sync) LH_HIP(hipDeviceSynchronize());
  stamps[2] = std::chrono::steady_clock::now();
  lh::launch_sample(smp, f->sampler_dev, host.n, fwd, FS, f->in.words.get<const uint32_t>(), smp.words_per_sample,
                    out.states.get<int32_t>(), nullptr);
  LH_HIP(hipGetLastError());
  if (sync) LH_HIP(hipDeviceSynchronize());
  stamps[3] = std::chrono::steady_clock::now();
  return 0;
}

}  // namespace

extern "C" {

int lh_eval_sample_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                         const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                         const uint32_t* words, double* loglik, double* rates, int32_t* states) {
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, "lh_eval_sample_batch", host, true)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays() || !words || !loglik || !states) return fail("lh_eval_sample_batch: null array");
  static const bool timing = lh::debug_options().sample_timing;  // stage times of every call, on stderr
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t0 = now();
  std::chrono::steady_clock::time_point st[4];
  if (sample_host_batch(f, host, words, true, timing, st)) return 1;
  const auto t2 = st[0], t3 = st[1], t4 = st[2], t5 = st[3];
  // (not finish_batch: the stage times want a stamp between the check and the copies)
  if (!valid_schedules(host)) return refuse_schedules(f, "lh_eval_sample_batch");
  auto t6 = now();
  HostOutputs& out = f->out;
  const size_t ll_bytes = sizeof(double) * n, rates_bytes = sizeof(double) * R * n,
               states_bytes = sizeof(int32_t) * f->sampler.states_per_sample * (size_t)n;
  if (copy_back(f, "lh_eval_sample_batch",
                {{loglik, out.loglik.get(), ll_bytes}, {rates, out.rates.get(), rates_bytes},
                 {states, out.states.get(), states_bytes}}))
    return 1;
  if (timing) {
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double, std::milli>(b - a).count();
    };
    std::fprintf(stderr,
                 "[lh_eval_sample_batch] n=%d: buffers %.2f ms, copies in %.2f, evaluation %.2f, sampling %.2f, check ops (beside "
                 "the device) %.2f, copies out %.2f\n",
                 n, ms(t0, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5), ms(t5, t6), ms(t6, now()));
  }
  return 0;
}

int lh_asr_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                        const double* brlen, const double* er, const double* pi, const double* rates, int32_t R,
                        const uint8_t* naive, uint64_t seed, uint64_t first_sample, uint8_t* anc,
                        uint8_t* rate_choice, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, rates, R, true};
  if (int rc = check_batch(f, "lh_asr_batch", b)) return rc > 0;
  DeviceGuard guard(f);
  if (lh::asr_lds_bytes(T, f->host.n_sites, R, f->host.n_prune) > 160 * 1024)
    return fail("lh_asr_batch: tree / alignment too large for the sampling kernel's LDS tables");
  if (!b.has_arrays() || !naive || !anc) return fail("lh_asr_batch: null array");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const size_t n_ops = b.n_ops(), L = f->host.n_sites;
  const size_t clv_per_sample = sizeof(double) * n_ops * 4 * lh::asr_slots((int)L, R);
  const int chunk = (int)std::min<size_t>(n, asr_group(f, T, R, clv_per_sample));
  if (ensure_workspace(f, chunk, R, T)) return 1;
  AsrWs& aw = f->asr;
  if (aw.clv.ensure(clv_per_sample * chunk) || aw.desc.ensure(lh::asr_desc_bytes(T) * chunk) ||
      (!rate_choice && aw.choice.ensure(L * (size_t)chunk)))
    return 1;
  Workspace& w = f->ws;
  double *eig = w.eig.get<double>(), *site_lik = w.site_lik.get<double>();
  int32_t* site_scal = w.site_scal.get<int32_t>();
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const TreeBatch g = b.slice(off, m);
    lh::launch_gtr_setup(m, g.er, g.pi, eig, stream);
    int planes = 0;
    if (prune_group(f, "lh_asr_batch", g, g.model, false, stream, &planes)) return 1;
    if (f->profile && f->asr_timer.begin(stream)) return 1;
    if (lh::launch_asr(f->host, m, R, T, g.ops, g.brlen, g.model, eig, g.pi, site_lik, site_scal, naive + (size_t)off * L, seed,
                       first_sample + (uint64_t)off, aw.clv.get<double>(), aw.desc.get(), anc + (size_t)off * n_ops * L,
                       rate_choice ? rate_choice + (size_t)off * L : aw.choice.get<uint8_t>(), w.prune.hdr, stream))
      return fail("lh_asr_batch: launch failed");
    if (f->profile && f->asr_timer.end(stream)) return 1;
    LH_HIP(hipGetLastError());
  }
  return 0;
}

int lh_asr_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                 const double* er, const double* pi, const double* rates, int32_t R, const uint8_t* naive,
                 uint64_t seed, uint64_t first_sample, uint8_t* anc, uint8_t* rate_choice) {
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, rates, R, true};
  if (int rc = check_batch(f, "lh_asr_batch", host)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays() || !naive || !anc) return fail("lh_asr_batch: null array");
  const size_t n_ops = host.n_ops(), L = f->host.n_sites;
  if (!valid_schedules(host)) return fail("lh_asr_batch: malformed schedule op (use lh_schedule_tree)");
  if (valid_naive("lh_asr_batch", naive, (size_t)n * L)) return 1;
  HostOutputs& out = f->out;
  // sub-batches bound the device copy of the output (anc: (T-2) * L bytes per sample)
  const int sub = (int)std::max<size_t>(1, std::min<size_t>(n, ((size_t)1 << 30) / std::max<size_t>(n_ops * L, 1)));
  for (int off = 0; off < n; off += sub) {
    const int m = std::min(sub, n - off);
    const size_t anc_bytes = n_ops * L * m, choice_bytes = L * m;
    TreeBatch dev;
    if (out.anc.ensure(anc_bytes) || out.rate_choice.ensure(choice_bytes) ||
        stage_batch(f, host.slice(off, m), {{naive + (size_t)off * L, L * m, &f->in.naive}}, &dev))
      return 1;
    if (lh_asr_batch_device(f, m, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, f->in.naive.get<const uint8_t>(), seed,
                            first_sample + (uint64_t)off, out.anc.get<uint8_t>(), out.rate_choice.get<uint8_t>(), nullptr))
      return 1;
    if (copy_back(f, "lh_asr_batch",
                  {{anc + (size_t)off * n_ops * L, out.anc.get(), anc_bytes},
                   {rate_choice ? rate_choice + (size_t)off * L : nullptr, out.rate_choice.get(), choice_bytes}}))
      return 1;
  }
  return 0;
}

}  // extern "C"

namespace {

// The chain of a sample's path under its own schedule, as K11c checks it on the device: the non-padding entries are inner
// nodes, each a child of the next, the last one the root; padding (anything outside T .. 2T-3) comes only after them.
// With seed_tip > 0 also what K12c checks: that tip is a child of path[0] (of the cherry or tip-accumulate op behind it).
// One pass over the schedule tells which of the two failed.
enum ChainFault { kChain = 0, kNotChain, kNotChild };
ChainFault chain_fault(const int32_t* ops, int T, const int32_t* path, int P, int seed_tip) {
  const int n_ops = T - 2;
  std::vector<int> parent_op(n_ops, -1), op_of_node(n_ops, -1), slot(16, -1);
  long long named = 0;
  auto name = [&](int op, int node) {
    if (node >= T && node <= 2 * T - 3) op_of_node[node - T] = op;
    named += node;
  };
  for (int k = 0; k < n_ops; ++k) {
    const int32_t* op = ops + (size_t)k * 4;
    const int kind = op[0] & 15;
    if (op[0] & lh::OP_PUSH_FLAG) slot[op[3] & 15] = k - 1;
    if (kind == lh::OP_TIP_ACC) {
      parent_op[k - 1] = k;
      name(k - 1, op[2]);
    } else if (kind == lh::OP_POP_ACC) {
      const int q = slot[op[3] & 15];
      if (q < 0) return kNotChain;
      parent_op[k - 1] = k;
      parent_op[q] = k;
      name(k - 1, op[2]);
      name(q, op[1]);
    }
  }
  const long long root = (long long)n_ops * T + (long long)n_ops * (n_ops - 1) / 2 - named;
  if (root < T || root > 2 * T - 3) return kNotChain;
  op_of_node[root - T] = n_ops - 1;
  int prev = -1, len = 0, first = -1;
  bool ended = false;
  for (int s = 0; s < P; ++s) {
    const int v = path[s];
    if (v < T || v > 2 * T - 3) {
      ended = true;
      continue;
    }
    if (ended) return kNotChain;
    const int k = op_of_node[v - T];
    if (k < 0 || (len > 0 && parent_op[prev] != k)) return kNotChain;
    if (len == 0) first = k;
    prev = k;
    ++len;
  }
  if (len < 1 || prev != n_ops - 1) return kNotChain;
  if (seed_tip > 0) {
    const int32_t* op = ops + (size_t)first * 4;
    const int kind = op[0] & 15;
    if (!((kind == lh::OP_CHERRY && (op[1] == seed_tip || op[2] == seed_tip)) || (kind == lh::OP_TIP_ACC && op[1] == seed_tip)))
      return kNotChild;
  }
  return kChain;
}

int ancestral_check(const lh_family* f, const std::string& W, const TreeBatch& b, int P) {
  if (P < 1 || P > b.T - 2) return fail(W + ": path length must be in 1 .. n_tips - 2");
  if (lh::anc_lds_bytes(b.T) > 160 * 1024) return fail(W + ": tree too large for the kernel's LDS tables");
  return 0;
}

// Samples per launch group of a lineage kernel (K11 to K15): at most kChunk and 8192 samples and `budget` bytes of K11's
// scratch with the family's `own` bytes per sample in place of K11b's partials, K3s's descriptors and K1's workspace (as
// asr_group bounds K3's: a group size by memory, at least one sample)
size_t lineage_group(const lh_family* f, int T, int R, int P, size_t own, size_t budget = (size_t)8 << 30) {
  const lh::AncWsBytes z = lh::anc_ws_bytes(T, f->host.n_sites, R, f->host.n_prune, P);
  const size_t per = z.total() - z.part + own + lh::asr_desc_bytes(T) + eval_bytes_per_sample(f, T, R);
  return std::max<size_t>(1, std::min<size_t>({(size_t)kChunk, (size_t)8192, budget / per}));
}

// The scratch every lineage kernel takes for a launch group of `chunk` samples: K11's CLVs, K11r's vectors (rho only where
// no caller's rate_post serves), K11c's chains and lengths, K3s's descriptors, and `part` (null: none), the buffer of the
// family's per-rate partials at part_bytes a sample.
int lineage_workspace(lh_family* f, int chunk, int T, int R, int P, bool own_rho, DevBuf* part, size_t part_bytes, lh::AncWs* ws) {
  AncestralWs& a = f->anc;
  const lh::AncWsBytes z = lh::anc_ws_bytes(T, f->host.n_sites, R, f->host.n_prune, P);
  const size_t m = chunk;
  if (a.clv.ensure(z.clv * m) || (part && part->ensure(part_bytes * m)) || a.tvec.ensure(z.tvec * m) ||
      (own_rho && a.rho.ensure(z.rho * m)) || a.chain.ensure(z.chain * m) || a.plen.ensure(sizeof(int32_t) * m) ||
      a.desc.ensure(lh::asr_desc_bytes(T) * m))
    return 1;
  *ws = {a.clv.get<double>(), part ? part->get<double>() : nullptr, a.tvec.get<double>(), a.rho.get<double>(),
         a.chain.get<int32_t>(), a.plen.get<int32_t>(), a.desc.get()};
  return 0;
}

// K11's own bytes per sample are K11b's partials
size_t ancestral_group(const lh_family* f, int T, int R, int P) {
  return lineage_group(f, T, R, P, lh::anc_ws_bytes(T, f->host.n_sites, R, f->host.n_prune, P).part);
}

int ancestral_workspace(lh_family* f, int chunk, int T, int R, int P, bool own_rho, lh::AncWs* ws) {
  return lineage_workspace(f, chunk, T, R, P, own_rho, &f->anc.part,
                           lh::anc_ws_bytes(T, f->host.n_sites, R, f->host.n_prune, P).part, ws);
}

// K11a's table: per (site, base) the compact entries (lh_eval_outputs.forward's layout) whose state writes that base on
// that site, in ascending order -- posterior.site_base's mapping and the host library's NaiveMarginals.
int ancestral_table(lh_family* f, const std::string& W) {
  AncestralWs& a = f->anc;
  if (a.have_table) return 0;
  const CodonSource& cs = f->codon_src;
  if (!cs.have) return fail(W + ": family was created without an MSA (forward-only)");
  const lh::DevFamily& h = f->host;
  const bool has_d = h.has_d != 0;
  const size_t L = h.n_sites;
  std::vector<std::vector<int32_t>> cell(L * 5);
  int32_t k = 0;
  auto column = [&](int32_t c) {  // the entry k writes what the caller's column c says
    if (c >= 0 && cs.site[c] >= 0 && (size_t)cs.site[c] < L && cs.base[c] <= 4) cell[(size_t)cs.site[c] * 5 + cs.base[c]].push_back(k);
  };
  auto germ = [&](const CodonSegments& g, int n_genes) {
    for (int i = 0; i < n_genes; ++i, ++k)
      for (int x = g.offsets[i]; x < g.offsets[i + 1]; ++x) column(g.inds[x]);
  };
  auto junction = [&](const CodonSourceJunction& j, const lh::DevJunction& d) {
    const size_t nL = d.n_left, nR = d.n_right;
    for (size_t i = 0; i < (size_t)d.n_rows; ++i) {
      for (size_t l = 0; l < nL; ++l, ++k) column(j.left_xmsa[i * nL + l]);
      for (size_t r = 0; r < nR; ++r)
        for (int b = 0; b < 4; ++b, ++k) column(j.nti_xmsa[(i * nR + r) * 4 + b]);
      for (size_t r = 0; r < nR; ++r, ++k) column(j.right_xmsa[i * nR + r]);
    }
  };
  germ(cs.v, h.vgerm.n_genes);
  junction(cs.vd, h.vd);
  if (has_d) {
    germ(cs.d, h.dgerm.n_genes);
    junction(cs.dj, h.dj);
  }
  germ(cs.j, h.jgerm.n_genes);
  if (k != (int32_t)h.forward_size) return fail(W + ": internal error (compact layout)");
  std::vector<int32_t> off(L * 5 + 1, 0), idx;
  for (size_t c = 0; c < cell.size(); ++c) {
    idx.insert(idx.end(), cell[c].begin(), cell[c].end());
    off[c + 1] = (int32_t)idx.size();
  }
  if (a.sb_off.ensure(sizeof(int32_t) * off.size()) || a.sb_idx.ensure(sizeof(int32_t) * idx.size())) return 1;
  LH_HIP(hipMemcpy(a.sb_off.get(), off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice));
  if (!idx.empty()) LH_HIP(hipMemcpy(a.sb_idx.get(), idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
  a.have_table = true;
  return 0;
}

int edges_check(const lh_family* f, const std::string& W, const TreeBatch& b, int P, int seed_tip) {
  if (ancestral_check(f, W, b, P)) return 1;
  if (seed_tip < 1 || seed_tip > b.T - 1) return fail(W + ": seed_tip must be a tip other than naive, 1 .. n_tips - 1");
  if (lh::sub_lds_bytes(b.T, P) > 160 * 1024) return fail(W + ": tree too large for the kernel's LDS tables");
  return 0;
}

// samples per launch group of K12: its own bytes are K12b's partials, the per-slot ones (four times K11's) only where edge is
// asked for
size_t edges_group(const lh_family* f, int T, int R, int P, bool with_edge) {
  return lineage_group(f, T, R, P, lh::sub_ws_bytes(f->host.n_sites, R, P).total(with_edge));
}

int edges_workspace(lh_family* f, int chunk, int T, int R, int P, bool own_rho, bool with_edge, bool with_seed, lh::AncWs* ws,
                    lh::SubWs* sws) {
  EdgesWs& e = f->edges;
  const lh::SubWsBytes y = lh::sub_ws_bytes(f->host.n_sites, R, P);
  const size_t m = chunk;
  if (lineage_workspace(f, chunk, T, R, P, own_rho, nullptr, 0, ws) || e.cc.ensure(y.cc * m) || e.ne.ensure(y.ne * m) ||
      (with_seed && e.se.ensure(y.se * m)) || e.el.ensure(y.el * m) || (with_edge && e.edge.ensure(y.edge * m)))
    return 1;
  *sws = {e.cc.get<double>(), e.ne.get<double>(), e.se.get<double>(), e.el.get<double>(), e.edge.get<double>()};
  return 0;
}

// ---- the skeleton under K11's and K12's entry points: tables per row along a seed's lineage and their weighted sums ----

// One per-row output of an entry point.  Each family states its outputs once (ancestral_rows, edges_rows); every size,
// offset, buffer and copy below is read from there.
struct RowOut {
  double* p;         // the caller's array (null: not taken)
  size_t width;      // doubles per row
  DevBuf* copy;      // the host-pointer form's device copy (null: no caller takes it)
  DevBuf* fallback;  // the device form's array when the caller does not take it (null: formed only for the caller)
  bool need = false;      // formed although not taken: another member is made from it
  double* sum = nullptr;  // the caller's weighted sum over the rows (null: none), its slab partials, its host-form copy
  DevBuf *partial = nullptr, *sum_copy = nullptr;
  double* slabs = nullptr;
  size_t step = width;  // doubles from one launch group's rows to the next (0: the array holds one group)
  bool wanted() const { return p || sum || need; }
  size_t bytes(size_t rows) const { return sizeof(double) * width * rows; }
  double* group(size_t off) const { return p ? p + off * step : nullptr; }
  // The device form's arrays: what the caller does not take lives per launch group or, where the reduction reads it, per
  // batch.
  int settle(size_t n, size_t chunk, size_t n_slabs) {
    if (!p) step = sum ? width : 0;
    return (!p && own(p, *fallback, bytes(sum ? n : chunk))) || (sum && own(slabs, *partial, bytes(n_slabs)));
  }
  // The host-pointer form's: *d is this member over the handle's device copies, `rows` rows of it
  int stage(size_t rows, RowOut* d) const {
    *d = *this;
    d->p = d->sum = nullptr;
    return (p && out_buf(p, *copy, bytes(rows), &d->p)) || (sum && out_buf(sum, *sum_copy, bytes(1), &d->sum));
  }
};

// An entry point's arguments beside its batch of trees
struct LineageCall {
  const double* naive_prob;  // the asr forms' input, a row of rows[kSiteBase].width (null: an eval form makes it, K11a)
  const int32_t* path;
  int P, seed_tip;  // seed_tip 0: K11
  std::vector<RowOut> rows;
  const double* log_offset = nullptr;  // the eval forms' (lh_posterior_outputs' members)
  double *loglik = nullptr, *weight_stats = nullptr;
  const int32_t* slot = nullptr;  // K13 / K14 at a node per row: [n] slots of `path` (null: the entry point's `node`)
  double* em_out = nullptr;  // the eval forms': a launch group's emissions in caller columns, [chunk][n_xmsa] (null: not formed)
  // the eval forms': called per launch group with (samples, first sample, the group's forward arrays, its log-likelihoods,
  // stream) before K5 overwrites the forward arrays (K14 runs K9 there); empty: nothing is called
  std::function<int(int, size_t, const double*, const double*, hipStream_t)> before_smoothing;
  bool asked() const {
    return loglik || weight_stats || std::any_of(rows.begin(), rows.end(), [](const RowOut& r) { return r.p || r.sum; });
  }
  // bytes per sample of the host-pointer form's device copies: of what it takes, or (all) of whatever a caller can take
  size_t copy_bytes(bool all) const {
    size_t per = 0;
    for (const RowOut& r : rows) per += (all ? r.copy != nullptr : r.p != nullptr) ? r.bytes(1) : 0;
    return per;
  }
};
enum { kSiteBase = 0 };  // K11a's output leads both families' rows

// the device copies of the per-row outputs bound the batch
int refuse_oversize(const std::string& W, size_t n, const LineageCall& c, int out_mb) {
  const size_t per = c.copy_bytes(false);
  const size_t most = per ? ((size_t)out_mb << 20) / per : (size_t)INT32_MAX;
  if (n > most)
    return fail(W + ": batch too large for the device copies of its per-row outputs: at most " + std::to_string(most) +
                " samples per call for this family and path length");
  return 0;
}

// The asr _device forms behind their argument checks and their kernel's scratch: per launch group of `chunk` samples K0a's
// eigensystems, one unmixed K1 and launch(group, first sample, rates, naive_prob, scratch, stream), K11b or K12b.
template <class Launch>
int lineage_asr_device(lh_family* f, const std::string& W, const TreeBatch& b, const LineageCall& c, int chunk, const lh::AncWs& ws,
                       KernelTimer<3> lh_family::*timer, void* hip_stream, Launch&& launch) {
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  KernelTimer<3>& t = f->*timer;
  for (int off = 0; off < b.n; off += chunk) {
    const TreeBatch g = b.slice(off, std::min(chunk, b.n - off));
    lh::launch_gtr_setup(g.n, g.er, g.pi, f->ws.eig.get<double>(), stream);
    int planes = 0;
    if (prune_group(f, W, g, g.model, false, stream, &planes)) return 1;
    if (f->profile && (t.begin(stream) || t.mark(1, stream))) return 1;
    if (launch(g, off, g.model, c.naive_prob + (size_t)off * c.rows[kSiteBase].width, ws, stream)) return fail(W + ": launch failed");
    if (f->profile && (t.mark(2, stream) || t.end(stream))) return 1;
    LH_HIP(hipGetLastError());
  }
  return 0;
}

// The eval _device forms behind theirs: per launch group K0, one unmixed K1 that serves K2 and the kernel (its planes
// outlive K2), K2 forward, K5, K11a and `launch` as above on K11a's output; then K11c's `ends` where the kernel looked at
// the paths (`checked`), from c.rows[marg] into c.rows[ends] where the family has them (-1: it only settles the weights);
// behind the last group the weights and the slabs of every member with a sum.
template <class Launch>
int lineage_eval_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, int chunk, lh::AncWs ws,
                        KernelTimer<3> lh_family::*timer, bool checked, int marg, int ends, void* hip_stream, Launch&& launch) {
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  KernelTimer<3>& t = f->*timer;
  const int n = b.n, P = c.P, R = b.R;
  const size_t L = f->host.n_sites, FS = f->host.forward_size, n_slabs = lh::posterior_slabs(n);
  AncestralWs& a = f->anc;
  RowOut& site_base = c.rows[kSiteBase];
  site_base.need = true;
  const bool run = std::any_of(c.rows.begin() + 1, c.rows.end(), [](const RowOut& r) { return r.wanted(); });
  const bool reduce = c.weight_stats || std::any_of(c.rows.begin(), c.rows.end(), [](const RowOut& r) { return r.sum != nullptr; });
  double* ll = c.loglik;
  WeightReduce wr;
  if (a.plen.ensure(sizeof(int32_t) * n) || a.rates.ensure(sizeof(double) * R * chunk) ||
      f->forward_dev.ensure(sizeof(double) * FS * n) || own(ll, a.loglik, sizeof(double) * n) ||
      (reduce && (a.ll_used.ensure(sizeof(double) * n) || wr.prepare(n, a.weights, a.stats, c.weight_stats))))
    return 1;
  for (RowOut& r : c.rows)
    if (r.wanted() && r.settle(n, chunk, n_slabs)) return 1;
  ws.plen = a.plen.get<int32_t>();  // (the batch's, for the reduction; a.plen.ensure above may have moved it)
  Workspace& w = f->ws;
  double *eig = w.eig.get<double>(), *site_lik = w.site_lik.get<double>(), *fwd = f->forward_dev.get<double>();
  double* rates = a.rates.get<double>();
  int32_t* site_scal = w.site_scal.get<int32_t>();
  const lh_eval_outputs fwd_outs{nullptr, nullptr, fwd, nullptr};
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const TreeBatch g = b.slice(off, m);
    lh::launch_model_setup(m, R, g.er, g.pi, g.model, rates, eig, stream);
    int planes = 0;
    if (prune_group(f, W, g, rates, false, stream, &planes)) return 1;
    if (run_forward(f, m, planes, site_lik, site_scal, g.pi, nullptr, c.em_out, ll + off, &fwd_outs, off, stream)) return 1;
    if (c.before_smoothing && c.before_smoothing(m, off, fwd + (size_t)off * FS, ll + off, stream)) return 1;
    lh::launch_posterior(f->sampler_dev, m, fwd + (size_t)off * FS, FS, ll + off, stream);
    if (f->profile && t.begin(stream)) return 1;
    lh::launch_site_base(m, (int)L, FS, a.sb_off.get<const int32_t>(), a.sb_idx.get<const int32_t>(), fwd + (size_t)off * FS,
                         ll + off, site_base.group(off), stream);
    if (f->profile && t.mark(1, stream)) return 1;
    lh::AncWs wg = ws;
    wg.plen = ws.plen + off;
    if (run && launch(g, off, rates, site_base.group(off), wg, stream)) return fail(W + ": launch failed");
    // the paths were checked wherever the kernel formed a table: a row without one then gets no weight
    if (reduce && checked)
      lh::launch_ancestral_ends(m, P, (int)L, wg.plen, marg < 0 ? nullptr : c.rows[marg].group(off), ll + off,
                                ends < 0 ? nullptr : c.rows[ends].group(off), a.ll_used.get<double>() + off, stream);
    if (f->profile && t.mark(2, stream)) return 1;
    if (reduce && off + m == n) {
      // (where no path was looked at, the weights are the rows' own)
      wr.launch(n, checked ? a.ll_used.get<const double>() : ll, c.log_offset, stream);
      for (const RowOut& r : c.rows)
        if (r.sum) lh::launch_weighted_slabs(n, r.width, r.p, wr.w, r.slabs, r.sum, stream);
    }
    if (f->profile && t.end(stream)) return 1;
    LH_HIP(hipGetLastError());
  }
  return 0;
}

// The host-pointer form W behind its argument checks and output bound: the paths validated, then per sub-batch of `sub`
// samples the arrays staged, device(batch, call), its _device form's body on the handle's device copies, and the copy
// back.  A batch that is evaluated (alpha, not rates) has K0c check its schedules beside the host: finish_batch reads the
// verdict, and a row with a malformed schedule has no chain to check here.
template <class Device>
int lineage_batch(lh_family* f, const std::string& W, const TreeBatch& host, const LineageCall& c, size_t sub, Device&& device) {
  const bool evaluated = !host.per_rate;
  const int n = host.n, P = c.P;
  if (!evaluated && !valid_schedules(host)) return fail(W + ": malformed schedule op (use lh_schedule_tree)");
  for (size_t i = 0; i < (size_t)n; ++i) {
    if (evaluated && !valid_schedule(host.schedule(i), host.T, (int)host.nodes(), host.max_depth)) continue;
    const ChainFault bad = chain_fault(host.schedule(i), host.T, c.path + i * P, P, c.seed_tip);
    if (bad == kNotChain)
      return fail(W + ": path of sample " + std::to_string(i) +
                  " is not a chain of inner nodes, each the child of the next, that ends at the root (padding after it)");
    if (bad == kNotChild)
      return fail(W + ": seed_tip " + std::to_string(c.seed_tip) + " is not a child of path[0] of sample " + std::to_string(i));
    if (c.slot) {
      int len = 0;  // (a chain: the inner nodes lead)
      while (len < P && c.path[i * P + len] >= host.T && c.path[i * P + len] <= 2 * host.T - 3) ++len;
      if (c.slot[i] < 0 || c.slot[i] >= len)
        return fail(W + ": slot " + std::to_string(c.slot[i]) + " of sample " + std::to_string(i) +
                    " lies outside the sample's lineage path (0 .. " + std::to_string(len - 1) + ")");
    }
  }
  AncestralWs& a = f->anc;
  HostOutputs& out = f->out;
  const size_t NP = c.rows[kSiteBase].width;
  for (size_t off = 0; off < (size_t)n; off += sub) {
    const size_t m = std::min(sub, n - off);
    LineageCall d = c;
    TreeBatch dev;
    std::vector<HostOut> back;
    if (evaluated && out.loglik.ensure(sizeof(double) * m)) return 1;
    d.loglik = evaluated ? out.loglik.get<double>() : nullptr;
    back.push_back({c.loglik ? c.loglik + off : nullptr, d.loglik, sizeof(double) * m});
    for (size_t k = 0; k < c.rows.size(); ++k) {
      const RowOut& h = c.rows[k];
      if (h.stage(m, &d.rows[k])) return 1;
      back.push_back({h.group(off), d.rows[k].p, h.bytes(m)});
      back.push_back({h.sum, d.rows[k].sum, h.bytes(1)});
    }
    if (out_buf(c.weight_stats, out.weight_stats, sizeof(double) * 3, &d.weight_stats) ||
        stage_batch(f, host.slice((int)off, (int)m),
                    {{c.naive_prob ? c.naive_prob + off * NP : nullptr, sizeof(double) * NP * m, &a.naive_prob},
                     {c.log_offset ? c.log_offset + off : nullptr, sizeof(double) * m, &f->in.log_offset},
                     {c.path + off * P, sizeof(int32_t) * P * m, &a.path},
                     {c.slot ? c.slot + off : nullptr, sizeof(int32_t) * m, &a.slot}},
                    &dev))
      return 1;
    back.push_back({c.weight_stats, d.weight_stats, sizeof(double) * 3});
    d.naive_prob = c.naive_prob ? a.naive_prob.get<const double>() : nullptr;
    d.log_offset = c.log_offset ? f->in.log_offset.get<const double>() : nullptr;
    d.path = a.path.get<const int32_t>();
    d.slot = c.slot ? a.slot.get<const int32_t>() : nullptr;
    if (device(dev, d)) return 1;
    if (evaluated ? finish_batch(f, W.c_str(), host.slice((int)off, (int)m), back) : copy_back(f, W.c_str(), back)) return 1;
  }
  return 0;
}

// ---- K11: exact ancestral-state marginals along a seed's lineage (lh_ancestral.hip) ----

// K11's per-row outputs; `ends` are the two slots of marg that mean the same in every tree, which weighted_sum sums.
// Row 0 (site_base) has a device copy of its own: the given-rates form's input, naive_prob, is staged at its width, and
// asr_entry's sub-batch rule counts it through copy_bytes.
enum { kMarg = 1, kEnds, kRatePost };
std::vector<RowOut> ancestral_rows(lh_family* f, int P, int R, double* site_base, double* marg, double* rate_post,
                                   double* weighted_sum, double* weighted_rate) {
  AncestralWs& a = f->anc;
  const size_t L = f->host.n_sites;
  return {{site_base, L * 5, &a.site_base, &a.site_base},
          {marg, (size_t)P * L * 4, &a.marg, &a.marg, weighted_sum != nullptr},
          {nullptr, 2 * L * 4, nullptr, &a.ends, false, weighted_sum, &a.partial_e, &a.out_wsum},
          {rate_post, L * R, &a.rate_post, &a.rate_post, false, weighted_rate, &a.partial_r, &a.out_wrate}};
}

// K11b on a launch group, as both skeletons call it
auto ancestral_launch(lh_family* f, const LineageCall& c) {
  return [f, &c](const TreeBatch& g, size_t off, const double* rates, const double* naive_prob, const lh::AncWs& ws, hipStream_t stream) {
    Workspace& w = f->ws;
    return lh::launch_ancestral(f->host, g.n, g.R, g.T, g.ops, g.brlen, rates, w.eig.get<double>(), g.pi, w.site_lik.get<double>(),
                                w.site_scal.get<int32_t>(), naive_prob, c.path + off * c.P, c.P, ws, c.rows[kMarg].group(off),
                                c.rows[kRatePost].group(off), w.prune.hdr, f->err_flag, stream);
  };
}

int asr_marginals_device(lh_family* f, const std::string& W, const TreeBatch& b, const LineageCall& c, void* hip_stream) {
  const int chunk = (int)std::min<size_t>(b.n, ancestral_group(f, b.T, b.R, c.P));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || ancestral_workspace(f, chunk, b.T, b.R, c.P, !c.rows[kRatePost].p, &ws)) return 1;
  return lineage_asr_device(f, W, b, c, chunk, ws, &lh_family::anc_timer, hip_stream, ancestral_launch(f, c));
}

int eval_ancestral_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, void* hip_stream) {
  if (ancestral_table(f, W)) return 1;
  const int chunk = (int)std::min<size_t>(b.n, std::min(ancestral_group(f, b.T, b.R, c.P), eval_group(f, b.T, b.R)));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || ancestral_workspace(f, chunk, b.T, b.R, c.P, !c.rows[kRatePost].wanted(), &ws))
    return 1;
  // (without marg or weighted_sum no path is looked at)
  return lineage_eval_device(f, W, b, c, chunk, ws, &lh_family::anc_timer, c.rows[kMarg].wanted(), kMarg, kEnds, hip_stream,
                             ancestral_launch(f, c));
}

LineageCall ancestral_call(lh_family* f, int P, int R, const int32_t* path, const lh_ancestral_outputs* outs) {
  const lh_ancestral_outputs o = outs ? *outs : lh_ancestral_outputs{};
  return {nullptr, path, P, 0, ancestral_rows(f, P, R, o.site_base, o.marg, o.rate_post, o.weighted_sum, o.weighted_rate),
          o.log_offset, o.loglik, o.weight_stats};
}

// ---- K12: exact substitution posteriors along the edges of a seed's lineage (lh_substitutions.hip) ----

// K12's per-row outputs (lh_edges_outputs has no seed_edge and no sums)
enum { kEdge = 1, kChainCounts, kSeedEdge, kNaiveEdge, kEdgeLoad, kEdgeRatePost };
std::vector<RowOut> edges_rows(lh_family* f, int P, int R, const lh_eval_edges_outputs& o) {
  AncestralWs& a = f->anc;
  EdgesWs& e = f->edges;
  const size_t L = f->host.n_sites;
  return {{o.site_base, L * 5, &a.site_base, &a.site_base},
          {o.edge, (size_t)P * L * 16, &e.out_edge, nullptr},
          {o.chain_counts, L * 16, &e.out_cc, &e.out_cc, false, o.weighted_counts, &e.partial_c, &e.out_wcc},
          {o.seed_edge, L * 16, &e.out_se, &e.out_se, false, o.weighted_seed_edge, &e.partial_s, &e.out_wse},
          {o.naive_edge, L * 20, &e.out_ne, &e.out_ne, false, o.weighted_naive_edge, &e.partial_n, &e.out_wne},
          {o.edge_load, (size_t)P + 1, &e.out_el, nullptr},
          {o.rate_post, L * R, &a.rate_post, nullptr}};
}

// K12b on a launch group, as both skeletons call it
auto edges_launch(lh_family* f, const LineageCall& c, const lh::SubWs& sws) {
  return [f, &c, sws](const TreeBatch& g, size_t off, const double* rates, const double* naive_prob, const lh::AncWs& ws, hipStream_t stream) {
    Workspace& w = f->ws;
    const std::vector<RowOut>& r = c.rows;
    const lh::SubOut so{r[kEdge].group(off),     r[kNaiveEdge].group(off), r[kChainCounts].group(off),
                        r[kSeedEdge].group(off), r[kEdgeLoad].group(off),  r[kEdgeRatePost].group(off)};
    return lh::launch_substitutions(f->host, g.n, g.R, g.T, g.ops, g.brlen, rates, w.eig.get<double>(), g.pi, w.site_lik.get<double>(),
                                    w.site_scal.get<int32_t>(), naive_prob, c.path + off * c.P, c.P, c.seed_tip, ws, sws, so,
                                    w.prune.hdr, f->err_flag, stream);
  };
}

int asr_edges_device(lh_family* f, const std::string& W, const TreeBatch& b, const LineageCall& c, void* hip_stream) {
  const bool with_edge = c.rows[kEdge].p != nullptr;
  const int chunk = (int)std::min<size_t>(b.n, edges_group(f, b.T, b.R, c.P, with_edge));
  lh::AncWs ws;
  lh::SubWs sws;
  if (ensure_workspace(f, chunk, b.R, b.T) ||
      edges_workspace(f, chunk, b.T, b.R, c.P, !c.rows[kEdgeRatePost].p, with_edge, false, &ws, &sws))
    return 1;
  return lineage_asr_device(f, W, b, c, chunk, ws, &lh_family::edges_timer, hip_stream, edges_launch(f, c, sws));
}

int eval_edges_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, void* hip_stream) {
  if (ancestral_table(f, W)) return 1;
  const bool with_edge = c.rows[kEdge].p != nullptr;
  const int chunk = (int)std::min<size_t>(b.n, std::min(edges_group(f, b.T, b.R, c.P, with_edge), eval_group(f, b.T, b.R)));
  lh::AncWs ws;
  lh::SubWs sws;
  if (ensure_workspace(f, chunk, b.R, b.T) ||
      edges_workspace(f, chunk, b.T, b.R, c.P, !c.rows[kEdgeRatePost].p, with_edge, c.rows[kSeedEdge].wanted(), &ws, &sws))
    return 1;
  // K12c checks the paths wherever a table is formed; rate_post alone forms none
  const bool tables = std::any_of(c.rows.begin() + kEdge, c.rows.begin() + kEdgeRatePost, [](const RowOut& r) { return r.wanted(); });
  return lineage_eval_device(f, W, b, c, chunk, ws, &lh_family::edges_timer, tables, -1, -1, hip_stream, edges_launch(f, c, sws));
}

LineageCall edges_call(lh_family* f, int P, int R, const double* naive_prob, const int32_t* path, int seed_tip,
                       const lh_eval_edges_outputs& o) {
  return {naive_prob, path, P, seed_tip, edges_rows(f, P, R, o), o.log_offset, o.loglik, o.weight_stats};
}
LineageCall edges_call(lh_family* f, int P, int R, const double* naive_prob, const int32_t* path, int seed_tip,
                       const lh_edges_outputs* outs) {
  lh_eval_edges_outputs o{};
  if (outs) {
    o.edge = outs->edge;
    o.naive_edge = outs->naive_edge;
    o.chain_counts = outs->chain_counts;
    o.edge_load = outs->edge_load;
    o.rate_post = outs->rate_post;
  }
  return edges_call(f, P, R, naive_prob, path, seed_tip, o);
}

// ---- K13: exact posterior probabilities of candidate ancestral sequences (lh_ancestral_probs.hip) ----

// K13's per-row outputs; the rows' exp(log_cand) are formed only for weighted_sum
enum { kCond = 1, kLogCand, kCandProb };
std::vector<RowOut> probs_rows(lh_family* f, const lh_ancestral_candidates_outputs& o) {
  AncestralWs& a = f->anc;
  AncProbsWs& p = f->probs;
  const size_t L = f->host.n_sites, K = p.K;
  return {{nullptr, L * 5, nullptr, &a.site_base},
          {o.cond, L * 20, &p.out_cond, nullptr},
          {o.log_cand, K, &p.out_log_cand, nullptr},
          {nullptr, K, nullptr, &p.prob, false, o.weighted_sum, &p.partial, &p.out_wsum}};
}

LineageCall probs_call(lh_family* f, int P, const int32_t* path, const lh_ancestral_candidates_outputs* outs) {
  const lh_ancestral_candidates_outputs o = outs ? *outs : lh_ancestral_candidates_outputs{};
  return {nullptr, path, P, 0, probs_rows(f, o), o.log_offset, o.loglik, o.weight_stats};
}

int probs_check(const lh_family* f, const std::string& W, const TreeBatch& b, int P, int node, bool at_slot = false) {
  if (ancestral_check(f, W, b, P)) return 1;
  if (!at_slot && node != 0 && node != 1) return fail(W + ": node must be 0 (the seed's parent) or 1 (the MRCA)");
  if (f->probs.K == 0) return fail(W + ": lh_family_set_ancestral_candidates has not been called");
  if (f->extended)
    return fail(W + ": not available on a handle in the extended-range mode: the candidates' sweeps run on plain doubles, and the "
                    "emissions they start from underflow exactly where that mode is needed");
  return 0;
}

// samples per launch group of K13: its own bytes are K13b's partials, the tables and the rows' emissions
size_t probs_group(const lh_family* f, int T, int R, int P) {
  const lh::CondWsBytes y = lh::cond_ws_bytes(R, f->host.n_prune);
  return lineage_group(f, T, R, P, y.part + y.table + sizeof(double) * (size_t)f->host.n_xmsa);
}

// (row, candidate) pairs per sweep: 256 MiB of emissions, C doubles a pair, at most 32 768 pairs (LH_ANC_PAIRS: test hook)
size_t probs_pairs(const lh_family* f, size_t chunk) {
  const size_t hook = lh::debug_options().anc_pairs;
  const size_t by_memory = std::max<size_t>(1, ((size_t)256 << 20) / (sizeof(double) * (size_t)f->host.n_xmsa));
  return std::min<size_t>(hook ? hook : std::min<size_t>(by_memory, 32768), chunk * (size_t)f->probs.K);
}

int probs_workspace(lh_family* f, int chunk, int T, int R, int P, size_t pairs, bool sweeps, lh::AncWs* ws) {
  AncProbsWs& p = f->probs;
  const lh::CondWsBytes y = lh::cond_ws_bytes(R, f->host.n_prune);
  const size_t m = chunk, C = f->host.n_xmsa;
  return lineage_workspace(f, chunk, T, R, P, true, &p.part, y.part, ws) || p.table.ensure(y.table * m) ||
         (sweeps && (p.em.ensure(sizeof(double) * C * m) || p.open_ll.ensure(sizeof(double) * m) ||
                     p.pair_em.ensure(sizeof(double) * C * pairs) || p.pair_ll.ensure(sizeof(double) * pairs)));
}

// K13b on a launch group, then (sweeps) the twin's sweep of the rows' own emissions and, `pairs` pairs at a time, K13e, the
// twin's sweep and the pairs' log_cand
auto probs_launch(lh_family* f, const LineageCall& c, int node, size_t pairs, bool sweeps) {
  return [f, &c, node, pairs, sweeps](const TreeBatch& g, size_t off, const double* rates, const double* naive_prob,
                                      const lh::AncWs& ws, hipStream_t stream) -> int {
    Workspace& w = f->ws;
    AncProbsWs& p = f->probs;
    CandidateWs& cw = f->cand;
    KernelTimer<2>& t = f->probs_stage_timer;
    if (f->profile && t.begin(stream)) return 1;
    if (lh::launch_ancestral_cond(f->host, g.n, g.R, g.T, g.ops, g.brlen, rates, w.eig.get<double>(), g.pi,
                                  w.site_lik.get<double>(), w.site_scal.get<int32_t>(), naive_prob, c.path + off * c.P, c.P, node,
                                  ws, p.table.get<double>(), c.rows[kCond].group(off), w.prune.hdr, f->err_flag, stream,
                                  c.slot ? c.slot + off : nullptr, (int)off))
      return 1;
    if (f->profile && t.mark(1, stream)) return 1;
    if (sweeps) {
      const int K = p.K;
      double *pair_em = p.pair_em.get<double>(), *pair_ll = p.pair_ll.get<double>(), *open_ll = p.open_ll.get<double>();
      lh::launch_row_mask(g.n, f->host.n_xmsa, ws.plen, c.em_out, stream);
      if (run_forward(cw.twin, g.n, 1, nullptr, nullptr, nullptr, c.em_out, nullptr, open_ll, nullptr, 0, stream)) return 1;
      const long long total = (long long)g.n * K;
      for (long long q0 = 0; q0 < total; q0 += (long long)pairs) {
        const int count = (int)std::min<long long>((long long)pairs, total - q0);
        lh::launch_pair_emissions(f->host, K, q0, count, p.seqs.get<const uint8_t>(), cw.col_site, cw.col_base, ws.plen, c.em_out,
                                  p.table.get<const double>(), pair_em, stream);
        if (run_forward(cw.twin, count, 1, nullptr, nullptr, nullptr, pair_em, nullptr, pair_ll, nullptr, 0, stream)) return 1;
        lh::launch_pair_finish(K, q0, count, pair_ll, open_ll, ws.plen, c.rows[kLogCand].group(off),
                               c.rows[kCandProb].group(off), stream);
      }
    }
    if (f->profile && t.end(stream)) return 1;
    return 0;
  };
}

int eval_probs_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, int node, void* hip_stream) {
  if (ancestral_table(f, W)) return 1;
  AncProbsWs& p = f->probs;
  const bool sweeps = c.rows[kLogCand].wanted() || c.rows[kCandProb].wanted();
  const int chunk = (int)std::min<size_t>(b.n, std::min(probs_group(f, b.T, b.R, c.P), eval_group(f, b.T, b.R)));
  const size_t pairs = probs_pairs(f, chunk);
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || probs_workspace(f, chunk, b.T, b.R, c.P, pairs, sweeps, &ws)) return 1;
  c.em_out = sweeps ? p.em.get<double>() : nullptr;
  // K11c checks the paths wherever a table is formed
  const bool tables = sweeps || c.rows[kCond].wanted();
  return lineage_eval_device(f, W, b, c, chunk, ws, &lh_family::probs_timer, tables, -1, -1, hip_stream,
                             probs_launch(f, c, node, pairs, sweeps));
}

// ---- K14: exact codon marginals of a node of a seed's lineage (lh_node_codon.hip) ----

// K14's per-row outputs.  Row 0 is what the skeletons lead with: the eval form's site_base (K11r reads it; nobody takes it), the
// given-rates form's input, the caller's naive codon posteriors.  It has no copy of its own (nobody takes it back), so
// asr_entry's sub-batch rule adds its bytes to copy_bytes.
enum { kNodeCodons = 1, kNodeChange };
std::vector<RowOut> node_codons_rows(lh_family* f, bool given, const lh_node_codons_outputs& o) {
  AncestralWs& a = f->anc;
  NodeCodonsWs& k = f->node_codons;
  const size_t L = f->host.n_sites, C = f->codon.n_codons;
  return {{nullptr, given ? C * 125 : L * 5, nullptr, &a.site_base},
          {o.codons, C * 64, &k.out_codons, &k.codons, false, o.weighted_codons, &k.partial_c, &k.out_wcodons},
          {o.change, C * 4, &k.out_change, &k.change, false, o.weighted_change, &k.partial_h, &k.out_wchange}};
}

int node_codons_check(const lh_family* f, const std::string& W, const TreeBatch& b, int P, int node, bool at_slot = false) {
  if (ancestral_check(f, W, b, P)) return 1;
  if (!at_slot && node != 0 && node != 1) return fail(W + ": node must be 0 (the seed's parent) or 1 (the MRCA)");
  if (f->codon.frame < 0) return fail(W + ": lh_family_set_codons has not been called");
  return 0;
}

// The tables that give every codon its naive posterior (lh::NodeCodonTables), from what lh_family_set_codons kept: for a
// codon inside one germline region, the triple every gene of the region writes there.
int node_codons_tables(lh_family* f, const std::string& W) {
  NodeCodonsWs& k = f->node_codons;
  if (k.have) return 0;
  const CodonWs& cw = f->codon;
  const lh::DevFamily& h = f->host;
  const int L = h.n_sites, C = cw.n_codons, frame = cw.frame;
  const int nV = h.vgerm.n_genes, nD = h.has_d ? h.dgerm.n_genes : 0, nJ = h.jgerm.n_genes;
  std::vector<int32_t> codon_src(std::max(C, 1), 0);
  std::vector<int4> germ;
  std::vector<uint8_t> codes;
  for (size_t i = 0; i < cw.window_codon.size(); ++i) codon_src[cw.window_codon[i]] = (int32_t)i + 1;  // (0: not a window)
  int32_t n_germ = 0;
  for (int c = 0; c < C; ++c) {
    if (codon_src[c] > 0) {
      codon_src[c] -= 1;
      continue;
    }
    const int s0 = frame + 3 * c, q = cw.site_pos[s0];
    if (cw.site_pos[s0 + 1] != q || cw.site_pos[s0 + 2] != q || (q != 0 && q != cw.q_j && !(h.has_d && q == cw.q_d)))
      return fail(W + ": internal error (germline codon)");
    const int region = q == 0 ? 0 : q == cw.q_j ? 2 : 1;
    const int ng = region == 0 ? nV : region == 1 ? nD : nJ, g0 = region == 0 ? 0 : region == 1 ? nV : nV + nD;
    const std::vector<uint8_t>& gb = cw.gene_base[region];
    germ.push_back(make_int4((int)codes.size(), g0, ng, 0));
    for (int g = 0; g < ng; ++g) {
      const uint8_t* b = gb.data() + (size_t)g * L + s0;
      codes.push_back((uint8_t)(25 * b[0] + 5 * b[1] + b[2]));
    }
    codon_src[c] = -1 - n_germ++;
  }
  auto put = [&](DevBuf& b, const void* v, size_t bytes) {
    if (b.ensure(bytes)) return 1;
    if (bytes) LH_HIP(hipMemcpy(b.get(), v, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  LH_HIP(hipDeviceSynchronize());  // queued work may still read the old tables
  if (put(k.codon_src, codon_src.data(), sizeof(int32_t) * codon_src.size()) || put(k.germ, germ.data(), sizeof(int4) * germ.size()) ||
      put(k.codes, codes.data(), codes.size()))
    return 1;
  k.tab = {C, cw.tab.n_window, cw.tab.n_genes, k.codon_src.get<const int32_t>(), k.germ.get<const int4>(),
           k.codes.get<const uint8_t>()};
  k.have = true;
  return 0;
}

// bytes per sample of K14's own arrays in a launch group: K9's outputs, the naive codon posteriors, K13m's table
size_t node_codons_bytes(const lh_family* f) {
  const CodonWs& cw = f->codon;
  return sizeof(double) * ((size_t)cw.tab.n_window * 125 + cw.tab.n_genes + (size_t)cw.n_codons * 125);
}

// samples per launch group of K14: its own bytes are K13b's partials, the tables and K14's group arrays
size_t node_codons_group(const lh_family* f, int T, int R, int P) {
  const lh::CondWsBytes y = lh::cond_ws_bytes(R, f->host.n_prune);
  return lineage_group(f, T, R, P, y.part + y.table + node_codons_bytes(f));
}

// ---- what K14 and K15 share around the naive codons ----

// Their group arrays: the given-rates forms' zeros for K11r; else K9's outputs and scratch and the naive codon posteriors
int naive_codons_workspace(lh_family* f, int chunk, bool given) {
  NodeCodonsWs& k = f->node_codons;
  const CodonWs& cw = f->codon;
  const size_t m = chunk;
  if (given) return k.zero.ensure(sizeof(double) * 5 * (size_t)f->host.n_sites * m);
  return k.windows.ensure(sizeof(double) * 125 * (size_t)cw.tab.n_window * m) ||
         k.genes.ensure(sizeof(double) * (size_t)cw.tab.n_genes * m) || k.naive.ensure(sizeof(double) * 125 * (size_t)cw.n_codons * m) ||
         f->codon.scratch.ensure(sizeof(double) * 4 * (size_t)cw.tab.max_vec * lh::codon_slots(chunk));
}

// The eval forms' before_smoothing: K9 on a launch group, reading the forward arrays before K5 smooths them in place; its
// outputs stay in the handle's arrays, *group_ll receives the group's log-likelihoods.
auto naive_codons_k9(lh_family* f, KernelTimer<1> lh_family::*timer, const double** group_ll) {
  return [f, timer, group_ll](int m, size_t, const double* fwd, const double* ll, hipStream_t stream) -> int {
    NodeCodonsWs& k = f->node_codons;
    KernelTimer<1>& t = f->*timer;
    *group_ll = ll;
    if (f->profile && t.begin(stream)) return 1;
    lh::launch_codons(f->sampler_dev, f->codon.tab, m, fwd, f->host.forward_size, ll, f->codon.scratch.get<double>(),
                      k.windows.get<double>(), k.genes.get<double>(), stream);
    if (f->profile && t.end(stream)) return 1;
    return 0;
  };
}

// Where a launch group of n samples takes the naive codon posteriors *Q and K11r's input *site_base from.  Eval form: the
// handle's array (launch_naive_codons fills it from K9's outputs behind this) and the skeleton's naive_prob.  Given-rates
// form: the caller's posteriors, handed in as the skeleton's naive_prob, and zeros (nobody takes K11r's output).
int naive_codons_inputs(lh_family* f, bool given, int n, const double* naive_prob, hipStream_t stream, const double** Q,
                        const double** site_base) {
  NodeCodonsWs& k = f->node_codons;
  *Q = k.naive.get<const double>();
  *site_base = naive_prob;
  if (!given) return 0;
  *Q = naive_prob;
  LH_HIP(hipMemsetAsync(k.zero.get(), 0, sizeof(double) * 5 * (size_t)f->host.n_sites * n, stream));
  *site_base = k.zero.get<const double>();
  return 0;
}

// K13's scratch (probs_workspace without the sweeps) and K14's group arrays
int node_codons_workspace(lh_family* f, int chunk, int T, int R, int P, bool given, lh::AncWs* ws) {
  return probs_workspace(f, chunk, T, R, P, 0, false, ws) || naive_codons_workspace(f, chunk, given);
}

// K13b + K13m on a launch group, the naive codon posteriors of every codon (naive_codons_inputs) and the contraction.
// *group_ll: the group's log-likelihoods (eval form), null otherwise.
auto node_codons_launch(lh_family* f, const LineageCall& c, int node, bool given, const double* const* group_ll) {
  return [f, &c, node, given, group_ll](const TreeBatch& g, size_t off, const double* rates, const double* naive_prob,
                                        const lh::AncWs& ws, hipStream_t stream) -> int {
    Workspace& w = f->ws;
    AncProbsWs& p = f->probs;
    NodeCodonsWs& k = f->node_codons;
    KernelTimer<2>& t = f->node_codons_stage_timer;
    const double *Q, *site_base;
    if (naive_codons_inputs(f, given, g.n, naive_prob, stream, &Q, &site_base)) return 1;
    if (f->profile && t.begin(stream)) return 1;
    if (lh::launch_ancestral_cond(f->host, g.n, g.R, g.T, g.ops, g.brlen, rates, w.eig.get<double>(), g.pi,
                                  w.site_lik.get<double>(), w.site_scal.get<int32_t>(), site_base, c.path + off * c.P, c.P, node,
                                  ws, p.table.get<double>(), nullptr, w.prune.hdr, f->err_flag, stream, c.slot ? c.slot + off : nullptr,
                                  (int)off))
      return 1;
    if (!given)
      lh::launch_naive_codons(k.tab, g.n, k.windows.get<const double>(), k.genes.get<const double>(), k.naive.get<double>(), stream);
    if (f->profile && t.mark(1, stream)) return 1;
    lh::launch_node_codons(f->host, g.n, f->codon.n_codons, f->codon.frame, p.table.get<const double>(), Q, ws.plen,
                           group_ll ? *group_ll : nullptr, c.rows[kNodeCodons].group(off), c.rows[kNodeChange].group(off), stream);
    if (f->profile && t.end(stream)) return 1;
    return 0;
  };
}

int eval_node_codons_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, int node, void* hip_stream) {
  if (ancestral_table(f, W) || node_codons_tables(f, W)) return 1;
  const int chunk = (int)std::min<size_t>(b.n, std::min(node_codons_group(f, b.T, b.R, c.P), eval_group(f, b.T, b.R)));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || node_codons_workspace(f, chunk, b.T, b.R, c.P, false, &ws)) return 1;
  const double* group_ll = nullptr;
  c.before_smoothing = naive_codons_k9(f, &lh_family::node_codons_k9_timer, &group_ll);
  // K11c checks the paths wherever a table is formed
  const bool tables = c.rows[kNodeCodons].wanted() || c.rows[kNodeChange].wanted();
  const int rc = lineage_eval_device(f, W, b, c, chunk, ws, &lh_family::node_codons_timer, tables, -1, -1, hip_stream,
                                     node_codons_launch(f, c, node, false, &group_ll));
  c.before_smoothing = nullptr;
  return rc;
}

int asr_node_codons_device(lh_family* f, const std::string& W, const TreeBatch& b, const LineageCall& c, int node, void* hip_stream) {
  const int chunk = (int)std::min<size_t>(b.n, node_codons_group(f, b.T, b.R, c.P));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || node_codons_workspace(f, chunk, b.T, b.R, c.P, true, &ws)) return 1;
  return lineage_asr_device(f, W, b, c, chunk, ws, &lh_family::node_codons_timer, hip_stream,
                            node_codons_launch(f, c, node, true, nullptr));
}

LineageCall node_codons_call(lh_family* f, int P, const int32_t* path, const lh_node_codons_outputs* outs) {
  const lh_node_codons_outputs o = outs ? *outs : lh_node_codons_outputs{};
  return {nullptr, path, P, 0, node_codons_rows(f, false, o), o.log_offset, o.loglik, o.weight_stats};
}
LineageCall node_codons_call(lh_family* f, int P, const double* naive_codons, const int32_t* path, double* codons, double* change) {
  lh_node_codons_outputs o{};
  o.codons = codons;
  o.change = change;
  return {naive_codons, path, P, 0, node_codons_rows(f, true, o)};
}

// ---- K15: exact amino-acid replacement posteriors along the edges of a seed's lineage (lh_codon_edges.hip) ----

// K15's per-row outputs.  Row 0 as K14's: the eval form's site_base, the given-rates form's naive codon posteriors (no copy
// of its own: asr_entry's sub-batch rule adds its bytes).
enum { kCeCounts = 1, kCeAa, kCeSeed, kCeEdgeChange, kCeEdgeLoad, kCeCond };
std::vector<RowOut> codon_edges_rows(lh_family* f, bool given, int P, const lh_codon_edges_outputs& o, double* cond_edge) {
  AncestralWs& a = f->anc;
  CodonEdgesWs& k = f->codon_edges;
  const size_t L = f->host.n_sites, C = f->codon.n_codons;
  return {{nullptr, given ? C * 125 : L * 5, nullptr, &a.site_base},
          {o.codon_counts, C * 4, &k.out_cc, &k.cc, false, o.weighted_codon_counts, &k.partial_c, &k.out_wcc},
          {o.aa_counts, C * 441, &k.out_aa, &k.aa, false, o.weighted_aa_counts, &k.partial_a, &k.out_waa},
          {o.seed_change, C * 3, &k.out_sc, &k.sc, false, o.weighted_seed_change, &k.partial_s, &k.out_wsc},
          {o.edge_change, ((size_t)P + 1) * C * 3, &k.out_ec, nullptr},
          {o.edge_load, ((size_t)P + 1) * 2, &k.out_el, nullptr},
          {cond_edge, (size_t)P * L * 80, &k.out_cond, nullptr}};
}

int codon_edges_check(const lh_family* f, const std::string& W, const TreeBatch& b, int P, int seed_tip) {
  if (edges_check(f, W, b, P, seed_tip)) return 1;
  if (f->codon.frame < 0) return fail(W + ": lh_family_set_codons has not been called (no frame set)");
  return 0;
}

// samples per launch group of K15: its own bytes are K15b's per-slot partials, K15m's tables and K14's group arrays
// (LH_CODON_EDGES_MB: the budget, a test hook)
size_t codon_edges_group(const lh_family* f, int T, int R, int P) {
  const lh::CondEdgeWsBytes y = lh::cond_edge_ws_bytes(R, f->host.n_prune, P);
  const size_t hook = (size_t)lh::debug_options().codon_edges_mb;
  return lineage_group(f, T, R, P, y.part + y.table + node_codons_bytes(f), hook ? hook << 20 : (size_t)8 << 30);
}

int codon_edges_workspace(lh_family* f, int chunk, int T, int R, int P, bool given, bool ec_tmp, lh::AncWs* ws) {
  CodonEdgesWs& e = f->codon_edges;
  const lh::CondEdgeWsBytes y = lh::cond_edge_ws_bytes(R, f->host.n_prune, P);
  const size_t m = chunk;
  return lineage_workspace(f, chunk, T, R, P, true, &e.part, y.part, ws) || e.table.ensure(y.table * m) ||
         (ec_tmp && e.ec_tmp.ensure(sizeof(double) * ((size_t)P + 1) * f->codon.n_codons * 3 * m)) ||
         naive_codons_workspace(f, chunk, given);
}

// K15b + K15m on a launch group, the naive codon posteriors of every codon (as node_codons_launch) and the contraction
auto codon_edges_launch(lh_family* f, const LineageCall& c, bool given, const double* const* group_ll) {
  return [f, &c, given, group_ll](const TreeBatch& g, size_t off, const double* rates, const double* naive_prob,
                                  const lh::AncWs& ws, hipStream_t stream) -> int {
    Workspace& w = f->ws;
    NodeCodonsWs& k = f->node_codons;
    CodonEdgesWs& e = f->codon_edges;
    KernelTimer<2>& t = f->codon_edges_stage_timer;
    const std::vector<RowOut>& r = c.rows;
    const double *Q, *site_base;
    if (naive_codons_inputs(f, given, g.n, naive_prob, stream, &Q, &site_base)) return 1;
    if (f->profile && t.begin(stream)) return 1;
    if (lh::launch_cond_edges(f->host, g.n, g.R, g.T, g.ops, g.brlen, rates, w.eig.get<double>(), g.pi, w.site_lik.get<double>(),
                              w.site_scal.get<int32_t>(), site_base, c.path + off * c.P, c.P, c.seed_tip, ws,
                              e.table.get<double>(), r[kCeCond].group(off), w.prune.hdr, f->err_flag, stream))
      return 1;
    if (!given)
      lh::launch_naive_codons(k.tab, g.n, k.windows.get<const double>(), k.genes.get<const double>(), k.naive.get<double>(), stream);
    if (f->profile && t.mark(1, stream)) return 1;
    double *load = r[kCeEdgeLoad].group(off), *ec = r[kCeEdgeChange].group(off);
    if (load && !ec) ec = e.ec_tmp.get<double>();
    lh::launch_codon_edges(f->host, g.n, f->codon.n_codons, f->codon.frame, c.P, e.table.get<const double>(), Q, ws.plen,
                           group_ll ? *group_ll : nullptr, r[kCeCounts].group(off), r[kCeAa].group(off), r[kCeSeed].group(off),
                           ec, load, stream);
    if (f->profile && t.end(stream)) return 1;
    return 0;
  };
}

bool codon_edges_tmp(const LineageCall& c) { return c.rows[kCeEdgeLoad].p && !c.rows[kCeEdgeChange].p; }

int eval_codon_edges_device(lh_family* f, const std::string& W, const TreeBatch& b, LineageCall& c, void* hip_stream) {
  if (ancestral_table(f, W) || node_codons_tables(f, W)) return 1;
  const int chunk = (int)std::min<size_t>(b.n, std::min(codon_edges_group(f, b.T, b.R, c.P), eval_group(f, b.T, b.R)));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || codon_edges_workspace(f, chunk, b.T, b.R, c.P, false, codon_edges_tmp(c), &ws))
    return 1;
  const double* group_ll = nullptr;
  c.before_smoothing = naive_codons_k9(f, &lh_family::codon_edges_k9_timer, &group_ll);
  // K11c and K12c check the paths wherever a table is formed
  const bool tables = std::any_of(c.rows.begin() + 1, c.rows.end(), [](const RowOut& r) { return r.wanted(); });
  const int rc = lineage_eval_device(f, W, b, c, chunk, ws, &lh_family::codon_edges_timer, tables, -1, -1, hip_stream,
                                     codon_edges_launch(f, c, false, &group_ll));
  c.before_smoothing = nullptr;
  return rc;
}

int asr_codon_edges_device(lh_family* f, const std::string& W, const TreeBatch& b, const LineageCall& c, void* hip_stream) {
  const int chunk = (int)std::min<size_t>(b.n, codon_edges_group(f, b.T, b.R, c.P));
  lh::AncWs ws;
  if (ensure_workspace(f, chunk, b.R, b.T) || codon_edges_workspace(f, chunk, b.T, b.R, c.P, true, codon_edges_tmp(c), &ws))
    return 1;
  return lineage_asr_device(f, W, b, c, chunk, ws, &lh_family::codon_edges_timer, hip_stream,
                            codon_edges_launch(f, c, true, nullptr));
}

LineageCall codon_edges_call(lh_family* f, int P, const int32_t* path, int seed_tip, const lh_codon_edges_outputs* outs) {
  const lh_codon_edges_outputs o = outs ? *outs : lh_codon_edges_outputs{};
  return {nullptr, path, P, seed_tip, codon_edges_rows(f, false, P, o, nullptr), o.log_offset, o.loglik, o.weight_stats};
}
LineageCall codon_edges_call(lh_family* f, int P, const double* naive_codons, const int32_t* path, int seed_tip,
                             double* codon_counts, double* aa_counts, double* seed_change, double* edge_change, double* edge_load,
                             double* cond_edge) {
  lh_codon_edges_outputs o{};
  o.codon_counts = codon_counts;
  o.aa_counts = aa_counts;
  o.seed_change = seed_change;
  o.edge_change = edge_change;
  o.edge_load = edge_load;
  return {naive_codons, path, P, seed_tip, codon_edges_rows(f, true, P, o, cond_edge)};
}

// ---- the bodies of the entry points of K11 to K15 ----
// check(): the family's argument check; `missing`: one of the entry point's own arrays (path, the given-rates forms'
// input, an `at` form's slots) is null; call(): its LineageCall, built behind those tests; run(batch, call, stream): its
// _device form's body.  slot: the `at` forms' (K13, K14), the node is slot[i], a slot of its own path for every row.
// `device`: the arrays are the device's and the call is queued on hip_stream; else they are the host's, and the device
// copies of the per-row outputs bound the batch.

// The eval forms: a batch whose copies pass out_mb MiB is refused (K11's rule).
template <class Check, class Call, class Run>
int eval_entry(lh_family* f, const std::string& W, const TreeBatch& b, bool missing, const int32_t* slot, int out_mb,
               bool device, void* hip_stream, Check&& check, Call&& call, Run&& run) {
  if (int rc = check_batch(f, W, b, true)) return rc > 0;
  if (check()) return 1;
  DeviceGuard guard(f);
  if (!b.has_arrays() || missing) return fail(W + ": null array");
  LineageCall c = call();
  c.slot = slot;
  if (device) return run(b, c, hip_stream);
  if (!c.asked()) return 0;
  if (refuse_oversize(W, b.n, c, out_mb)) return 1;
  return lineage_batch(f, W, b, c, b.n, [&](const TreeBatch& dev, LineageCall d) { return run(dev, d, nullptr); });
}

// The given-rates (asr) forms.  out_mb 0: no refusal, sub-batches bound the device copies of the inputs and outputs at
// 1 GiB (marg: 32 P L bytes per sample).  The input is staged at row 0's width: where the family declares row 0 with a copy
// (K11: ancestral_rows) copy_bytes has counted it, where it declares none (K14, K15) its bytes are added here.
template <class Check, class Call, class Run>
int asr_entry(lh_family* f, const std::string& W, const TreeBatch& b, bool missing, const int32_t* slot, int out_mb,
              bool device, void* hip_stream, Check&& check, Call&& call, Run&& run) {
  if (int rc = check_batch(f, W, b)) return rc > 0;
  if (check()) return 1;
  DeviceGuard guard(f);
  if (!b.has_arrays() || missing) return fail(W + ": null array");
  LineageCall c = call();
  c.slot = slot;
  if (!c.asked()) return 0;  // nothing asked for
  if (device) return run(b, c, hip_stream);
  size_t sub = b.n;
  if (out_mb) {
    if (refuse_oversize(W, b.n, c, out_mb)) return 1;
  } else {
    const RowOut& in = c.rows[kSiteBase];
    const size_t per = c.copy_bytes(true) + (in.copy ? 0 : in.bytes(1));
    sub = std::max<size_t>(1, std::min<size_t>(b.n, ((size_t)1 << 30) / std::max<size_t>(per, 1)));
  }
  return lineage_batch(f, W, b, c, sub, [&](const TreeBatch& dev, const LineageCall& d) { return run(dev, d, nullptr); });
}

int asr_marginals_entry(lh_family* f, const TreeBatch& b, const double* naive_prob, const int32_t* path, int P, double* marg,
                        double* rate_post, bool device, void* hip_stream) {
  const std::string W = "lh_asr_marginals_batch";
  return asr_entry(
      f, W, b, !naive_prob || !path, nullptr, 0, device, hip_stream, [&] { return ancestral_check(f, W, b, P); },
      [&] { return LineageCall{naive_prob, path, P, 0, ancestral_rows(f, P, b.R, nullptr, marg, rate_post, nullptr, nullptr)}; },
      [&](const TreeBatch& g, const LineageCall& c, void* s) { return asr_marginals_device(f, W, g, c, s); });
}

int eval_ancestral_entry(lh_family* f, const TreeBatch& b, const int32_t* path, int P, const lh_ancestral_outputs* outs,
                         bool device, void* hip_stream) {
  const std::string W = "lh_eval_ancestral_batch";
  return eval_entry(
      f, W, b, !path, nullptr, lh::debug_options().anc_out_mb, device, hip_stream, [&] { return ancestral_check(f, W, b, P); },
      [&] { return ancestral_call(f, P, b.R, path, outs); },
      [&](const TreeBatch& g, LineageCall& c, void* s) { return eval_ancestral_device(f, W, g, c, s); });
}

int asr_edges_entry(lh_family* f, const TreeBatch& b, const double* naive_prob, const int32_t* path, int P, int seed_tip,
                    const lh_edges_outputs* outs, bool device, void* hip_stream) {
  const std::string W = "lh_asr_edges_batch";
  return asr_entry(
      f, W, b, !naive_prob || !path, nullptr, lh::debug_options().edge_out_mb, device, hip_stream,
      [&] { return edges_check(f, W, b, P, seed_tip); }, [&] { return edges_call(f, P, b.R, naive_prob, path, seed_tip, outs); },
      [&](const TreeBatch& g, const LineageCall& c, void* s) { return asr_edges_device(f, W, g, c, s); });
}

int eval_edges_entry(lh_family* f, const TreeBatch& b, const int32_t* path, int P, int seed_tip, const lh_eval_edges_outputs* outs,
                     bool device, void* hip_stream) {
  const std::string W = "lh_eval_edges_batch";
  return eval_entry(
      f, W, b, !path, nullptr, lh::debug_options().edge_out_mb, device, hip_stream,
      [&] { return edges_check(f, W, b, P, seed_tip); },
      [&] { return edges_call(f, P, b.R, nullptr, path, seed_tip, outs ? *outs : lh_eval_edges_outputs{}); },
      [&](const TreeBatch& g, LineageCall& c, void* s) { return eval_edges_device(f, W, g, c, s); });
}

int candidates_entry(lh_family* f, const std::string& W, const TreeBatch& b, const int32_t* path, int P, int node, bool at,
                     const int32_t* slot, const lh_ancestral_candidates_outputs* outs, bool device, void* hip_stream) {
  return eval_entry(
      f, W, b, !path || (at && !slot), slot, lh::debug_options().anc_out_mb, device, hip_stream, [&] { return probs_check(f, W, b, P, node, at); },
      [&] { return probs_call(f, P, path, outs); },
      [&](const TreeBatch& g, LineageCall& c, void* s) { return eval_probs_device(f, W, g, c, node, s); });
}

int eval_node_codons_entry(lh_family* f, const std::string& W, const TreeBatch& b, const int32_t* path, int P, int node, bool at,
                           const int32_t* slot, const lh_node_codons_outputs* outs, bool device, void* hip_stream) {
  return eval_entry(
      f, W, b, !path || (at && !slot), slot, lh::debug_options().anc_out_mb, device, hip_stream,
      [&] { return node_codons_check(f, W, b, P, node, at); }, [&] { return node_codons_call(f, P, path, outs); },
      [&](const TreeBatch& g, LineageCall& c, void* s) { return eval_node_codons_device(f, W, g, c, node, s); });
}

int asr_node_codons_entry(lh_family* f, const std::string& W, const TreeBatch& b, const double* naive_codons, const int32_t* path,
                          int P, int node, bool at, const int32_t* slot, double* codons, double* change, bool device,
                          void* hip_stream) {
  return asr_entry(
      f, W, b, !naive_codons || !path || (at && !slot), slot, 0, device, hip_stream, [&] { return node_codons_check(f, W, b, P, node, at); },
      [&] { return node_codons_call(f, P, naive_codons, path, codons, change); },
      [&](const TreeBatch& g, const LineageCall& c, void* s) { return asr_node_codons_device(f, W, g, c, node, s); });
}

int eval_codon_edges_entry(lh_family* f, const TreeBatch& b, const int32_t* path, int P, int seed_tip,
                           const lh_codon_edges_outputs* outs, bool device, void* hip_stream) {
  const std::string W = "lh_eval_codon_edges_batch";
  return eval_entry(
      f, W, b, !path, nullptr, lh::debug_options().edge_out_mb, device, hip_stream,
      [&] { return codon_edges_check(f, W, b, P, seed_tip); }, [&] { return codon_edges_call(f, P, path, seed_tip, outs); },
      [&](const TreeBatch& g, LineageCall& c, void* s) { return eval_codon_edges_device(f, W, g, c, s); });
}

int asr_codon_edges_entry(lh_family* f, const TreeBatch& b, const double* naive_codons, const int32_t* path, int P, int seed_tip,
                          double* codon_counts, double* aa_counts, double* seed_change, double* edge_change, double* edge_load,
                          double* cond_edge, bool device, void* hip_stream) {
  const std::string W = "lh_asr_codon_edges_batch";
  return asr_entry(
      f, W, b, !naive_codons || !path, nullptr, 0, device, hip_stream, [&] { return codon_edges_check(f, W, b, P, seed_tip); },
      [&] {
        return codon_edges_call(f, P, naive_codons, path, seed_tip, codon_counts, aa_counts, seed_change, edge_change, edge_load,
                                cond_edge);
      },
      [&](const TreeBatch& g, const LineageCall& c, void* s) { return asr_codon_edges_device(f, W, g, c, s); });
}

}  // namespace

extern "C" {

int lh_asr_marginals_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                  const double* brlen, const double* er, const double* pi, const double* rates, int32_t R,
                                  const double* naive_prob, const int32_t* path, int32_t P, double* marg, double* rate_post,
                                  void* hip_stream) {
  return asr_marginals_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_prob, path, P, marg, rate_post, true,
                             hip_stream);
}

int lh_asr_marginals_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                           const double* er, const double* pi, const double* rates, int32_t R, const double* naive_prob,
                           const int32_t* path, int32_t P, double* marg, double* rate_post) {
  return asr_marginals_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_prob, path, P, marg, rate_post, false,
                             nullptr);
}

int lh_eval_ancestral_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                   const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                   const int32_t* path, int32_t P, const lh_ancestral_outputs* outs, void* hip_stream) {
  return eval_ancestral_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, outs, true, hip_stream);
}

int lh_eval_ancestral_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                            const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path, int32_t P,
                            const lh_ancestral_outputs* outs) {
  return eval_ancestral_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, outs, false, nullptr);
}

int lh_ancestral_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::anc_timer, ms, n_launches);
}

int lh_asr_edges_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                              const double* er, const double* pi, const double* rates, int32_t R, const double* naive_prob,
                              const int32_t* path, int32_t P, int32_t seed_tip, const lh_edges_outputs* outs, void* hip_stream) {
  return asr_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_prob, path, P, seed_tip, outs, true,
                         hip_stream);
}

int lh_asr_edges_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                       const double* er, const double* pi, const double* rates, int32_t R, const double* naive_prob,
                       const int32_t* path, int32_t P, int32_t seed_tip, const lh_edges_outputs* outs) {
  return asr_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_prob, path, P, seed_tip, outs, false,
                         nullptr);
}

int lh_eval_edges_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                               const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path, int32_t P,
                               int32_t seed_tip, const lh_eval_edges_outputs* outs, void* hip_stream) {
  return eval_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, seed_tip, outs, true, hip_stream);
}

int lh_eval_edges_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                        const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path, int32_t P,
                        int32_t seed_tip, const lh_eval_edges_outputs* outs) {
  return eval_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, seed_tip, outs, false, nullptr);
}

int lh_edges_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::edges_timer, ms, n_launches);
}

int lh_family_set_ancestral_candidates(lh_family* f, int32_t K, const uint8_t* seqs) {
  const std::string W = "lh_family_set_ancestral_candidates";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  AncProbsWs& p = f->probs;
  p.K = 0;  // a call that fails leaves no candidates
  if (f->host.n_seqs < 1) return fail(W + ": family was created without an MSA (forward-only)");
  if (!f->cand.twin) return fail(W + ": no constrained forward sweep for this family: " + f->cand.twin_error);
  if (K < 1 || K > 65536) return fail(W + ": K must be 1 .. 65536 candidates");
  if (!seqs) return fail(W + ": null array");
  const size_t L = f->host.n_sites;
  for (size_t i = 0; i < (size_t)K * L; ++i)
    if (seqs[i] > 4)
      return fail(W + ": candidate " + std::to_string(i / L) + ", site " + std::to_string(i % L) + ": base " +
                  std::to_string(seqs[i]) + " is not one of A,C,G,T = 0..3 or 4 (the site is left open)");
  if (p.seqs.ensure((size_t)K * L) || stage_inputs(f, {{seqs, (size_t)K * L, &p.seqs}})) return 1;
  LH_HIP(hipDeviceSynchronize());
  p.K = K;
  return 0;
}

int lh_ancestral_candidates_info(const lh_family* f, int32_t* n_candidates, int32_t* n_sites) {
  if (!f) return fail("lh_ancestral_candidates_info: null family");
  if (n_candidates) *n_candidates = f->probs.K;
  if (n_sites) *n_sites = f->host.n_sites;
  return 0;
}

int lh_eval_ancestral_candidates_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                              const double* brlen, const double* er, const double* pi, const double* alpha,
                                              int32_t R, const int32_t* path, int32_t P, int32_t node,
                                              const lh_ancestral_candidates_outputs* outs, void* hip_stream) {
  return candidates_entry(f, "lh_eval_ancestral_candidates_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, node,
                          false, nullptr, outs, true, hip_stream);
}

int lh_eval_ancestral_candidates_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                       const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                       const int32_t* path, int32_t P, int32_t node,
                                       const lh_ancestral_candidates_outputs* outs) {
  return candidates_entry(f, "lh_eval_ancestral_candidates_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, node,
                          false, nullptr, outs, false, nullptr);
}

int lh_eval_ancestral_candidates_at_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                                 const double* brlen, const double* er, const double* pi, const double* alpha,
                                                 int32_t R, const int32_t* path, int32_t P, const int32_t* slot,
                                                 const lh_ancestral_candidates_outputs* outs, void* hip_stream) {
  return candidates_entry(f, "lh_eval_ancestral_candidates_at_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, 0,
                          true, slot, outs, true, hip_stream);
}

int lh_eval_ancestral_candidates_at_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                          const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                          const int32_t* path, int32_t P, const int32_t* slot,
                                          const lh_ancestral_candidates_outputs* outs) {
  return candidates_entry(f, "lh_eval_ancestral_candidates_at_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, 0,
                          true, slot, outs, false, nullptr);
}

int lh_ancestral_candidates_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  double skeleton[3] = {}, stage[2] = {};
  if (profile_read(f, &lh_family::probs_timer, skeleton, n_launches) ||
      profile_read(f, &lh_family::probs_stage_timer, stage, nullptr))
    return 1;
  if (ms) {
    ms[0] = stage[0];
    ms[1] = stage[1];
    ms[2] = skeleton[2];
  }
  return 0;
}

int lh_eval_node_codons_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                     const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                     const int32_t* path, int32_t P, int32_t node, const lh_node_codons_outputs* outs,
                                     void* hip_stream) {
  return eval_node_codons_entry(f, "lh_eval_node_codons_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, node,
                                false, nullptr, outs, true, hip_stream);
}

int lh_eval_node_codons_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                              const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path, int32_t P,
                              int32_t node, const lh_node_codons_outputs* outs) {
  return eval_node_codons_entry(f, "lh_eval_node_codons_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, node,
                                false, nullptr, outs, false, nullptr);
}

int lh_eval_node_codons_at_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                        const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                        const int32_t* path, int32_t P, const int32_t* slot, const lh_node_codons_outputs* outs,
                                        void* hip_stream) {
  return eval_node_codons_entry(f, "lh_eval_node_codons_at_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, 0,
                                true, slot, outs, true, hip_stream);
}

int lh_eval_node_codons_at_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                                 const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path,
                                 int32_t P, const int32_t* slot, const lh_node_codons_outputs* outs) {
  return eval_node_codons_entry(f, "lh_eval_node_codons_at_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, 0,
                                true, slot, outs, false, nullptr);
}

int lh_asr_node_codons_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* rates, int32_t R,
                                    const double* naive_codons, const int32_t* path, int32_t P, int32_t node, double* codons,
                                    double* change, void* hip_stream) {
  return asr_node_codons_entry(f, "lh_asr_node_codons_batch", {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_codons,
                               path, P, node, false, nullptr, codons, change, true, hip_stream);
}

int lh_asr_node_codons_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                             const double* er, const double* pi, const double* rates, int32_t R, const double* naive_codons,
                             const int32_t* path, int32_t P, int32_t node, double* codons, double* change) {
  return asr_node_codons_entry(f, "lh_asr_node_codons_batch", {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_codons,
                               path, P, node, false, nullptr, codons, change, false, nullptr);
}

int lh_asr_node_codons_at_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                       const double* brlen, const double* er, const double* pi, const double* rates, int32_t R,
                                       const double* naive_codons, const int32_t* path, int32_t P, const int32_t* slot,
                                       double* codons, double* change, void* hip_stream) {
  return asr_node_codons_entry(f, "lh_asr_node_codons_at_batch", {n, T, max_depth, ops, brlen, er, pi, rates, R, true},
                               naive_codons, path, P, 0, true, slot, codons, change, true, hip_stream);
}

int lh_asr_node_codons_at_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                                const double* er, const double* pi, const double* rates, int32_t R, const double* naive_codons,
                                const int32_t* path, int32_t P, const int32_t* slot, double* codons, double* change) {
  return asr_node_codons_entry(f, "lh_asr_node_codons_at_batch", {n, T, max_depth, ops, brlen, er, pi, rates, R, true},
                               naive_codons, path, P, 0, true, slot, codons, change, false, nullptr);
}

int lh_node_codon_classes(uint8_t* classes) {
  if (!classes) return fail("lh_node_codon_classes: null array");
  lh::node_codon_classes(classes);
  return 0;
}

int lh_node_codons_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  double skeleton[3] = {}, stage[2] = {}, k9 = 0.0;
  if (profile_read(f, &lh_family::node_codons_timer, skeleton, n_launches) ||
      profile_read(f, &lh_family::node_codons_stage_timer, stage, nullptr) ||
      profile_read(f, &lh_family::node_codons_k9_timer, &k9, nullptr))
    return 1;
  if (ms) {
    ms[0] = k9 + stage[0];
    ms[1] = stage[1];
    ms[2] = skeleton[2];
  }
  return 0;
}

int lh_eval_codon_edges_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                     const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                     const int32_t* path, int32_t P, int32_t seed_tip, const lh_codon_edges_outputs* outs,
                                     void* hip_stream) {
  return eval_codon_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, seed_tip, outs, true, hip_stream);
}

int lh_eval_codon_edges_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                              const double* er, const double* pi, const double* alpha, int32_t R, const int32_t* path, int32_t P,
                              int32_t seed_tip, const lh_codon_edges_outputs* outs) {
  return eval_codon_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, alpha, R}, path, P, seed_tip, outs, false, nullptr);
}

int lh_asr_codon_edges_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* rates, int32_t R,
                                    const double* naive_codons, const int32_t* path, int32_t P, int32_t seed_tip,
                                    double* codon_counts, double* aa_counts, double* seed_change, double* edge_change,
                                    double* edge_load, double* cond_edge, void* hip_stream) {
  return asr_codon_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_codons, path, P, seed_tip,
                               codon_counts, aa_counts, seed_change, edge_change, edge_load, cond_edge, true, hip_stream);
}

int lh_asr_codon_edges_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                             const double* er, const double* pi, const double* rates, int32_t R, const double* naive_codons,
                             const int32_t* path, int32_t P, int32_t seed_tip, double* codon_counts, double* aa_counts,
                             double* seed_change, double* edge_change, double* edge_load, double* cond_edge) {
  return asr_codon_edges_entry(f, {n, T, max_depth, ops, brlen, er, pi, rates, R, true}, naive_codons, path, P, seed_tip,
                               codon_counts, aa_counts, seed_change, edge_change, edge_load, cond_edge, false, nullptr);
}

int lh_codon_edge_symbols(uint8_t* sym) {
  if (!sym) return fail("lh_codon_edge_symbols: null array");
  lh::codon_edge_symbols(sym);
  return 0;
}

int lh_codon_edges_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  double skeleton[3] = {}, stage[2] = {}, k9 = 0.0;
  if (profile_read(f, &lh_family::codon_edges_timer, skeleton, n_launches) ||
      profile_read(f, &lh_family::codon_edges_stage_timer, stage, nullptr) ||
      profile_read(f, &lh_family::codon_edges_k9_timer, &k9, nullptr))
    return 1;
  if (ms) {
    ms[0] = k9 + stage[0];
    ms[1] = stage[1];
    ms[2] = skeleton[2];
  }
  return 0;
}

int lh_forward_batch(lh_family* f, int32_t n, const double* em, double* loglik, const lh_eval_outputs* outs) {
  if (!f) return fail("lh_forward_batch: null family");
  DeviceGuard guard(f);
  if (n <= 0) return n == 0 ? 0 : fail("lh_forward_batch: negative batch size");
  if (!em || !loglik) return fail("lh_forward_batch: null array");
  const size_t C = f->host.n_xmsa, FS = f->host.forward_size, SS = f->host.scaler_size;
  const lh_eval_outputs none{};
  const lh_eval_outputs& o = outs ? *outs : none;
  HostOutputs& out = f->out;
  lh_eval_outputs d_outs{};
  if (out.loglik.ensure(sizeof(double) * n) || out_buf(o.forward, out.forward, sizeof(double) * FS * n, &d_outs.forward) ||
      out_buf(o.scaler_counts, out.scaler_counts, sizeof(int32_t) * SS * n, &d_outs.scaler_counts) ||
      stage_inputs(f, {{em, sizeof(double) * C * n, &f->in.em}}))
    return 1;
  if (run_forward(f, n, 1, nullptr, nullptr, nullptr, f->in.em.get<const double>(), nullptr, out.loglik.get<double>(),
                  &d_outs, 0, nullptr))
    return 1;
  return copy_back(f, nullptr,
                   {{loglik, out.loglik.get(), sizeof(double) * n},
                    {o.forward, d_outs.forward, sizeof(double) * FS * n},
                    {o.scaler_counts, d_outs.scaler_counts, sizeof(int32_t) * SS * n}});
}

int lh_sample_forward_batch(lh_family* f, int32_t n, const double* em, const uint32_t* words, double* loglik, int32_t* states,
                            const lh_eval_outputs* outs) {
  const std::string W = "lh_sample_forward_batch";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (!f->have_sampler) return fail(W + ": lh_family_set_sampler has not been called");
  if (n <= 0) return n == 0 ? 0 : fail(W + ": negative batch size");
  if (!em || !words || !states) return fail(W + ": null array");
  const size_t C = f->host.n_xmsa, FS = f->host.forward_size, SS = f->host.scaler_size;
  const size_t NW = f->sampler.words_per_sample, S = f->sampler.states_per_sample;
  const lh_eval_outputs none{};
  const lh_eval_outputs& o = outs ? *outs : none;
  HostOutputs& out = f->out;
  // the forward arrays stay where K4 reads them (as in lh_eval_sample_batch); outs->forward is a copy of exactly those
  lh_eval_outputs d_outs{};
  if (out.loglik.ensure(sizeof(double) * n) || out.states.ensure(sizeof(int32_t) * S * n) ||
      f->forward_dev.ensure(sizeof(double) * FS * n) ||
      out_buf(o.scaler_counts, out.scaler_counts, sizeof(int32_t) * SS * n, &d_outs.scaler_counts) ||
      stage_inputs(f, {{em, sizeof(double) * C * n, &f->in.em}, {words, sizeof(uint32_t) * NW * n, &f->in.words}}))
    return 1;
  d_outs.forward = f->forward_dev.get<double>();
  if (run_forward(f, n, 1, nullptr, nullptr, nullptr, f->in.em.get<const double>(), nullptr, out.loglik.get<double>(),
                  &d_outs, 0, nullptr))
    return 1;
  lh::launch_sample(f->sampler, f->sampler_dev, n, d_outs.forward, FS, f->in.words.get<const uint32_t>(), (int)NW,
                    out.states.get<int32_t>(), nullptr);
  LH_HIP(hipGetLastError());
  return copy_back(f, nullptr,
                   {{loglik, out.loglik.get(), sizeof(double) * n},
                    {states, out.states.get(), sizeof(int32_t) * S * n},
                    {o.forward, d_outs.forward, sizeof(double) * FS * n},
                    {o.scaler_counts, d_outs.scaler_counts, sizeof(int32_t) * SS * n}});
}

int lh_posterior_forward_batch(lh_family* f, int32_t n, const double* em, double* loglik, double* posterior) {
  const std::string W = "lh_posterior_forward_batch";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (!f->have_sampler) return fail(W + ": lh_family_set_sampler has not been called");
  if (n <= 0) return n == 0 ? 0 : fail(W + ": negative batch size");
  if (!em) return fail(W + ": null array");
  const size_t C = f->host.n_xmsa, FS = f->host.forward_size;
  HostOutputs& out = f->out;
  if (out.loglik.ensure(sizeof(double) * n) || f->forward_dev.ensure(sizeof(double) * FS * n) ||
      stage_inputs(f, {{em, sizeof(double) * C * n, &f->in.em}}))
    return 1;
  double* post = f->forward_dev.get<double>();  // K5 overwrites the forward arrays in place
  lh_eval_outputs eo{nullptr, nullptr, post, nullptr};
  if (run_forward(f, n, 1, nullptr, nullptr, nullptr, f->in.em.get<const double>(), nullptr, out.loglik.get<double>(), &eo, 0,
                  nullptr))
    return 1;
  lh::launch_posterior(f->sampler_dev, n, post, FS, out.loglik.get<const double>(), nullptr);
  LH_HIP(hipGetLastError());
  return copy_back(f, nullptr, {{loglik, out.loglik.get(), sizeof(double) * n}, {posterior, post, sizeof(double) * FS * n}});
}

int lh_eval_posterior_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                   const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                   const lh_posterior_outputs* outs, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, "lh_eval_posterior_batch_device", b, true)) return rc > 0;
  DeviceGuard guard(f);
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const lh_posterior_outputs none{};
  const lh_posterior_outputs& o = outs ? *outs : none;
  const size_t FS = f->host.forward_size;
  PosteriorWs& pw = f->post;
  // the forward arrays go where the posteriors are wanted: K5 overwrites them in place
  double *post = o.posterior, *ll = o.loglik, *w = nullptr, *stats = o.weight_stats, *partial = nullptr;
  const bool reduce = o.weighted_sum || o.weight_stats;
  if (own(post, f->forward_dev, sizeof(double) * FS * n) || own(ll, pw.loglik, sizeof(double) * n) ||
      (reduce && (own(w, pw.weights, sizeof(double) * n) || own(stats, pw.stats, sizeof(double) * 3) ||
                  (o.weighted_sum && own(partial, pw.partial, sizeof(double) * FS * lh::posterior_slabs(n))))))
    return 1;
  lh_eval_outputs eo{nullptr, nullptr, post, nullptr};
  if (eval_device(f, b, ll, &eo, hip_stream)) return 1;
  if (f->profile && f->post_timer.begin(stream)) return 1;
  lh::launch_posterior(f->sampler_dev, n, post, FS, ll, stream);
  // (not WeightReduce: K5's reduction also sums the posteriors, through its slab partials)
  if (reduce) lh::launch_posterior_reduce(n, FS, post, ll, o.log_offset, w, partial, o.weighted_sum, stats, stream);
  if (f->profile && f->post_timer.end(stream)) return 1;
  LH_HIP(hipGetLastError());
  return 0;
}

int lh_eval_posterior_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                            const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                            const lh_posterior_outputs* outs) {
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, "lh_eval_posterior_batch", host, true)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays()) return fail("lh_eval_posterior_batch: null array");
  const lh_posterior_outputs none{};
  const lh_posterior_outputs& o = outs ? *outs : none;
  if (!o.posterior && !o.weighted_sum && !o.weight_stats && !o.loglik) return 0;  // nothing asked for
  const size_t FS = f->host.forward_size;
  HostOutputs& out = f->out;
  lh_posterior_outputs d{};
  TreeBatch dev;
  if (f->forward_dev.ensure(sizeof(double) * FS * n) || out.loglik.ensure(sizeof(double) * n) ||
      out_buf(o.weighted_sum, out.weighted_sum, sizeof(double) * FS, &d.weighted_sum) ||
      out_buf(o.weight_stats, out.weight_stats, sizeof(double) * 3, &d.weight_stats) ||
      stage_batch(f, host, {{o.log_offset, sizeof(double) * n, &f->in.log_offset}}, &dev))
    return 1;
  d.log_offset = o.log_offset ? f->in.log_offset.get<const double>() : nullptr;
  d.loglik = out.loglik.get<double>();
  d.posterior = f->forward_dev.get<double>();
  if (lh_eval_posterior_batch_device(f, n, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, &d, nullptr)) return 1;
  return finish_batch(f, "lh_eval_posterior_batch", host,
                      {{o.loglik, d.loglik, sizeof(double) * n},
                       {o.posterior, d.posterior, sizeof(double) * FS * n},
                       {o.weighted_sum, d.weighted_sum, sizeof(double) * FS},
                       {o.weight_stats, d.weight_stats, sizeof(double) * 3}});
}

int lh_posterior_profile_read(lh_family* f, double* ms_posterior, int64_t* n_launches) {
  return profile_read(f, &lh_family::post_timer, ms_posterior, n_launches);
}

// ---- K6: posterior probabilities of candidate naive sequences (lh_naive_probs.hip) ----

int lh_family_set_candidates(lh_family* f, int32_t K, const uint8_t* seqs, double* log_prior) {
  const std::string W = "lh_family_set_candidates";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  CandidateWs& cw = f->cand;
  if (f->host.n_seqs < 1) return fail(W + ": family was created without an MSA (forward-only)");
  if (!cw.twin) return fail(W + ": no constrained forward sweep for this family: " + cw.twin_error);
  if (K < 1 || K > 65536) return fail(W + ": K must be 1 .. 65536 candidates");
  if (!seqs) return fail(W + ": null array");
  const int L = f->host.n_sites, C = f->host.n_xmsa, NPr = f->host.n_prune;
  for (size_t i = 0; i < (size_t)K * L; ++i)
    if (seqs[i] > 4)
      return fail(W + ": candidate " + std::to_string(i / L) + ", site " + std::to_string(i % L) + ": base " +
                  std::to_string(seqs[i]) + " is not one of A,C,G,T,N = 0..4");
  // the u-column of (site, base), as lh_family_create numbers them
  std::vector<int32_t> site_pat(std::max(L, 1));
  LH_HIP(hipMemcpy(site_pat.data(), f->host.site_pat, sizeof(int32_t) * L, hipMemcpyDeviceToHost));
  auto ucol = [&](int i, int b) { return site_pat[i] < NPr ? b * NPr + site_pat[i] : 5 * NPr + b; };
  std::vector<int32_t> var_sites;
  std::vector<char> agrees(L, 1);
  for (int i = 0; i < L; ++i) {
    for (int k = 1; k < K && agrees[i]; ++k) agrees[i] = seqs[(size_t)k * L + i] == seqs[i];
    if (!agrees[i]) var_sites.push_back(i);
  }
  // K2a's list: the variable sites' u-columns first (the scoring kernel's LDS), then the rest of the agreeing sites'
  std::vector<int32_t> pos(f->host.n_ucol, -1), lem_cols;
  const size_t V = var_sites.size();
  std::vector<uint16_t> idx(V * K);
  for (size_t v = 0; v < V; ++v)
    for (int k = 0; k < K; ++k) {
      const int u = ucol(var_sites[v], seqs[(size_t)k * L + var_sites[v]]);
      if (pos[u] < 0) {
        pos[u] = (int32_t)lem_cols.size();
        lem_cols.push_back(u);
      }
      idx[v * K + k] = (uint16_t)pos[u];
    }
  const int n_vlem = (int)lem_cols.size();
  if ((size_t)n_vlem * sizeof(double) > lh::candidate_lds_limit())
    return fail(W + ": the candidates differ at too many (site, base) pairs for the scoring kernel's LDS (" +
                std::to_string(n_vlem) + ")");
  std::vector<double> agree;
  for (int i = 0; i < L; ++i)
    if (agrees[i]) {
      const int u = ucol(i, seqs[i]);
      if (pos[u] < 0) {
        pos[u] = (int32_t)lem_cols.size();
        lem_cols.push_back(u);
      }
    }
  agree.assign(lem_cols.size(), 0.0);
  for (int i = 0; i < L; ++i)
    if (agrees[i]) agree[pos[ucol(i, seqs[i])]] += 1.0;
  cw.tab.K = 0;  // the arguments are good: the old tables go before their buffers change (a call failing below leaves none)
  if (cw.seqs.ensure((size_t)K * L) || cw.idx.ensure(sizeof(uint16_t) * idx.size()) ||
      cw.agree.ensure(sizeof(double) * agree.size()) || cw.lem_cols.ensure(sizeof(int32_t) * lem_cols.size()) ||
      cw.prior.ensure(sizeof(double) * K) ||
      stage_inputs(f, {{seqs, (size_t)K * L, &cw.seqs},
                       {idx.empty() ? nullptr : idx.data(), sizeof(uint16_t) * idx.size(), &cw.idx},
                       {agree.empty() ? nullptr : agree.data(), sizeof(double) * agree.size(), &cw.agree},
                       {lem_cols.empty() ? nullptr : lem_cols.data(), sizeof(int32_t) * lem_cols.size(), &cw.lem_cols}}))
    return 1;
  // K6a: the constrained forward sweep, in groups of candidates (the indicator emissions take C doubles each)
  const int chunk = std::min(K, 4096);
  if (cw.em.ensure(sizeof(double) * chunk * C)) return 1;
  if (f->profile && f->prior_timer.begin(nullptr)) return 1;
  for (int off = 0; off < K; off += chunk) {
    const int m = std::min(chunk, K - off);
    lh::launch_candidate_indicators(m, L, C, cw.seqs.get<uint8_t>() + (size_t)off * L, cw.col_site, cw.col_base,
                                    cw.em.get<double>(), nullptr);
    if (run_forward(cw.twin, m, 1, nullptr, nullptr, nullptr, cw.em.get<const double>(), nullptr,
                    cw.prior.get<double>() + off, nullptr, 0, nullptr))
      return 1;
  }
  if (f->profile && f->prior_timer.end(nullptr)) return 1;
  LH_HIP(hipGetLastError());
  cw.tab = {K, (int32_t)V, (int32_t)lem_cols.size(), n_vlem, cw.idx.get<const uint16_t>(), cw.agree.get<const double>(),
            cw.prior.get<const double>()};
  return copy_back(f, nullptr, {{log_prior, cw.prior.get(), sizeof(double) * K}});
}

int lh_eval_candidates_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                    const lh_candidate_outputs* outs, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  const std::string W = "lh_eval_candidates_batch_device";
  if (int rc = check_batch(f, W, b)) return rc > 0;
  DeviceGuard guard(f);
  CandidateWs& cw = f->cand;
  const lh::CandidateTables& tab = cw.tab;
  if (tab.K == 0) return fail(W + ": lh_family_set_candidates has not been called");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const lh_candidate_outputs none{};
  const lh_candidate_outputs& o = outs ? *outs : none;
  double *ll = o.loglik, *partial = nullptr;
  WeightReduce wr;
  const bool reduce = o.weighted_sum || o.weight_stats;
  const int slabs = lh::candidate_slabs(n);
  if (own(ll, cw.loglik, sizeof(double) * n) || cw.lem.ensure(sizeof(double) * n * (size_t)tab.n_lem) ||
      cw.base.ensure(sizeof(double) * n) ||
      (reduce && (wr.prepare(n, cw.weights, cw.stats, o.weight_stats) ||
                  (o.weighted_sum && own(partial, cw.partial, sizeof(double) * slabs * (size_t)tab.K)))))
    return 1;
  const lh::LogEmRequest lem{cw.lem_cols.get<const int32_t>(), tab.n_lem, cw.lem.get<double>()};
  if (eval_device(f, b, ll, nullptr, hip_stream, lem)) return 1;
  if (f->profile && f->cand_timer.begin(stream)) return 1;
  if (reduce) wr.launch(n, ll, o.log_offset, stream);
  if (o.log_cand || o.weighted_sum)
    lh::launch_candidates(tab, n, cw.lem.get<const double>(), ll, o.weighted_sum ? wr.w : nullptr, cw.base.get<double>(),
                          o.log_cand, partial, stream);
  if (o.weighted_sum) lh::launch_slab_sum(slabs, tab.K, partial, o.weighted_sum, stream);
  if (f->profile && f->cand_timer.end(stream)) return 1;
  LH_HIP(hipGetLastError());
  return 0;
}

int lh_eval_candidates_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                             const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                             const lh_candidate_outputs* outs) {
  const std::string W = "lh_eval_candidates_batch";
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, W, host)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays()) return fail(W + ": null array");
  if (f->cand.tab.K == 0) return fail(W + ": lh_family_set_candidates has not been called");
  const lh_candidate_outputs none{};
  const lh_candidate_outputs& o = outs ? *outs : none;
  if (!o.log_cand && !o.weighted_sum && !o.weight_stats && !o.loglik) return 0;  // nothing asked for
  const size_t K = f->cand.tab.K;
  HostOutputs& out = f->out;
  lh_candidate_outputs d{};
  TreeBatch dev;
  if (out.loglik.ensure(sizeof(double) * n) || out_buf(o.log_cand, out.log_cand, sizeof(double) * K * n, &d.log_cand) ||
      out_buf(o.weighted_sum, out.weighted_sum, sizeof(double) * K, &d.weighted_sum) ||
      out_buf(o.weight_stats, out.weight_stats, sizeof(double) * 3, &d.weight_stats) ||
      stage_batch(f, host, {{o.log_offset, sizeof(double) * n, &f->in.log_offset}}, &dev))
    return 1;
  d.log_offset = o.log_offset ? f->in.log_offset.get<const double>() : nullptr;
  d.loglik = out.loglik.get<double>();
  if (lh_eval_candidates_batch_device(f, n, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, &d, nullptr)) return 1;
  return finish_batch(f, W.c_str(), host,
                      {{o.loglik, d.loglik, sizeof(double) * n},
                       {o.log_cand, d.log_cand, sizeof(double) * K * n},
                       {o.weighted_sum, d.weighted_sum, sizeof(double) * K},
                       {o.weight_stats, d.weight_stats, sizeof(double) * 3}});
}

int lh_candidates_info(const lh_family* f, int32_t* n_candidates, int32_t* n_sites) {
  if (!f) return fail("lh_candidates_info: null family");
  if (n_candidates) *n_candidates = f->cand.tab.K;
  if (n_sites) *n_sites = f->host.n_sites;
  return 0;
}

int lh_candidates_layout(const lh_family* f, int32_t* n_var_sites, int32_t* n_lem, int32_t* n_vlem) {
  if (!f) return fail("lh_candidates_layout: null family");
  const lh::CandidateTables& t = f->cand.tab;
  if (n_var_sites) *n_var_sites = t.V;
  if (n_lem) *n_lem = t.n_lem;
  if (n_vlem) *n_vlem = t.n_vlem;
  return 0;
}

int lh_candidates_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  double a = 0.0, b = 0.0;
  if (profile_read(f, &lh_family::prior_timer, &a, nullptr) || profile_read(f, &lh_family::cand_timer, &b, n_launches))
    return 1;
  if (ms) {
    ms[0] = a;
    ms[1] = b;
  }
  return 0;
}

// ---- K6c: naive sequences of sampled states, and the candidate store (lh_collect.hip) ----

}  // extern "C"

namespace {

// K6c's tables: pointers the family already holds (the twin's segments and junction matrices, K4's state classes, K6a's
// column map).  Fails when the family has no sampler or no twin.
int collect_tables(lh_family* f, const std::string& who, lh::CollectTables* t) {
  if (!f->have_sampler) return fail(who + ": lh_family_set_sampler has not been called");
  if (f->host.n_seqs < 1) return fail(who + ": family was created without an MSA (forward-only)");
  if (!f->cand.twin) return fail(who + ": no column tables for this family: " + f->cand.twin_error);
  const lh::DevFamily& w = f->cand.twin->host;
  *t = lh::CollectTables{};
  t->L = f->host.n_sites;
  t->has_d = f->host.has_d;
  t->states_per_sample = f->sampler.states_per_sample;
  t->n_cols = f->host.n_xmsa;
  t->seg_scale = w.idx_byte_offsets ? 8 : 1;
  t->seg_sentinel = w.n_ucol * t->seg_scale;
  auto seg = [](const lh::DevSegments& d) { return lh::CollectSegments{d.n_genes, d.n_chunks, d.inds_c}; };
  t->vg = seg(w.vgerm);
  t->jg = seg(w.jgerm);
  if (w.has_d) t->dg = seg(w.dgerm);
  auto junc = [](const lh::DevJunction& d, const lh::DevSampleJunction& s) {
    return lh::CollectJunction{d.n_rows, d.n_left, d.n_right, d.left_pad, d.right_pad, s.n_states,
                               d.left_xmsa, d.right_xmsa, d.nti_xmsa, s.state_class};
  };
  t->vd = junc(w.vd, f->sampler.vd);
  if (w.has_d) t->dj = junc(w.dj, f->sampler.dj);
  t->jcols = w.jcols;
  t->n_jcols = w.n_jcols;
  t->col_site = f->cand.col_site;
  t->col_base = f->cand.col_base;
  const int bits = lh::debug_options().collect_hash_bits;
  t->hash_mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
  if (lh::collect_lds_bytes(t->L) > 160 * 1024) return fail(who + ": alignment too long for the assembly kernel's LDS");
  return 0;
}

// assembles the batch's rows into the handle's workspace (seqs [n][L], hash [n]) from device states
int collect_launch(lh_family* f, const lh::CollectTables& t, int n, const int32_t* states, hipStream_t stream) {
  CollectWs& c = f->collect;
  if (c.seqs.ensure((size_t)n * t.L) || c.hash.ensure(sizeof(uint64_t) * n)) return 1;
  if (f->profile && f->collect_timer.begin(stream)) return 1;
  lh::launch_collect(t, n, states, c.seqs.get<uint8_t>(), c.hash.get<uint64_t>(), stream);
  LH_HIP(hipGetLastError());
  if (f->profile && f->collect_timer.end(stream)) return 1;
  c.n_last = n;
  return 0;
}


// The sequence store's operations, once for both features: `src` is the last batch's row source with n slots (the entry
// point has checked that there is one), W the entry point's name.
// ids[x] of slot x: -1 leaves it out, below s.K names a stored sequence, from s.K on a new one.  New ids must be
// consecutive, each with a slot of the batch, whose first is appended.  Every slot with an id is then compared with its
// stored sequence: the mismatching slots come back in ascending order.
template <class Rows>
int store_resolve(const std::string& W, SeqStore& s, const Rows& src, int32_t n, const int32_t* ids, int32_t* n_mismatch,
                  int32_t* mismatch) {
  if (n > 0 && !ids) return fail(W + ": null array");
  const int L = src.L;
  int32_t K_new = s.K;
  for (int32_t x = 0; x < n; ++x) {
    if (ids[x] < -1) return fail(W + ": id below -1");
    K_new = std::max(K_new, ids[x] + 1);
  }
  std::vector<int32_t> first((size_t)(K_new - s.K), -1), pairs;
  for (int32_t x = 0; x < n; ++x)
    if (ids[x] >= s.K && first[ids[x] - s.K] < 0) first[ids[x] - s.K] = x;
  for (size_t k = 0; k < first.size(); ++k) {
    if (first[k] < 0) return fail(W + ": new ids must be consecutive, each with a row of the batch");
    pairs.push_back(s.K + (int32_t)k);
    pairs.push_back(first[k]);
  }
  LH_HIP(hipDeviceSynchronize());
  if ((size_t)K_new > s.cap) {  // grow the store, keeping what it holds
    const size_t cap = std::max<size_t>({(size_t)K_new, 2 * s.cap, 256});
    DevBuf& nb = s.store[s.cur ^ 1];
    if (nb.ensure(cap * L)) return 1;
    if (s.K > 0) LH_HIP(hipMemcpy(nb.get(), s.store[s.cur].get(), (size_t)s.K * L, hipMemcpyDeviceToDevice));
    s.cur ^= 1;
    s.cap = cap;
  }
  if (n == 0) {
    if (n_mismatch) *n_mismatch = 0;
    return 0;
  }
  if (s.ids.ensure(sizeof(int32_t) * n) || s.flag.ensure(n) || s.pairs.ensure(sizeof(int32_t) * pairs.size())) return 1;
  LH_HIP(hipMemcpy(s.ids.get(), ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  if (!pairs.empty()) LH_HIP(hipMemcpy(s.pairs.get(), pairs.data(), sizeof(int32_t) * pairs.size(), hipMemcpyHostToDevice));
  uint8_t* store = s.store[s.cur].get<uint8_t>();
  lh::launch_store_append(src, K_new, (int)(pairs.size() / 2), s.pairs.get<const int32_t>(), store, nullptr);
  lh::launch_store_verify(src, K_new, s.ids.get<const int32_t>(), store, s.flag.get<uint8_t>(), nullptr);
  LH_HIP(hipGetLastError());
  std::vector<uint8_t> flag(n);
  LH_HIP(hipMemcpy(flag.data(), s.flag.get(), n, hipMemcpyDeviceToHost));
  s.K = K_new;
  int32_t m = 0;
  for (int32_t x = 0; x < n; ++x)
    if (flag[x]) {
      if (mismatch) mismatch[m] = x;
      ++m;
    }
  if (n_mismatch) *n_mismatch = m;
  return 0;
}

// seqs[q][0..L) = the bytes of slot slots[q] of the last batch (a padding slot reads as N)
template <class Rows>
int store_rows_read(const std::string& W, SeqStore& s, const Rows& src, int32_t n, int32_t n_out, const int32_t* slots,
                    uint8_t* seqs) {
  if (n_out > 0 && (!slots || !seqs)) return fail(W + ": null array");
  for (int32_t q = 0; q < n_out; ++q)
    if (slots[q] < 0 || slots[q] >= n) return fail(W + ": row outside the last batch");
  if (n_out <= 0) return 0;
  const size_t bytes = (size_t)n_out * src.L;
  if (s.gather_slots.ensure(sizeof(int32_t) * n_out) || s.gather_out.ensure(bytes)) return 1;
  LH_HIP(hipDeviceSynchronize());
  LH_HIP(hipMemcpy(s.gather_slots.get(), slots, sizeof(int32_t) * n_out, hipMemcpyHostToDevice));
  lh::launch_store_gather(src, n_out, s.gather_slots.get<const int32_t>(), s.gather_out.get<uint8_t>(), nullptr);
  LH_HIP(hipGetLastError());
  LH_HIP(hipMemcpy(seqs, s.gather_out.get(), bytes, hipMemcpyDeviceToHost));
  return 0;
}

// *K = the store's count; seqs[count][L] = its sequences first .. first + count - 1
int store_read(const std::string& W, const SeqStore& s, size_t L, int32_t first, int32_t count, int32_t* K, uint8_t* seqs) {
  if (K) *K = s.K;
  if (!seqs || count == 0) return 0;
  if (first < 0 || count < 0 || first > s.K || count > s.K - first) return fail(W + ": ids outside the store");
  LH_HIP(hipDeviceSynchronize());
  LH_HIP(hipMemcpy(seqs, s.store[s.cur].get<uint8_t>() + first * L, count * L, hipMemcpyDeviceToHost));
  return 0;
}

// the rows of the last K6c batch
lh::FlatRows draw_rows(const lh_family* f) {
  return lh::FlatRows{f->collect.n_last, f->host.n_sites, f->collect.seqs.get<const uint8_t>()};
}

}  // namespace

extern "C" {

int lh_eval_draw_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                              const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                              const uint32_t* words, double* loglik, uint64_t* hash, int32_t* states, void* hip_stream) {
  const std::string W = "lh_eval_draw_batch_device";
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, W, b, true)) return rc > 0;
  DeviceGuard guard(f);
  lh::CollectTables t;
  if (collect_tables(f, W, &t)) return 1;
  if (!words || !loglik || !hash) return fail(W + ": null array");
  CollectWs& c = f->collect;
  if (!states) {
    if (c.states.ensure(sizeof(int32_t) * t.states_per_sample * (size_t)n)) return 1;
    states = c.states.get<int32_t>();
  }
  if (lh_eval_sample_batch_device(f, n, T, max_depth, ops, brlen, er, pi, alpha, R, words, loglik, nullptr, states,
                                  hip_stream))
    return 1;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (collect_launch(f, t, n, states, stream)) return 1;
  LH_HIP(hipMemcpyAsync(hash, c.hash.get(), sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, stream));
  return 0;
}

int lh_eval_draw_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                       const double* er, const double* pi, const double* alpha, int32_t R, const uint32_t* words,
                       double* loglik, uint64_t* hash, int32_t* states) {
  const std::string W = "lh_eval_draw_batch";
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, W, host, true)) return rc > 0;
  DeviceGuard guard(f);
  lh::CollectTables t;
  if (collect_tables(f, W, &t)) return 1;
  if (!host.has_arrays() || !words || !loglik || !hash) return fail(W + ": null array");
  std::chrono::steady_clock::time_point st[4];
  if (sample_host_batch(f, host, words, false, false, st)) return 1;
  HostOutputs& out = f->out;
  if (collect_launch(f, t, n, out.states.get<const int32_t>(), nullptr)) return 1;
  return finish_batch(f, W.c_str(), host,
                      {{loglik, out.loglik.get(), sizeof(double) * n},
                       {hash, f->collect.hash.get(), sizeof(uint64_t) * n},
                       {states, out.states.get(), sizeof(int32_t) * f->sampler.states_per_sample * (size_t)n}});
}

int lh_naive_sequences(lh_family* f, int32_t n, const int32_t* states, uint8_t* seqs, uint64_t* hash) {
  const std::string W = "lh_naive_sequences";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  lh::CollectTables t;
  if (collect_tables(f, W, &t)) return 1;
  if (n < 0) return fail(W + ": negative row count");
  if (n == 0) return 0;
  if (!states) return fail(W + ": null array");
  CollectWs& c = f->collect;
  const size_t sb = sizeof(int32_t) * t.states_per_sample * (size_t)n;
  if (c.states.ensure(sb)) return 1;
  LH_HIP(hipDeviceSynchronize());
  LH_HIP(hipMemcpy(c.states.get(), states, sb, hipMemcpyHostToDevice));
  if (collect_launch(f, t, n, c.states.get<const int32_t>(), nullptr)) return 1;
  return copy_back(f, nullptr, {{seqs, c.seqs.get(), (size_t)n * t.L}, {hash, c.hash.get(), sizeof(uint64_t) * n}});
}

int lh_draws_resolve(lh_family* f, int32_t n, const int32_t* cand, int32_t* n_mismatch, int32_t* mismatch_rows) {
  const std::string W = "lh_draws_resolve";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (n != f->collect.n_last) return fail(W + ": n differs from the last batch's row count");
  return store_resolve(W, f->collect.store, draw_rows(f), n, cand, n_mismatch, mismatch_rows);
}

int lh_draws_rows_read(lh_family* f, int32_t n_rows, const int32_t* rows, uint8_t* seqs) {
  const std::string W = "lh_draws_rows_read";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  return store_rows_read(W, f->collect.store, draw_rows(f), f->collect.n_last, n_rows, rows, seqs);
}

int lh_draws_candidates_read(lh_family* f, int32_t* K, uint8_t* seqs) {
  const std::string W = "lh_draws_candidates_read";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  return store_read(W, f->collect.store, f->host.n_sites, 0, f->collect.store.K, K, seqs);
}

int lh_draws_reset(lh_family* f) {
  if (!f) return fail("lh_draws_reset: null family");
  f->collect.store.K = 0;
  f->collect.n_last = -1;
  return 0;
}

int lh_collect_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::collect_timer, ms, n_launches);
}

}  // extern "C"

// ---- K7: the lineage of a seed sequence, and the lineage store (lh_lineage.hip) ----

extern "C" {

int lh_lineage_collect_device(lh_family* f, int32_t n, int32_t T, const uint8_t* anc, const uint8_t* naive,
                              const int32_t* path, int32_t P, uint64_t* nt_hash, uint64_t* aa_hash, void* hip_stream) {
  const std::string W = "lh_lineage_collect_device";
  if (!f) return fail(W + ": null family");
  if (n < 0) return fail(W + ": negative batch size");
  if (f->host.n_seqs < 1) return fail(W + ": family was created without an MSA (forward-only)");
  if (T != f->host.n_seqs + 1 || T < 3) return fail(W + ": n_tips must equal n_seqs + 1 (naive), at least 3");
  if (P < 1 || P > T - 2) return fail(W + ": path length must be in 1 .. n_tips - 2");
  if ((size_t)n * (size_t)(P + 1) > (size_t)INT32_MAX) return fail(W + ": too many lineage slots for one batch");
  DeviceGuard guard(f);
  LineageWs& w = f->lineage;
  w.last.n = -1;
  if (n == 0) return 0;
  if (!anc || !naive || !path || !nt_hash || !aa_hash) return fail(W + ": null array");
  const int bits = lh::debug_options().collect_hash_bits;
  const lh::LineageBatch b{n, T, f->host.n_sites, P, anc, naive, path, bits >= 64 ? ~0ull : ((1ull << bits) - 1)};
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (f->profile && f->lineage_timer.begin(stream)) return 1;
  lh::launch_lineage(b, nt_hash, aa_hash, stream);
  LH_HIP(hipGetLastError());
  if (f->profile && f->lineage_timer.end(stream)) return 1;
  w.last = b;
  return 0;
}

int lh_lineage_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                     const double* er, const double* pi, const double* rates, int32_t R, const uint8_t* naive,
                     uint64_t seed, uint64_t first_sample, const int32_t* path, int32_t P, uint64_t* nt_hash,
                     uint64_t* aa_hash) {
  const std::string W = "lh_lineage_batch";
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, rates, R, true};
  if (int rc = check_batch(f, W, host)) {
    if (rc < 0) f->lineage.last.n = -1;
    return rc > 0;
  }
  DeviceGuard guard(f);
  f->lineage.last.n = -1;
  if (!host.has_arrays() || !naive || !path || !nt_hash || !aa_hash) return fail(W + ": null array");
  if (P < 1 || P > T - 2) return fail(W + ": path length must be in 1 .. n_tips - 2");
  const size_t n_ops = host.n_ops(), L = f->host.n_sites;
  // the whole batch's anc stays on the device for lh_lineage_resolve: no sub-batches here
  const size_t most = std::min<size_t>(((size_t)1 << 30) / std::max<size_t>(n_ops * L, 1), (size_t)INT32_MAX / (P + 1));
  if ((size_t)n > most)
    return fail(W + ": batch too large to keep its sampled states on the device: at most " + std::to_string(most) +
                " samples per call for this family");
  if (!valid_schedules(host)) return fail(W + ": malformed schedule op (use lh_schedule_tree)");
  if (valid_naive(W, naive, (size_t)n * L) || valid_paths(W, path, P, host)) return 1;
  HostOutputs& out = f->out;
  LineageWs& w = f->lineage;
  const size_t hb = sizeof(uint64_t) * n * (P + 1);
  TreeBatch dev;
  if (out.anc.ensure(n_ops * L * n) || out.rate_choice.ensure(L * n) || w.nt_hash.ensure(hb) || w.aa_hash.ensure(hb) ||
      stage_batch(f, host, {{naive, L * n, &w.naive}, {path, sizeof(int32_t) * P * n, &w.path}}, &dev))
    return 1;
  if (lh_asr_batch_device(f, n, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, w.naive.get<const uint8_t>(), seed, first_sample,
                          out.anc.get<uint8_t>(), out.rate_choice.get<uint8_t>(), nullptr))
    return 1;
  if (lh_lineage_collect_device(f, n, T, out.anc.get<const uint8_t>(), w.naive.get<const uint8_t>(),
                                w.path.get<const int32_t>(), P, w.nt_hash.get<uint64_t>(), w.aa_hash.get<uint64_t>(),
                                nullptr))
    return 1;
  if (copy_back(f, "lh_lineage_batch", {{nt_hash, w.nt_hash.get(), hb}, {aa_hash, w.aa_hash.get(), hb}})) {
    w.last.n = -1;
    return 1;
  }
  return 0;
}

int lh_lineage_resolve(lh_family* f, int32_t n_slots, const int32_t* ids, int32_t* n_mismatch, int32_t* mismatch_slots) {
  const std::string W = "lh_lineage_resolve";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  const lh::LineageBatch& b = f->lineage.last;
  if (b.n < 0) return fail(W + ": no lineage batch on the handle");
  if ((size_t)n_slots != lh::n_slots(b))
    return fail(W + ": n_slots differs from the last batch's rows x draws x (path length + 1)");
  return store_resolve(W, f->lineage.store, b, n_slots, ids, n_mismatch, mismatch_slots);
}

int lh_lineage_rows_read(lh_family* f, int32_t n_slots, const int32_t* slots, uint8_t* seqs) {
  const std::string W = "lh_lineage_rows_read";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  const lh::LineageBatch& b = f->lineage.last;
  if (b.n < 0) return fail(W + ": no lineage batch on the handle");
  return store_rows_read(W, f->lineage.store, b, (int32_t)lh::n_slots(b), n_slots, slots, seqs);
}

int lh_lineage_store_read(lh_family* f, int32_t first, int32_t count, int32_t* K, uint8_t* seqs) {
  const std::string W = "lh_lineage_store_read";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  return store_read(W, f->lineage.store, f->host.n_sites, first, count, K, seqs);
}

int lh_lineage_reset(lh_family* f) {
  if (!f) return fail("lh_lineage_reset: null family");
  f->lineage.store.K = 0;
  f->lineage.last.n = -1;
  return 0;
}

int lh_lineage_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::lineage_timer, ms, n_launches);
}

}  // extern "C"

// ---- the chain: evaluation, naive draw, ancestral draws and lineage hashes of a batch in one pass ----

namespace {

// The shape checks lh_eval_lineage_batch[_device] share (everything that needs no array): lh_lineage_batch's and
// lh_eval_draw_batch's refusals, the draws, and the bound on the sampled states that stay on the device.
int lineage_eval_check(lh_family* f, const std::string& W, const TreeBatch& b, uint64_t first_sample, int32_t D, int32_t P,
                       lh::CollectTables* t) {
  const int n = b.n, T = b.T, R = b.R;
  if (int rc = check_batch(f, W, b, true)) {
    if (rc < 0) f->lineage.last.n = -1;
    return rc;
  }
  f->lineage.last.n = -1;
  if (D < 1 || D > 64) return fail(W + ": draws must be in 1 .. 64");
  if (P < 1 || P > T - 2) return fail(W + ": path length must be in 1 .. n_tips - 2");
  if (D > 1 && (first_sample > ((uint64_t)1 << 32) || first_sample + (uint64_t)n > ((uint64_t)1 << 32)))
    return fail(W + ": with more than one draw per row the sample numbers first_sample .. first_sample + n - 1 must lie "
                    "below 2^32 (the draw number takes the upper half)");
  const size_t n_ops = b.n_ops(), L = f->host.n_sites;
  // the whole batch's anc stays on the device for lh_lineage_resolve: n * draws samples of it
  const size_t most = std::min<size_t>(((size_t)1 << 30) / std::max<size_t>(n_ops * L, 1), (size_t)INT32_MAX / (P + 1)) / (size_t)D;
  if ((size_t)n > most)
    return fail(W + ": batch too large to keep its sampled states on the device: at most " + std::to_string(most) +
                " samples per call for this family with " + std::to_string(D) + " draws each");
  DeviceGuard guard(f);
  if (collect_tables(f, W, t)) return 1;
  if (lh::asr_lds_bytes(T, f->host.n_sites, R, f->host.n_prune) > 160 * 1024)
    return fail(W + ": tree / alignment too large for the sampling kernel's LDS tables");
  return 0;
}

}  // namespace

extern "C" {

int lh_eval_lineage_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                 const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                 const uint32_t* words, uint64_t seed, uint64_t first_sample, int32_t D,
                                 const int32_t* path, int32_t P, const lh_lineage_eval_outputs* outs, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  const std::string W = "lh_eval_lineage_batch_device";
  lh::CollectTables t;
  if (int rc = lineage_eval_check(f, W, b, first_sample, D, P, &t)) return rc > 0;
  DeviceGuard guard(f);
  if (!b.has_arrays() || !words || !path || !outs || !outs->loglik || !outs->nt_hash || !outs->aa_hash)
    return fail(W + ": null array");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const size_t n_ops = b.n_ops(), L = f->host.n_sites, FS = f->host.forward_size;
  const size_t NS = t.states_per_sample, NW = f->sampler.words_per_sample, S = (size_t)P + 1;
  // launch groups: the smaller of the evaluation's limit and the sampling kernel's (whose CLV area and grid count
  // virtual samples); one K1 launch, unmixed, serves K2 and K3 of the group, so its planes outlive K2
  const size_t clv_per_sample = sizeof(double) * n_ops * 4 * lh::asr_slots((int)L, R);
  const size_t asr_limit = std::max<size_t>(1, asr_group(f, T, R, clv_per_sample) / (size_t)D);
  const int chunk = (int)std::min<size_t>((size_t)n, std::min(eval_group(f, T, R), asr_limit));
  if (ensure_workspace(f, chunk, R, T)) return 1;
  AsrWs& aw = f->asr;
  CollectWs& c = f->collect;
  HostOutputs& out = f->out;
  if (aw.clv.ensure(clv_per_sample * chunk * D) || aw.desc.ensure(lh::asr_desc_bytes(T) * chunk) ||
      out.anc.ensure(n_ops * L * n * D) || out.rate_choice.ensure(L * (size_t)n * D) ||
      f->forward_dev.ensure(sizeof(double) * FS * n) || c.seqs.ensure((size_t)n * L) || c.hash.ensure(sizeof(uint64_t) * n) ||
      (!outs->states && c.states.ensure(sizeof(int32_t) * NS * n)) || (!outs->rates && aw.rates.ensure(sizeof(double) * R * n)))
    return 1;
  Workspace& w = f->ws;
  double *eig = w.eig.get<double>(), *site_lik = w.site_lik.get<double>(), *fwd = f->forward_dev.get<double>();
  int32_t* site_scal = w.site_scal.get<int32_t>();
  double* rates = outs->rates ? outs->rates : aw.rates.get<double>();
  int32_t* states = outs->states ? outs->states : c.states.get<int32_t>();
  uint8_t *naive = c.seqs.get<uint8_t>(), *anc = out.anc.get<uint8_t>(), *choice = out.rate_choice.get<uint8_t>();
  uint64_t* naive_hash = c.hash.get<uint64_t>();
  const int bits = lh::debug_options().collect_hash_bits;
  const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
  const lh_eval_outputs fwd_outs{nullptr, nullptr, fwd, nullptr};
  c.n_last = -1;
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const TreeBatch g = b.slice(off, m);
    double* r_m = rates + (size_t)off * R;
    if (f->profile && f->chain_timer.begin(stream)) return 1;
    lh::launch_model_setup(m, R, g.er, g.pi, g.model, r_m, eig, stream);
    if (f->profile && f->chain_timer.mark(1, stream)) return 1;
    int planes = 0;
    if (prune_group(f, W, g, r_m, false, stream, &planes)) return 1;
    if (f->profile && f->chain_timer.mark(2, stream)) return 1;
    if (run_forward(f, m, planes, site_lik, site_scal, g.pi, nullptr, nullptr, outs->loglik + off, &fwd_outs, off, stream)) return 1;
    lh::launch_sample(f->sampler, f->sampler_dev, m, fwd + (size_t)off * FS, FS, words + (size_t)off * NW, (int)NW,
                      states + (size_t)off * NS, stream);
    lh::launch_collect(t, m, states + (size_t)off * NS, naive + (size_t)off * L, naive_hash + off, stream);
    LH_HIP(hipGetLastError());
    if (f->profile && f->chain_timer.mark(3, stream)) return 1;
    uint8_t* anc_m = anc + (size_t)off * D * n_ops * L;
    if (lh::launch_asr(f->host, m, R, T, g.ops, g.brlen, r_m, eig, g.pi, site_lik, site_scal, naive + (size_t)off * L, seed,
                       first_sample + (uint64_t)off, aw.clv.get<double>(), aw.desc.get(), anc_m, choice + (size_t)off * D * L,
                       w.prune.hdr, stream, D))
      return fail(W + ": launch failed");
    LH_HIP(hipGetLastError());
    if (f->profile && f->chain_timer.mark(4, stream)) return 1;
    const lh::LineageBatch lg{m, T, (int32_t)L, P, anc_m, naive + (size_t)off * L, path + (size_t)off * P, mask, D};
    lh::launch_lineage(lg, outs->nt_hash + (size_t)off * D * S, outs->aa_hash + (size_t)off * D * S, stream);
    LH_HIP(hipGetLastError());
    if (f->profile && f->chain_timer.end(stream)) return 1;
  }
  if (outs->naive) LH_HIP(hipMemcpyAsync(outs->naive, naive, (size_t)n * L, hipMemcpyDeviceToDevice, stream));
  if (outs->naive_hash)
    LH_HIP(hipMemcpyAsync(outs->naive_hash, naive_hash, sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, stream));
  c.n_last = n;
  f->lineage.last = lh::LineageBatch{n, T, (int32_t)L, P, anc, naive, path, mask, D};
  return 0;
}

int lh_eval_lineage_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                          const double* er, const double* pi, const double* alpha, int32_t R, const uint32_t* words,
                          uint64_t seed, uint64_t first_sample, int32_t D, const int32_t* path, int32_t P,
                          const lh_lineage_eval_outputs* outs) {
  const std::string W = "lh_eval_lineage_batch";
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  lh::CollectTables t;
  if (int rc = lineage_eval_check(f, W, host, first_sample, D, P, &t)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays() || !words || !path || !outs || !outs->loglik || !outs->nt_hash || !outs->aa_hash)
    return fail(W + ": null array");
  const size_t L = f->host.n_sites, NS = t.states_per_sample, NW = f->sampler.words_per_sample;
  if (valid_paths(W, path, P, host)) return 1;
  HostOutputs& out = f->out;
  LineageWs& lw = f->lineage;
  const size_t hb = sizeof(uint64_t) * n * D * (P + 1);
  lh_lineage_eval_outputs d{};
  TreeBatch dev;
  if (out.loglik.ensure(sizeof(double) * n) || out_buf(outs->rates, out.rates, sizeof(double) * R * n, &d.rates) ||
      out_buf(outs->states, out.states, sizeof(int32_t) * NS * n, &d.states) || lw.nt_hash.ensure(hb) || lw.aa_hash.ensure(hb) ||
      stage_batch(f, host, {{words, sizeof(uint32_t) * NW * n, &f->in.words}, {path, sizeof(int32_t) * P * n, &lw.path}}, &dev))
    return 1;
  d.loglik = out.loglik.get<double>();
  d.nt_hash = lw.nt_hash.get<uint64_t>();
  d.aa_hash = lw.aa_hash.get<uint64_t>();
  if (lh_eval_lineage_batch_device(f, n, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, f->in.words.get<const uint32_t>(), seed, first_sample, D,
                                   lw.path.get<const int32_t>(), P, &d, nullptr))
    return 1;
  // (the schedules are checked on the host beside the device, as in lh_eval_draw_batch)
  const int rc = finish_batch(f, W.c_str(), host,
                              {{outs->loglik, d.loglik, sizeof(double) * n},
                               {outs->rates, d.rates, sizeof(double) * R * n},
                               {outs->states, d.states, sizeof(int32_t) * NS * n},
                               {outs->naive, f->collect.seqs.get(), (size_t)n * L},
                               {outs->naive_hash, f->collect.hash.get(), sizeof(uint64_t) * n},
                               {outs->nt_hash, d.nt_hash, hb},
                               {outs->aa_hash, d.aa_hash, hb}});
  if (rc) {
    lw.last.n = -1;
    f->collect.n_last = -1;
  }
  return rc;
}

int lh_lineage_eval_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::chain_timer, ms, n_launches);
}

}  // extern "C"

// ---- K8: the most probable state path, candidate paths (lh_viterbi.hip) ----

namespace {

// K8 for the m samples K2a's hand-off buffers hold (run_forward has just been enqueued on `stream` for them)
int viterbi_launch(lh_family* f, int m, const double* loglik, int32_t* states, double* log_path, hipStream_t stream) {
  ForwardWs& w = f->fws;
  if (f->vit.bp.ensure(lh::viterbi_bp_bytes(f->host) * (size_t)m)) return 1;
  lh::launch_viterbi(f->host, f->sampler_dev, m, w.gem.get<const double>(), w.gcnt.get<const int32_t>(),
                     w.jem.get<const double>(), w.jrs.get<const int32_t>(), loglik, f->vit.bp.get<uint8_t>(), states, log_path,
                     f->extended, stream);
  LH_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int lh_eval_viterbi_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                 const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                 const lh_viterbi_outputs* outs, void* hip_stream) {
  const TreeBatch b{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  const std::string W = "lh_eval_viterbi_batch_device";
  if (int rc = check_batch(f, W, b, true)) return rc > 0;
  DeviceGuard guard(f);
  if (lh::viterbi_lds_bytes(f->host) > 160 * 1024) return fail(W + ": the junction tables do not fit K8's LDS");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const lh_viterbi_outputs none{};
  const lh_viterbi_outputs& o = outs ? *outs : none;
  ViterbiWs& vw = f->vit;
  const size_t S = f->sampler.states_per_sample;
  double *ll = o.loglik, *lp = o.log_path;
  WeightReduce wr;
  int32_t* states = o.states;
  if (own(ll, vw.loglik, sizeof(double) * n) || own(lp, vw.log_path, sizeof(double) * n) ||
      (!states && vw.states.ensure(sizeof(int32_t) * S * n)) ||
      (o.weight_stats && wr.prepare(n, vw.weights, vw.stats, o.weight_stats)) ||
      vw.bp.ensure(lh::viterbi_bp_bytes(f->host) * (size_t)std::min(n, kChunk)))
    return 1;
  if (!states) states = vw.states.get<int32_t>();
  const std::function<int(int, int)> after = [&](int off, int m) {
    if (f->profile && f->vit_timer.begin(stream)) return 1;
    if (viterbi_launch(f, m, ll + off, states + (size_t)off * S, lp + off, stream)) return 1;
    if (f->profile && f->vit_timer.end(stream)) return 1;
    return 0;
  };
  if (eval_device(f, b, ll, nullptr, hip_stream, lh::LogEmRequest{}, &after)) return 1;
  if (o.weight_stats) wr.launch(n, ll, o.log_offset, stream);
  LH_HIP(hipGetLastError());
  return 0;
}

int lh_eval_viterbi_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                          const double* er, const double* pi, const double* alpha, int32_t R,
                          const lh_viterbi_outputs* outs) {
  const std::string W = "lh_eval_viterbi_batch";
  const TreeBatch host{n, T, max_depth, ops, brlen, er, pi, alpha, R};
  if (int rc = check_batch(f, W, host, true)) return rc > 0;
  DeviceGuard guard(f);
  if (!host.has_arrays()) return fail(W + ": null array");
  const lh_viterbi_outputs none{};
  const lh_viterbi_outputs& o = outs ? *outs : none;
  if (!o.loglik && !o.states && !o.log_path && !o.weight_stats) return 0;  // nothing asked for
  const size_t S = f->sampler.states_per_sample;
  HostOutputs& out = f->out;
  lh_viterbi_outputs d{};
  TreeBatch dev;
  if (out.loglik.ensure(sizeof(double) * n) || out.states.ensure(sizeof(int32_t) * S * n) ||
      out.log_path.ensure(sizeof(double) * n) ||
      out_buf(o.weight_stats, out.weight_stats, sizeof(double) * 3, &d.weight_stats) ||
      stage_batch(f, host, {{o.log_offset, sizeof(double) * n, &f->in.log_offset}}, &dev))
    return 1;
  d.log_offset = o.log_offset ? f->in.log_offset.get<const double>() : nullptr;
  d.loglik = out.loglik.get<double>();
  d.states = out.states.get<int32_t>();
  d.log_path = out.log_path.get<double>();
  if (lh_eval_viterbi_batch_device(f, n, T, max_depth, dev.ops, dev.brlen, dev.er, dev.pi, dev.model, R, &d, nullptr)) return 1;
  return finish_batch(f, W.c_str(), host,
                      {{o.loglik, d.loglik, sizeof(double) * n},
                       {o.states, d.states, sizeof(int32_t) * S * n},
                       {o.log_path, d.log_path, sizeof(double) * n},
                       {o.weight_stats, d.weight_stats, sizeof(double) * 3}});
}

int lh_viterbi_forward_batch(lh_family* f, int32_t n, const double* em, double* log_path, int32_t* states) {
  const std::string W = "lh_viterbi_forward_batch";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (!f->have_sampler) return fail(W + ": lh_family_set_sampler has not been called");
  if (n <= 0) return n == 0 ? 0 : fail(W + ": negative batch size");
  if (!em) return fail(W + ": null array");
  if (lh::viterbi_lds_bytes(f->host) > 160 * 1024) return fail(W + ": the junction tables do not fit K8's LDS");
  const size_t C = f->host.n_xmsa, S = f->sampler.states_per_sample;
  HostOutputs& out = f->out;
  if (out.loglik.ensure(sizeof(double) * n) || out.states.ensure(sizeof(int32_t) * S * n) ||
      out.log_path.ensure(sizeof(double) * n) || stage_inputs(f, {{em, sizeof(double) * C * n, &f->in.em}}))
    return 1;
  if (run_forward(f, n, 1, nullptr, nullptr, nullptr, f->in.em.get<const double>(), nullptr, out.loglik.get<double>(), nullptr,
                  0, nullptr))
    return 1;
  if (viterbi_launch(f, n, out.loglik.get<const double>(), out.states.get<int32_t>(), out.log_path.get<double>(), nullptr))
    return 1;
  return copy_back(f, nullptr,
                   {{log_path, out.log_path.get(), sizeof(double) * n}, {states, out.states.get(), sizeof(int32_t) * S * n}});
}

int lh_family_set_candidate_paths(lh_family* f, int32_t K, const int32_t* states, double* log_prior) {
  const std::string W = "lh_family_set_candidate_paths";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  lh::CollectTables t;
  if (collect_tables(f, W, &t)) return 1;
  if (K < 1 || K > 65536) return fail(W + ": K must be 1 .. 65536 paths");
  if (!states) return fail(W + ": null array");
  ViterbiWs& vw = f->vit;
  CandidateWs& cw = f->cand;
  const size_t S = f->sampler.states_per_sample;
  const int32_t none = INT32_MAX;
  cw.tab.K = 0;  // a call that fails leaves the handle without candidates
  // the priors first: they also decide whether every vector is a path (K6c is given nothing else)
  if (vw.log_path.ensure(sizeof(double) * K) || vw.first_bad.ensure(sizeof(int32_t)) ||
      stage_inputs(f, {{states, sizeof(int32_t) * S * K, &vw.paths}, {&none, sizeof(none), &vw.first_bad}}))
    return 1;
  lh::launch_path_prior(f->host, f->sampler_dev, K, vw.paths.get<const int32_t>(), vw.log_path.get<double>(),
                        vw.first_bad.get<int32_t>(), nullptr);
  LH_HIP(hipGetLastError());
  int32_t bad = none;
  LH_HIP(hipMemcpy(&bad, vw.first_bad.get(), sizeof(bad), hipMemcpyDeviceToHost));
  if (bad != none)
    return fail(W + ": vector " + std::to_string(bad) +
                " is not a path of the model (a state index out of range or a transition of probability 0)");
  // their naive sequences, registered as lh_family_set_candidates registers sequences; then the paths' priors replace the
  // sequences' in the tables
  std::vector<uint8_t> seqs((size_t)K * t.L);
  if (collect_launch(f, t, K, vw.paths.get<const int32_t>(), nullptr)) return 1;
  if (copy_back(f, nullptr, {{seqs.data(), f->collect.seqs.get(), seqs.size()}})) return 1;
  if (lh_family_set_candidates(f, K, seqs.data(), nullptr)) return 1;
  LH_HIP(hipMemcpy(cw.prior.get(), vw.log_path.get(), sizeof(double) * K, hipMemcpyDeviceToDevice));
  return copy_back(f, nullptr, {{log_prior, cw.prior.get(), sizeof(double) * K}});
}

int lh_viterbi_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::vit_timer, ms, n_launches);
}

}  // extern "C"

// ---- K9 and K10: a table per row, the gene posteriors and the weighted sums of both, behind one evaluation ----

namespace {

// lh_codon_outputs and lh_events_outputs, member for member (`table`: the windows or the events)
struct TableOuts {
  const double* log_offset;
  double *loglik, *table, *genes, *weighted_table, *weighted_genes, *weight_stats;
};

// The _device form behind its argument checks: rows of NT table entries and NG genes.  launch(fwd, loglik, table, genes)
// enqueues the kernels behind the evaluation and begins the timer's group when the handle profiles; the reduction joins
// the group's last stage.  The caller has taken the kernel's own scratch.
template <int Stages, class Launch>
int table_batch_device(lh_family* f, const TreeBatch& b, TableWs& ws, size_t NT, size_t NG, const TableOuts& o,
                       void* hip_stream, KernelTimer<Stages> lh_family::*timer, Launch&& launch) {
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const int n = b.n;
  double *ll = o.loglik, *tbl = o.table, *gen = o.genes, *pt = nullptr, *pg = nullptr;
  WeightReduce wr;
  const bool reduce = o.weighted_table || o.weighted_genes || o.weight_stats;
  const size_t slabs = lh::posterior_slabs(n);
  // the forward arrays stay in the handle's buffer: the kernels only read them
  if (f->forward_dev.ensure(sizeof(double) * f->host.forward_size * n) || own(ll, ws.loglik, sizeof(double) * n) ||
      own(tbl, ws.table, sizeof(double) * NT * n) || own(gen, ws.genes, sizeof(double) * NG * n) ||
      (reduce && (wr.prepare(n, ws.weights, ws.stats, o.weight_stats) ||
                  (o.weighted_table && own(pt, ws.partial_t, sizeof(double) * NT * slabs)) ||
                  (o.weighted_genes && own(pg, ws.partial_g, sizeof(double) * NG * slabs)))))
    return 1;
  double* fwd = f->forward_dev.get<double>();
  lh_eval_outputs eo{nullptr, nullptr, fwd, nullptr};
  if (eval_device(f, b, ll, &eo, hip_stream)) return 1;
  if (launch(fwd, ll, tbl, gen, stream)) return 1;
  if (reduce) {
    wr.launch(n, ll, o.log_offset, stream);
    if (o.weighted_table) lh::launch_weighted_slabs(n, NT, tbl, wr.w, pt, o.weighted_table, stream);
    if (o.weighted_genes) lh::launch_weighted_slabs(n, NG, gen, wr.w, pg, o.weighted_genes, stream);
  }
  if (f->profile && (f->*timer).end(stream)) return 1;
  LH_HIP(hipGetLastError());
  return 0;
}

// The host-pointer form W behind its argument checks: `device` is its _device form, run on the handle's device copies.
using TableDevice = int(lh_family*, const std::string&, const TreeBatch&, const TableOuts&, void*, bool);
int table_batch(lh_family* f, const std::string& W, const TreeBatch& host, TableWs& ws, size_t NT, size_t NG,
                const TableOuts& o, TableDevice* device) {
  if (!host.has_arrays()) return fail(W + ": null array");
  if (!o.loglik && !o.table && !o.genes && !o.weighted_table && !o.weighted_genes && !o.weight_stats) return 0;
  const int n = host.n;
  HostOutputs& out = f->out;
  TableOuts d{};
  TreeBatch dev;
  if (out.loglik.ensure(sizeof(double) * n) || out_buf(o.table, ws.table, sizeof(double) * NT * n, &d.table) ||
      out_buf(o.genes, ws.genes, sizeof(double) * NG * n, &d.genes) ||
      out_buf(o.weighted_table, ws.out_tsum, sizeof(double) * NT, &d.weighted_table) ||
      out_buf(o.weighted_genes, ws.out_gsum, sizeof(double) * NG, &d.weighted_genes) ||
      out_buf(o.weight_stats, out.weight_stats, sizeof(double) * 3, &d.weight_stats) ||
      stage_batch(f, host, {{o.log_offset, sizeof(double) * n, &f->in.log_offset}}, &dev))
    return 1;
  d.log_offset = o.log_offset ? f->in.log_offset.get<const double>() : nullptr;
  d.loglik = out.loglik.get<double>();
  if (device(f, W + "_device", dev, d, nullptr, false)) return 1;
  return finish_batch(f, W.c_str(), host,
                      {{o.loglik, d.loglik, sizeof(double) * n},
                       {o.table, d.table, sizeof(double) * NT * n},
                       {o.genes, d.genes, sizeof(double) * NG * n},
                       {o.weighted_table, d.weighted_table, sizeof(double) * NT},
                       {o.weighted_genes, d.weighted_genes, sizeof(double) * NG},
                       {o.weight_stats, d.weight_stats, sizeof(double) * 3}});
}

TableOuts table_outs(const lh_codon_outputs* o) {
  if (!o) return {};
  return {o->log_offset, o->loglik, o->windows, o->genes, o->weighted_windows, o->weighted_genes, o->weight_stats};
}
TableOuts table_outs(const lh_events_outputs* o) {
  if (!o) return {};
  return {o->log_offset, o->loglik, o->events, o->genes, o->weighted_events, o->weighted_genes, o->weight_stats};
}

// lh_eval_codons_batch_device; host (b's arrays are the host's): lh_eval_codons_batch, which comes back here once, staged
int codons_batch(lh_family* f, const std::string& W, const TreeBatch& b, const TableOuts& o, void* hip_stream, bool host) {
  if (f && f->have_sampler && f->codon.frame < 0) return fail(W + ": lh_family_set_codons has not been called");
  if (int rc = check_batch(f, W, b, true)) return rc > 0;
  DeviceGuard guard(f);
  CodonWs& cw = f->codon;
  const lh::CodonTables& tab = cw.tab;
  const size_t NW = (size_t)tab.n_window * 125, NG = tab.n_genes;
  if (host) return table_batch(f, W, b, cw, NW, NG, o, codons_batch);
  if (cw.scratch.ensure(sizeof(double) * 4 * (size_t)tab.max_vec * lh::codon_slots(b.n))) return 1;
  return table_batch_device(f, b, cw, NW, NG, o, hip_stream, &lh_family::codon_timer,
                            [&](const double* fwd, const double* ll, double* win, double* gen, hipStream_t stream) {
                              if (f->profile && f->codon_timer.begin(stream)) return 1;
                              lh::launch_codons(f->sampler_dev, tab, b.n, fwd, f->host.forward_size, ll,
                                                cw.scratch.get<double>(), win, gen, stream);
                              return 0;
                            });
}

}  // namespace

extern "C" {

// ---- K9: exact posterior distributions of the naive sequence's codons (lh_codon.hip) ----

int lh_family_set_codons(lh_family* f, int32_t frame) {
  const std::string W = "lh_family_set_codons";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (frame < 0 || frame > 2) return fail(W + ": frame must be 0, 1 or 2");
  if (!f->have_sampler) return fail(W + ": lh_family_set_sampler has not been called");
  const CodonSource& cs = f->codon_src;
  if (!cs.have) return fail(W + ": family was created without an MSA (forward-only)");
  const lh::DevFamily& h = f->host;
  const bool has_d = h.has_d != 0;
  const int L = h.n_sites, nV = h.vgerm.n_genes, nD = has_d ? h.dgerm.n_genes : 0, nJ = h.jgerm.n_genes;
  const int Wvd = h.vd.n_rows, Wdj = has_d ? h.dj.n_rows : 0;
  // the alignment site of every junction row (the NTI states have a column on each)
  auto row_sites = [&](const CodonSourceJunction& j, int rows, int nR, int* site0) {
    for (int i = 0; i < rows; ++i) {
      const int32_t c = j.nti_xmsa[(size_t)i * nR * 4];
      if (c < 0) return fail(W + ": a junction row without an NTI column");
      if (i == 0) *site0 = cs.site[c];
      else if (cs.site[c] != *site0 + i) return fail(W + ": the rows of a junction are not on consecutive sites");
    }
    return *site0 < 0 || *site0 + rows > L ? fail(W + ": junction rows outside the alignment") : 0;
  };
  int vs0 = 0, ds0 = 0;
  if (row_sites(cs.vd, Wvd, h.vd.n_right, &vs0)) return 1;
  if (has_d) {
    if (row_sites(cs.dj, Wdj, h.dj.n_right, &ds0)) return 1;
    if (ds0 < vs0 + Wvd) return fail(W + ": the junctions overlap");
    if (ds0 == vs0 + Wvd)
      return fail(W + ": the D region has no alignment site of its own between the two junctions (d_l[1] == d_r[0]): a codon "
                      "would span more than three chain positions");
  }
  // chain positions: V | V-D rows | D | D-J rows | J
  const int n_pos = has_d ? Wvd + Wdj + 3 : Wvd + 2;
  const int q_d = Wvd + 1, q_j = n_pos - 1;
  std::vector<int32_t> pos(std::max(L, 1));
  for (int s = 0; s < L; ++s) {
    if (s < vs0) pos[s] = 0;
    else if (s < vs0 + Wvd) pos[s] = 1 + (s - vs0);
    else if (!has_d) pos[s] = q_j;
    else if (s < ds0) pos[s] = q_d;
    else if (s < ds0 + Wdj) pos[s] = q_d + 1 + (s - ds0);
    else pos[s] = q_j;
  }
  // the base every gene of a region writes on every site (N where it writes none)
  auto gene_bases = [&](const CodonSegments& g, int n_genes, int q, std::vector<uint8_t>* gb) {
    gb->assign((size_t)n_genes * std::max(L, 1), 4);
    for (int k = 0; k < n_genes; ++k)
      for (int x = g.offsets[k]; x < g.offsets[k + 1]; ++x) {
        const int s = cs.site[g.inds[x]];
        if (pos[s] != q) return fail(W + ": a germline gene writes a site outside its region");
        (*gb)[(size_t)k * L + s] = cs.base[g.inds[x]];
      }
    return 0;
  };
  std::vector<uint8_t> gb_v, gb_d, gb_j;
  if (gene_bases(cs.v, nV, 0, &gb_v) || (has_d && gene_bases(cs.d, nD, q_d, &gb_d)) || gene_bases(cs.j, nJ, q_j, &gb_j))
    return 1;
  // the code pool: first the base every compact entry of every junction row writes
  std::vector<uint8_t> codes;
  auto row_codes = [&](const CodonSourceJunction& j, int rows, int nL, int nR, std::vector<int32_t>* off) {
    for (int i = 0; i < rows; ++i) {
      off->push_back((int32_t)codes.size());
      for (int l = 0; l < nL; ++l) {
        const int32_t c = j.left_xmsa[(size_t)i * nL + l];
        codes.push_back(c >= 0 ? cs.base[c] : 4);
      }
      for (int r = 0; r < nR; ++r)
        for (int a = 0; a < 4; ++a) codes.push_back((uint8_t)a);
      for (int r = 0; r < nR; ++r) {
        const int32_t c = j.right_xmsa[(size_t)i * nR + r];
        codes.push_back(c >= 0 ? cs.base[c] : 4);
      }
    }
  };
  std::vector<int32_t> off_vd, off_dj;
  row_codes(cs.vd, Wvd, h.vd.n_left, h.vd.n_right, &off_vd);
  if (has_d) row_codes(cs.dj, Wdj, h.dj.n_left, h.dj.n_right, &off_dj);
  auto is_row = [&](int q) { return (q >= 1 && q <= Wvd) || (has_d && q > q_d && q < q_j); };
  const int n_codons = L >= frame ? (L - frame) / 3 : 0;
  std::vector<lh::CodonWindow> wins;
  std::vector<int32_t> window_codon;
  static const int kPow5[3] = {1, 5, 25};
  for (int c = 0; c < n_codons; ++c) {
    const int s0 = frame + 3 * c;
    if (!is_row(pos[s0]) && !is_row(pos[s0 + 1]) && !is_row(pos[s0 + 2])) continue;
    lh::CodonWindow w{};
    for (int o = 0; o < 3;) {
      const int q = pos[s0 + o];
      int o_last = o;
      while (o_last + 1 < 3 && pos[s0 + o_last + 1] == q) ++o_last;
      const int k = o_last - o + 1, slot = w.npos;
      if (slot >= 3 || k > 2 || (slot > 0 && q != w.top + 1)) return fail(W + ": internal error (codon window)");
      w.top = q;
      w.mult[slot] = kPow5[2 - o_last];
      w.ncodes[slot] = kPow5[k];
      if (is_row(q)) {
        w.code_off[slot] = q <= Wvd ? off_vd[q - 1] : off_dj[q - q_d - 1];
      } else {
        const std::vector<uint8_t>& gb = q == 0 ? gb_v : q == q_j ? gb_j : gb_d;
        const int ng = q == 0 ? nV : q == q_j ? nJ : nD;
        w.code_off[slot] = (int32_t)codes.size();
        for (int g = 0; g < ng; ++g) {
          const uint8_t* b = gb.data() + (size_t)g * L + s0;
          codes.push_back(k == 1 ? b[o] : (uint8_t)(5 * b[o] + b[o + 1]));
        }
      }
      ++w.npos;
      o = o_last + 1;
    }
    if (w.npos < 2) return fail(W + ": internal error (codon window of one position)");
    w.out = (int32_t)window_codon.size();
    window_codon.push_back(c);
    wins.push_back(w);
  }
  std::reverse(wins.begin(), wins.end());  // by top, descending: the order the backward recursion meets them
  CodonWs& cw = f->codon;
  cw.frame = -1;
  if (cw.win.ensure(sizeof(lh::CodonWindow) * wins.size()) || cw.codes.ensure(codes.size())) return 1;
  LH_HIP(hipDeviceSynchronize());  // queued work may still read the old tables
  if (!wins.empty())
    LH_HIP(hipMemcpy(cw.win.get(), wins.data(), sizeof(lh::CodonWindow) * wins.size(), hipMemcpyHostToDevice));
  if (!codes.empty()) LH_HIP(hipMemcpy(cw.codes.get(), codes.data(), codes.size(), hipMemcpyHostToDevice));
  cw.tab = lh::CodonTables{};
  cw.tab.n_window = (int32_t)wins.size();
  cw.tab.n_genes = nV + nD + nJ;
  cw.tab.n_pos = n_pos;
  cw.tab.max_vec = std::max({nV, nD, nJ, h.vd.n_left + 5 * h.vd.n_right, has_d ? h.dj.n_left + 5 * h.dj.n_right : 0});
  cw.tab.win = cw.win.get<const lh::CodonWindow>();
  cw.tab.codes = cw.codes.get<const uint8_t>();
  cw.n_codons = n_codons;
  cw.window_codon = window_codon;
  cw.site_pos = pos;
  cw.q_d = q_d;
  cw.q_j = q_j;
  cw.gene_base[0] = gb_v;
  cw.gene_base[1] = gb_d;
  cw.gene_base[2] = gb_j;
  f->node_codons.have = false;  // K14 builds its tables again
  cw.frame = frame;
  return 0;
}

int lh_codon_layout(const lh_family* f, int32_t* n_codons, int32_t* n_window, int32_t* window_codon, int32_t* n_genes) {
  if (!f) return fail("lh_codon_layout: null family");
  const CodonWs& cw = f->codon;
  if (cw.frame < 0) return fail("lh_codon_layout: lh_family_set_codons has not been called");
  if (n_codons) *n_codons = cw.n_codons;
  if (n_window) *n_window = cw.tab.n_window;
  if (window_codon) std::copy(cw.window_codon.begin(), cw.window_codon.end(), window_codon);
  if (n_genes) *n_genes = cw.tab.n_genes;
  return 0;
}

int lh_eval_codons_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                const lh_codon_outputs* outs, void* hip_stream) {
  return codons_batch(f, "lh_eval_codons_batch_device", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, table_outs(outs),
                      hip_stream, false);
}

int lh_eval_codons_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                         const double* er, const double* pi, const double* alpha, int32_t R, const lh_codon_outputs* outs) {
  return codons_batch(f, "lh_eval_codons_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, table_outs(outs), nullptr,
                      true);
}

int lh_codon_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::codon_timer, ms, n_launches);
}

}  // extern "C"

// ---- K10: exact posteriors of the recombination events (lh_events.hip) ----

namespace {

struct EventsLayout {
  int32_t n_junctions = 0, n_genes = 0;
  int32_t rows[2] = {0, 0}, n_left[2] = {0, 0}, n_right[2] = {0, 0};
  int64_t exit_off[2] = {0, 0}, enter_off[2] = {0, 0}, span_off[2] = {0, 0}, size = 0;
};

EventsLayout events_layout(const lh_family* f) {
  const lh::DevSampler& smp = f->sampler;
  EventsLayout lay;
  lay.n_junctions = smp.has_d ? 2 : 1;
  lay.n_genes = smp.n_v + (smp.has_d ? smp.n_d : 0) + smp.n_j;
  for (int j = 0; j < lay.n_junctions; ++j) {
    const lh::DevSampleJunction& J = j == 0 ? smp.vd : smp.dj;
    const int64_t W1 = (int64_t)J.n_rows + 1;
    lay.rows[j] = J.n_rows;
    lay.n_left[j] = J.n_left;
    lay.n_right[j] = J.n_right;
    lay.exit_off[j] = lay.size;
    lay.enter_off[j] = lay.exit_off[j] + J.n_left * W1;
    lay.span_off[j] = lay.enter_off[j] + J.n_right * W1;
    lay.size = lay.span_off[j] + W1 * W1;
  }
  return lay;
}

// K5 on a copy of the forward arrays fwd[m][FS] (it smooths in place; K10 reads both), then K10
int events_launch(lh_family* f, int m, const double* fwd, const double* loglik, double* events, double* genes,
                  hipStream_t stream, bool timed) {
  EventsWs& ew = f->events;
  const size_t FS = f->host.forward_size;
  double* post = ew.post.get<double>();
  if (timed && f->events_timer.begin(stream)) return 1;
  LH_HIP(hipMemcpyAsync(post, fwd, sizeof(double) * FS * m, hipMemcpyDeviceToDevice, stream));
  lh::launch_posterior(f->sampler_dev, m, post, FS, loglik, stream);
  if (timed && f->events_timer.mark(1, stream)) return 1;
  lh::launch_events(f->sampler, f->sampler_dev, m, fwd, post, FS, loglik, ew.scratch.get<double>(), events,
                    (size_t)events_layout(f).size, genes, stream);
  LH_HIP(hipGetLastError());
  return 0;
}

int events_buffers(lh_family* f, int n) {
  EventsWs& ew = f->events;
  return ew.post.ensure(sizeof(double) * f->host.forward_size * n) ||
         ew.scratch.ensure(sizeof(double) * lh::events_scratch_doubles(f->sampler) * lh::events_slots(n));
}

// lh_eval_events_batch_device, and (host) lh_eval_events_batch, as codons_batch
int events_batch(lh_family* f, const std::string& W, const TreeBatch& b, const TableOuts& o, void* hip_stream, bool host) {
  if (int rc = check_batch(f, W, b, true)) return rc > 0;
  DeviceGuard guard(f);
  const EventsLayout lay = events_layout(f);
  const size_t NE = (size_t)lay.size, NG = lay.n_genes;
  if (host) return table_batch(f, W, b, f->events, NE, NG, o, events_batch);
  if (events_buffers(f, b.n)) return 1;  // K5 smooths a copy of the forward arrays: K10 reads both
  return table_batch_device(f, b, f->events, NE, NG, o, hip_stream, &lh_family::events_timer,
                            [&](const double* fwd, const double* ll, double* ev, double* gen, hipStream_t stream) {
                              return events_launch(f, b.n, fwd, ll, ev, gen, stream, f->profile);
                            });
}

}  // namespace

extern "C" {

int lh_events_layout(const lh_family* f, int32_t* n_junctions, int32_t* rows, int32_t* n_left, int32_t* n_right,
                     int64_t* exit_off, int64_t* enter_off, int64_t* span_off, int64_t* size, int32_t* n_genes) {
  if (!f) return fail("lh_events_layout: null family");
  if (!f->have_sampler) return fail("lh_events_layout: lh_family_set_sampler has not been called");
  const EventsLayout lay = events_layout(f);
  if (n_junctions) *n_junctions = lay.n_junctions;
  for (int j = 0; j < 2; ++j) {
    if (rows) rows[j] = lay.rows[j];
    if (n_left) n_left[j] = lay.n_left[j];
    if (n_right) n_right[j] = lay.n_right[j];
    if (exit_off) exit_off[j] = lay.exit_off[j];
    if (enter_off) enter_off[j] = lay.enter_off[j];
    if (span_off) span_off[j] = lay.span_off[j];
  }
  if (size) *size = lay.size;
  if (n_genes) *n_genes = lay.n_genes;
  return 0;
}

int lh_eval_events_batch_device(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha, int32_t R,
                                const lh_events_outputs* outs, void* hip_stream) {
  return events_batch(f, "lh_eval_events_batch_device", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, table_outs(outs),
                      hip_stream, false);
}

int lh_eval_events_batch(lh_family* f, int32_t n, int32_t T, int32_t max_depth, const int32_t* ops, const double* brlen,
                         const double* er, const double* pi, const double* alpha, int32_t R, const lh_events_outputs* outs) {
  return events_batch(f, "lh_eval_events_batch", {n, T, max_depth, ops, brlen, er, pi, alpha, R}, table_outs(outs), nullptr,
                      true);
}

int lh_events_forward_batch(lh_family* f, int32_t n, const double* em, double* loglik, double* events) {
  const std::string W = "lh_events_forward_batch";
  if (!f) return fail(W + ": null family");
  DeviceGuard guard(f);
  if (!f->have_sampler) return fail(W + ": lh_family_set_sampler has not been called");
  if (n <= 0) return n == 0 ? 0 : fail(W + ": negative batch size");
  if (!em) return fail(W + ": null array");
  const size_t C = f->host.n_xmsa, FS = f->host.forward_size, NE = (size_t)events_layout(f).size;
  HostOutputs& out = f->out;
  EventsWs& ew = f->events;
  if (out.loglik.ensure(sizeof(double) * n) || f->forward_dev.ensure(sizeof(double) * FS * n) || events_buffers(f, n) ||
      ew.table.ensure(sizeof(double) * NE * n) || stage_inputs(f, {{em, sizeof(double) * C * n, &f->in.em}}))
    return 1;
  lh_eval_outputs eo{nullptr, nullptr, f->forward_dev.get<double>(), nullptr};
  if (run_forward(f, n, 1, nullptr, nullptr, nullptr, f->in.em.get<const double>(), nullptr, out.loglik.get<double>(), &eo, 0,
                  nullptr))
    return 1;
  if (events_launch(f, n, f->forward_dev.get<const double>(), out.loglik.get<const double>(), ew.table.get<double>(), nullptr,
                    nullptr, false))
    return 1;
  return copy_back(f, nullptr,
                   {{loglik, out.loglik.get(), sizeof(double) * n}, {events, ew.table.get(), sizeof(double) * NE * n}});
}

int lh_events_profile_read(lh_family* f, double* ms, int64_t* n_launches) {
  return profile_read(f, &lh_family::events_timer, ms, n_launches);
}

}  // extern "C"
