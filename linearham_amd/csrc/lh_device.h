// Internal declarations shared by the HIP translation units of liblinearham_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "linearham_amd.h"

namespace lh {

constexpr double kScaleFactor = 0x1p256;      // SCALE_FACTOR, src/utils.hpp:22
constexpr double kScaleThreshold = 0x1p-256;  // SCALE_THRESHOLD, src/utils.hpp:24
constexpr double kLogScaleFactor = 177.445678223345993274;  // log(2^256)

// Launch a kernel with `lds` bytes of dynamic LDS: beyond the 64 KB every kernel may ask for, the kernel's limit is
// raised first (the result of that call is not looked at: a launch that cannot have its LDS fails as a launch).
template <class... P, class... A>
static inline void launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                              const A&... args) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// Wave helpers of the kernels.  wave_sum: the butterfly sum of a wave of 64 in ascending xor distance (a fixed order: the
// kernels that use it promise the same bits whatever the batch); every lane ends with the same value.
__device__ static __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// lane j's v, j wave-uniform
__device__ static __forceinline__ double read_lane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// v of the lane the DPP control kCtrl pairs this one with, inside its row of 16 lanes
template <int kCtrl>
__device__ static __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// schedule op kinds (ops[4k] & 15); bit 4 = push the accumulator to stack slot ops[4k+3] first
// bits 8..: for a tip-into-accumulator / pop op, the number of inner-branch P-matrices the earlier ops need (its own
// one or two follow): K1's prologue packs its matrix work by it
enum : int { OP_CHERRY = 0, OP_TIP_ACC = 1, OP_POP_ACC = 2, OP_PUSH_FLAG = 16, OP_RANK_SHIFT = 8 };

// Walk ops: what K1 executes.  K0c (schedule_check_kernel, lh_prune.hip) validates a sample's schedule ON THE
// DEVICE and rewrites it with every cherry that can be folded into its consumer replaced by a table look-up: for
// a cherry (y, z) under branch c the vector P_c (P_y[:, s_y] o P_z[:, s_z]) takes 16 values per (sample, rate)
// (25 with N tips), which K1's prologue tabulates; then
//   cherry + tip-into-accumulator      ->  W_CTIP      a = table[s_y][s_z] o tipcol_w         (no mat-vec)
//   pushed cherry + pop                ->  W_CTAB_ACC  a = table[s_y][s_z] o (P_first a)      (one mat-vec, no push / pop)
// A walk op is an 8-byte descriptor (WalkOp in lh_prune.hip).
enum : int { W_CHERRY = 0, W_TIP_ACC = 1, W_POP = 2, W_CTIP = 3, W_CTAB_ACC = 4 };

// K0c's output and K1's scratch area (all device memory, sized by prune_ws_sizes)
struct PruneWs {
  double* scratch;    // per (sample, rate): [n_mat + n_tab][16] P-matrices (walk order, then the cherry branches'),
                      // then [n_tab][E][4] cherry tables, E = 16 or 25
  int2* wops;         // [n][T-2] walk-op descriptors
  double* wlen;       // [n][T-2] branch length of inner-branch matrix i of the prologue's list (walk order, then the tables')
  int4* tabs;         // [n][(T-1)/2] cherry tables: tip y, tip z, the cherry's node
  int4* hdr;          // [n] walk ops, matrices, tables, error (malformed schedule: the sample's results are NaN)
  int32_t* err_flag;  // set when any sample of any launch had a malformed schedule (lh_family_status reads and clears it)
};
struct PruneWsSizes {
  size_t scratch_doubles_per_rate;  // per (sample, rate)
  size_t tabs_per_sample;
};
PruneWsSizes prune_ws_sizes(int T, bool mixed_n);
// K0c beside K0a (eval_device, lh_capi.hip): launch_prune puts the schedule kernel (K0c, or the register-stack forms' stack
// check) on `sched` instead of its own stream and calls join() between that launch and K1's.  join() must order
// launch_prune's stream behind `sched` (and behind whatever else K1 has to wait for); nonzero fails the launch.
struct PruneFork {
  hipStream_t sched;
  std::function<int()> join;
};

// Device copy of lh_segments / lh_junction / family constants (all pointers are device pointers).
struct DevSegments {
  int32_t n_genes;
  int32_t n_chunks;      // ceil(longest segment / 8)
  // Consensus form (lh_family_create builds it when the genes of the set are site-aligned and alike, as the
  // Smith-Waterman candidates of one rearrangement are): per covered alignment site the u-column most genes
  // take there; a gene's product is then (prefix product of the consensus up to its last site) / (prefix up to
  // its first site) x the few factors where it departs from the consensus.  cons_sites == 0: not available.
  int32_t cons_sites;        // covered sites (<= 510)
  int32_t cons_diffs;        // diff entries per gene (padded)
  const uint16_t* cons_col;  // [cons_sites] consensus u-column (index or byte offset like inds_c)
  const uint32_t* cons_rng;  // [n_genes] first | (last + 1) << 16 | rounds of 8 departures << 25, in consensus positions
  const uint32_t* cons_dif;  // [cons_diffs][n_genes] position | own u-column << 16; padding = position
                             // cons_sites (reciprocal 1.0) | the sentinel column (emission 1.0)
  const uint4* inds_c;   // [n_chunks][n_genes] eight 16-bit u-column indices (or byte offsets, see
                         // DevFamily::idx_byte_offsets) per entry (lane g's next
                         // eight factors in one coalesced 16-byte load), padded with the sentinel
                         // column C whose emission is 1.0
};

// Junction tables as K2b reads them: gene dimensions padded to a multiple of 64 with entries that
// contribute nothing (zero transitions, emission index = the zero sentinel), so that every lane of a
// wave loads and computes unconditionally.  Emission indices point into the compact junction-column
// vector (DevFamily::jcols); position n_jcols is the sentinel holding 0.0.
struct DevJunction {
  int32_t n_rows, n_left, n_right;
  int32_t left_pad, right_pad;  // padded gene counts (row strides)
  const double *enter_lo;       // [left_pad]
  const double *left_trans;     // [n_rows][left_pad], row 0 = enter_trans
  const double *left_lo;        // [n_rows][left_pad]
  const int32_t* left_xmsa;     // [n_rows][left_pad]
  const double *right_gp_nli;   // [right_pad][4]
  const double *right_ntt;      // [right_pad][4][4] stored transposed: [r][b][a] = transition a -> b
  const double *right_nlo;      // [n_rows][right_pad][4]
  const double *right_trans, *right_gp_li;  // [n_rows][right_pad]
  const int32_t *right_xmsa;    // [n_rows][right_pad]
  const int32_t *nti_xmsa;      // [n_rows][right_pad][4]
  const double *exit_nlo;       // [right_pad][4]
  const double *exit_trans, *exit_gp_li;  // [right_pad]
  const int32_t* row_pat;       // [n_rows] K1 pattern of the row's alignment site (>= n_prune: the all-N pattern
                                // or a family without an alignment); used by the extended-range mode only
};

// Two reductions happen once per family, on the host (lh_family_create):
//  * identical alignment columns (site patterns) are pruned once: K1 runs over the n_pat distinct
//    columns of the MSA, msa is stored pattern-major;
//  * xMSA columns that pair the same naive base with the same pattern have the same emission: K2 works
//    on (naive base, pattern) pairs ("u-columns").  With an alignment there are always n_ucol = 5 n_prune + 5 slots,
//    numbered by their place in K1's output planes: u = base * n_prune + pattern, the all-N pattern's five pairs last;
//    a pair no xMSA column uses keeps its slot (u_base = 0xff), so K2a fills its emission vector from the planes
//    without a look-up.  Every index table below is in u-column space.  Limits that follow: K2a's LDS emission vector
//    takes (n_ucol + 1) * 8 = (5 n_prune + 6) * 8 bytes per sample, and the segment index chunks can hold 16-bit BYTE
//    offsets (idx_byte_offsets) while that is < 65 536, i.e. n_prune <= 1637.  Families without an alignment
//    (n_seqs == 0) keep their columns one to one.
struct DevFamily {
  int32_t has_d, n_seqs, n_sites, n_xmsa;  // as described by the caller
  int32_t n_pat;                           // distinct alignment columns
  int32_t n_prune;                         // K1's site dimension: n_pat minus the all-N pattern, which
                                           // comes last and whose emission is 1 whatever the tree
  int32_t msa_mixed_n;                     // 1 if some pattern mixes N with bases (K1 then handles N tips)
  int32_t n_ucol;                          // (naive base, pattern) pairs (K2's column dimension): with an alignment
                                           // 5 n_prune + 5, u = base * n_prune + pattern (the all-N pattern's five last)
  int32_t idx_byte_offsets;                // 1: the segment index chunks hold byte offsets (index * 8),
                                           // possible when (n_ucol + 1) * 8 fits 16 bits
  const uint8_t* msa;                      // [n_seqs][n_prune]
  // the same states as BIT PLANES for K1's assembly walk -- [n_seqs][ceil(n_prune / 128)][2 site sets][2 or 3] 64-bit masks:
  // bit l of plane (row i, block b, set s, bit q) is bit q of the state of row i at pattern 128 b + 64 s + l (patterns past
  // the last one repeat it); alignments that mix N with bases (msa_mixed_n) carry a third plane per set flagging N (state
  // bits 0 there).  A wave fetches the 32 / 48 bytes of (row, its block) with one / two scalar loads.
  const uint64_t* msa_planes;
  const int32_t* site_pat;                 // [n_sites] pattern of alignment site j (n_prune = the all-N pattern)
  const int32_t* u_pat;                    // [n_ucol] pattern of u-column u
  const uint8_t* u_base;                   // [n_ucol] its naive base (4 = N; 0xff: no xMSA column is this pair)
  const int32_t* ucol_of_col;              // [n_xmsa] u-column of the caller's column c
  const int32_t* col_of_ucol;              // [n_ucol] one caller column per u-column (-1: none)
  DevSegments vpadding, vgerm, dgerm, jgerm, jpadding;
  const double *vgerm_gene_prob, *vpadding_transition, *vgerm_trans_prod, *jpadding_transition;
  DevJunction vd, dj;
  int32_t max_genes;      // max over regions of the gene count
  int32_t n_jcols;        // distinct u-columns referenced by the junction tables
  const int32_t* jcols;   // [n_jcols] their u-column indices, ascending
  int64_t gem_size;       // doubles per sample of germline/padding emission products (2nV + nD + 2nJ)
  int64_t forward_size;   // doubles per sample in the compact forward output
  int64_t scaler_size;    // ints per sample in the scaler-count output
};

// 1/v to ~1 ulp from the hardware estimate and two Newton steps (normal-range v; a quarter of the IEEE division
// sequence).
__device__ static inline double fast_rcp(double v) {
  double r = __builtin_amdgcn_rcp(v);
  r = fma(fma(-v, r, 1.0), r, r);
  r = fma(fma(-v, r, 1.0), r, r);
  return r;
}

// The 2^256 rescaling of a conditional-likelihood vector (entries >= 0) goes on until its largest entry is back at or
// above 2^-256: a tip joining the accumulator falls by one mismatch, but the join of two subtrees that each sit up to 256
// binades down leaves the product up to 512 and a mismatch further down.  How many multiplications by 2^256 that takes
// (1 .. 3), from the high word hw < 0x2FF00000 of the largest entry: with its biased exponent E >= 1 the entry is
// a < 2^-256 and a 2^(256 n) >= 2^-256 needs E + 256 n >= 767.  A subnormal largest entry (E = 0: bits are lost already)
// gets the three of E = 1, and a vector with nothing left to bring back (hw = 0) is rescaled once, as it always was.
__device__ static __forceinline__ int rescale_steps(unsigned hw) {
  return hw == 0u ? 1 : (int)((1022u - (hw >> 20)) >> 8);
}

// K4 (lh_sample.hip): what a backward sampling step needs of one junction, in the unfused form FillTransition
// multiplies it together (src/HMM.cpp:964-1089), so that every weight has the bits of the dense matrices.
// Unpadded [W][nL] / [W][nR] tables; dense = index in the reference's junction state vector.
struct DevSampleJunction {
  int32_t n_rows, n_left, n_right, n_states;
  int32_t right_first_block;     // 1: the right genes' states precede the left genes' in the dense vector
  const int32_t* state_class;    // [S] kind (0 left, 1 NTI, 2 right germline) | NTI base << 2 | gene << 4
  const int32_t* left_rows;      // [nL] the gene has states on rows 0 .. left_rows - 1
  const int32_t* left_dense;     // [nL] dense index of its row-0 state
  const double* left_lo;         // [W][nL] landing_out of the row-i state
  const double* left_trans;      // [W][nL] transition into the row-i state (row 0: out of the germline region)
  const double* enter_lo;        // [nL] landing_out of the last germline-region position
  const int32_t* right_dense;    // [nR] dense index of the gene's NTI state A
  const int32_t* right_first;    // [nR] first row with a germline state of the gene (W: none)
  const double* gp;              // [nR] gene_prob
  const double* nli;             // [nR][4] nti_landing_in
  const double* ntt;             // [nR][4][4] nti_transition a -> b
  const double* nlo;             // [W][nR][4] nti_landing_out into the row-i germline state
  const double* li;              // [W][nR] landing_in of the row-i germline state
  const double* rtrans;          // [W][nR] transition into the row-i germline state from the row before
  const double* exit_nlo;        // [nR][4] nti_landing_out into the germline region x prod
  const double* exit_trans;      // [nR] transition into the germline region x prod (0: no last-row state)
  const double* exit_li;         // [nR] landing_in of the germline region's first position
  const double* prod;            // [nR] product of the in-region transitions (src/HMM.cpp:872-876)
};

struct DevSampler {
  int32_t has_d, n_v, n_d, n_j, states_per_sample, words_per_sample;
  DevSampleJunction vd, dj;
};

// K4: states[n][states_per_sample] from the compact forward arrays fwd[n][forward_size] and each sample's
// std::mt19937 outputs words[n][words_per_sample].
// smp_dev: the device copy of smp (the kernel reads the table addresses from it instead of holding forty of them in
// scalar registers).
void launch_sample(const DevSampler& smp, const DevSampler* smp_dev, int n, const double* fwd, size_t forward_size, const uint32_t* words,
                   int words_per_sample, int32_t* states, hipStream_t stream);

// K5 (lh_posterior.hip): the compact forward arrays post[n][forward_size] are replaced in place by the posterior state
// marginals of the same entries (NaN for a sample whose loglik is not finite).
void launch_posterior(const DevSampler* smp_dev, int n, double* post, size_t forward_size, const double* loglik,
                      hipStream_t stream);
// K5's reduction: w[n] = exp(lw - max lw), lw = loglik - log_offset (log_offset may be null; 0 where lw is not
// finite), stats[3] = max lw, sum w, sum w^2; weighted_sum[forward_size] = sum_i w_i post[i] (skipped if null), through
// partial[posterior_slabs(n)][forward_size].  Fixed summation order, no atomics.
int posterior_slabs(int n);
void launch_posterior_reduce(int n, size_t forward_size, const double* post, const double* loglik, const double* log_offset,
                             double* w, double* partial, double* weighted_sum, double* stats, hipStream_t stream);
// out[j] = sum over k < n_slabs, in order, of partial[k][j] (K5's last reduction step; K6b's too)
void launch_slab_sum(int n_slabs, size_t size, const double* partial, double* out, hipStream_t stream);
// K5's slab reduction alone, for weights launch_posterior_reduce has already written: weighted_sum[size] = sum_i w_i
// rows[i][0..size) through partial[posterior_slabs(n)][size] (K9 reduces two arrays with one set of weights)
void launch_weighted_slabs(int n, size_t size, const double* rows, const double* w, double* partial, double* weighted_sum,
                           hipStream_t stream);

// K9 (lh_codon.hip): exact posterior distributions of the naive sequence's codons that touch a junction row ("window
// codons"), and the sample's V / D / J gene posteriors, from the compact forward arrays (read only).
// Chain positions: 0 = V genes, 1 .. W_vd = V-D rows, then (igh) D genes, D-J rows, J genes; light chains V | rows | J.
// A window covers npos = 2 or 3 consecutive positions, slot 0 the lowest.  A position's entries (the compact layout's: genes of
// a region, or left | NTI x 4 | right of a row) carry a local code each, codes[code_off[slot] + entry] < ncodes[slot] (5: one
// base; 25: 5 * first base + second base of a germline gene that writes two of the codon's sites); the codon index
// 25 b1 + 5 b2 + b3 of a triple of entries is sum_slot mult[slot] * code.
struct CodonWindow {
  int32_t npos, top, out;  // top: chain position of the highest slot; out: index of the window in the output
  int32_t mult[3], ncodes[3], code_off[3];
};
struct CodonTables {
  int32_t n_window, n_genes, n_pos;
  int32_t max_vec;             // entries of the largest position vector
  const CodonWindow* win;      // [n_window], by `top` descending
  const uint8_t* codes;        // the code pool
};
int codon_slots(int n);  // samples that are in flight at once: scratch[codon_slots(n)][4][max_vec] doubles
// windows[n][n_window][125], genes[n][n_genes] (V | D | J); NaN for a sample whose loglik is not finite
void launch_codons(const DevSampler* smp_dev, const CodonTables& t, int n, const double* fwd, size_t forward_size,
                   const double* loglik, double* scratch, double* windows, double* genes, hipStream_t stream);

// K10 (lh_events.hip): exact posteriors of the recombination events, from the compact forward arrays fwd and K5's
// posteriors of the same entries post (both read only).  Per sample one flat row events[events_size]: per junction (V-D,
// then D-J)  exit[nL][W+1] | enter[nR][W+1] | span[W+1][W+1]  (include/linearham_amd.h, lh_events_layout); genes[n][nV +
// nD + nJ] (may be null) are K5's gene posteriors.  NaN for a sample whose loglik is not finite.
int events_slots(int n);  // samples that are in flight at once: scratch[events_slots(n)][events_scratch_doubles(smp)]
size_t events_scratch_doubles(const DevSampler& smp);
void launch_events(const DevSampler& smp, const DevSampler* smp_dev, int n, const double* fwd, const double* post,
                   size_t forward_size, const double* loglik, double* scratch, double* events, size_t events_size,
                   double* genes, hipStream_t stream);

// K6 (lh_naive_probs.hip): exact posterior probabilities of candidate naive sequences.
// K6a: em[k][c] = 1 where candidate k has the naive base of the caller's column c at its site, else 0 (the
// indicator emissions of the constrained forward sweep), for K candidates of L sites and C columns.
void launch_candidate_indicators(int K, int L, int C, const uint8_t* seqs, const int32_t* col_site, const uint8_t* col_base,
                                 double* em, hipStream_t stream);
// K6b's tables (lh_family_set_candidates): the log emissions K2a writes per sample are lem[n][n_lem] (LogEmRequest);
// the first n_vlem of them are the u-columns of the variable sites, which idx[V][K] (uint16) names per (variable site,
// candidate); agree[n_lem] counts the sites where all candidates agree on each u-column.
struct CandidateTables {
  int32_t K, V, n_lem, n_vlem;
  const uint16_t* idx;
  const double* agree;
  const double* log_prior;  // [K]
};
// log_cand[n][K] (may be null) = log_prior + sum of the candidate's log emissions - loglik (NaN for a row whose loglik is
// not finite); base[n] scratch; when w is not null, partial[candidate_slabs(n)][K] receives the slabs' sums
// of w_i exp(log_cand[i][k]) (rows with w_i = 0 skipped), in order.
int candidate_slabs(int n);
size_t candidate_lds_limit();  // largest n_vlem * 8 the scoring kernel takes
void launch_candidates(const CandidateTables& t, int n, const double* lem, const double* loglik, const double* w,
                       double* base, double* log_cand, double* partial, hipStream_t stream);

// K6c (lh_collect.hip): the naive sequences of K4's state rows.  Every pointer is one the family already holds: the K6
// twin's germline segments and junction column matrices (its columns are the caller's one to one), K4's state classes
// and K6a's caller column -> (site, naive base) map.
struct CollectSegments {
  int32_t n_genes, n_chunks;
  const uint4* inds;  // DevSegments::inds_c of the twin
};
struct CollectJunction {
  int32_t n_rows, n_left, n_right, left_pad, right_pad, n_states;
  const int32_t *left_xmsa, *right_xmsa, *nti_xmsa;  // the twin's DevJunction tables (compact junction-column positions)
  const int32_t* state_class;                         // DevSampleJunction::state_class
};
struct CollectTables {
  int32_t L, has_d, states_per_sample, n_cols;
  int32_t seg_scale, seg_sentinel;  // the twin's segment entries: column * seg_scale, padding = seg_sentinel
  CollectSegments vg, dg, jg;
  CollectJunction vd, dj;
  const int32_t* jcols;  // the twin's compact junction-column list (caller columns)
  int32_t n_jcols;
  const int32_t* col_site;
  const uint8_t* col_base;
  uint64_t hash_mask;  // ~0, or the low LH_COLLECT_HASH_BITS bits (DebugOptions)
};
// seqs[n][L] (A,C,G,T,N = 0..4) and hash[n] of states[n][states_per_sample]
// The sequence hash K6c and K7 share: XOR over the sequence's 8-byte words (little-endian, padded to a whole word) of a
// 64-bit mix of (word, position), then one more mix with the length.  XOR is exact and order-free.
__host__ __device__ inline uint64_t mix64(uint64_t z) {  // the splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t hash_word(uint64_t word, int q) {
  return mix64(word + 0x9e3779b97f4a7c15ull * (uint64_t)(q + 1));
}
__host__ __device__ inline uint64_t hash_finish(uint64_t h, int length) { return mix64(h ^ (uint64_t)length); }

void launch_collect(const CollectTables& t, int n, const int32_t* states, uint8_t* seqs, uint64_t* hash, hipStream_t stream);
size_t collect_lds_bytes(int L);

// The sequence store (lh_collect.hip): a growable device array of distinct byte sequences, store[K][L], behind three
// kernels that are generic over where a batch's rows lie.  A row source answers two questions: n_slots(src), how many
// flat slots the batch has (at most INT32_MAX), and slot_row(src, x), the src.L bytes of slot x or null for a slot without
// a row.  K6c's source is FlatRows, K7's is LineageBatch.
struct FlatRows {
  int32_t n, L;
  const uint8_t* seqs;  // [n][L]
};
__host__ __device__ inline size_t n_slots(const FlatRows& r) { return r.n > 0 ? (size_t)r.n : 0; }
__device__ inline const uint8_t* slot_row(const FlatRows& r, int x) { return r.seqs + (size_t)x * r.L; }

// K7 (lh_lineage.hip): the lineage slots of a batch.  A batch holds n tree samples with `draws` ancestral draws each: n * draws
// virtual samples, v standing for row v / draws and draw v % draws.  Slot s < P of virtual sample v is the row
// anc[v][path[row*P + s] - T][0..L) of K3's output (path entries outside T .. 2T-3 are padding), slot P the row
// naive[row][0..L), the same for every draw of the row.  A flat slot is v*(P+1)+s.
struct LineageBatch {
  int32_t n, T, L, P;
  const uint8_t* anc;    // [n * draws][T-2][L]
  const uint8_t* naive;  // [n][L]
  const int32_t* path;   // [n][P]
  uint64_t hash_mask;
  int32_t draws = 1;
};
__host__ __device__ inline size_t n_slots(const LineageBatch& b) {
  return b.n > 0 ? (size_t)b.n * (size_t)b.draws * (b.P + 1) : 0;
}
// the row of slot (v, s), null for a padding slot
__device__ inline const uint8_t* slot_row(const LineageBatch& b, int v, int s) {
  const int i = b.draws > 1 ? v / b.draws : v;
  if (s == b.P) return b.naive + (size_t)i * b.L;
  const int node = b.path[(size_t)i * b.P + s];
  if (node < b.T || node >= 2 * b.T - 2) return nullptr;
  return b.anc + ((size_t)v * (b.T - 2) + (node - b.T)) * b.L;
}
__device__ inline const uint8_t* slot_row(const LineageBatch& b, int x) { return slot_row(b, x / (b.P + 1), x % (b.P + 1)); }
constexpr uint64_t kLineagePadHash = 0;  // LH_LINEAGE_PAD_HASH
// nt_hash, aa_hash [n * draws][P+1]
void launch_lineage(const LineageBatch& b, uint64_t* nt_hash, uint64_t* aa_hash, hipStream_t stream);

// The store's kernels, instantiated for FlatRows and LineageBatch (a slot outside the batch counts as one without a row).
// flag[x] = 1 where slot x differs from store[ids[x]] (ids[x] < 0: 0; ids[x] >= K or no row: 1)
template <class Rows>
void launch_store_verify(const Rows& src, int K, const int32_t* ids, const uint8_t* store, uint8_t* flag,
                         hipStream_t stream);
// store[pairs[2p]] = slot pairs[2p + 1] for p < n_pairs (pairs outside the store or the batch, or without a row: skipped)
template <class Rows>
void launch_store_append(const Rows& src, int K, int n_pairs, const int32_t* pairs, uint8_t* store, hipStream_t stream);
// out[q][..] = slot slots[q] for q < n_out (slots without a row read as N)
template <class Rows>
void launch_store_gather(const Rows& src, int n_out, const int32_t* slots, uint8_t* out, hipStream_t stream);

// P = I + U expm1(lambda * t*r) Uinv, clamped at 0 (K1's prologue).
// e: lambda[4] | U[4][4] | Uinv[4][4]
// (mode 0 is the stationary one, eigenvalue 0 -- K0a orders them so -- and contributes nothing: three modes are summed)
__device__ static inline void compute_pmatrix(const double* __restrict__ e, double tr, double P[4][4]) {
  double ex[4];
#pragma unroll
  for (int k = 1; k < 4; ++k) ex[k] = expm1(e[k] * tr);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = (i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 1; k < 4; ++k) v = fma(e[4 + i * 4 + k] * ex[k], e[20 + k * 4 + j], v);
      P[i][j] = fmax(v, 0.0);
    }
}

// ---- kernel launchers (each enqueues on `stream`, no synchronisation) -------------------------

// K0a: per sample: discrete-Gamma mean rates from alpha, GTR eigendecomposition.
// eig layout per sample: lambda[4] | U[4][4] | Uinv[4][4]  (36 doubles)
void launch_model_setup(int n, int R, const double* er, const double* pi, const double* alpha,
                        double* rates, double* eig, hipStream_t stream);

// K1: Felsenstein pruning over the MSA sites with the naive tip factored out; each workgroup first
// computes the P-matrices of its (sample, rate): P = I + U expm1(lambda t r) U^-1 for every branch,
// inner-branch matrices in schedule order into the scratch area pmat[n][R][T-2][2][16] (op k: [0] =
// matrix of the child whose CLV is in the accumulator, [1] = matrix of the popped child), tip-branch
// matrices into its LDS tip table.
// site_lik[n][R][5][n_prune], site_scal[n][R][n_prune]
// test_every_op: the cherry-table form runs its C++ walk (a rescaling test after every op) where it would run the assembly
// walk (a test after every fourth): the extended-range mode asks for it (lh_prune.hip, launch_prune).
// Returns the number of rate planes left in site_lik / site_scal: R, or 1 if the rates were mixed in K1
// (site_lik[n][1][5][n_prune], site_scal[n][1][n_prune]); K2a is to be run with that count.
int launch_prune(const DevFamily& fam, int n, int R, int T, int max_depth, const int32_t* ops,
                 const double* brlen, const double* rates, const double* eig, const PruneWs& ws, const double* pi,
                 double* site_lik, int32_t* site_scal, hipStream_t stream, bool allow_fused = true,
                 bool test_every_op = false, const PruneFork* fork = nullptr);
// the kernel form the calling thread's last launch_prune chose ("w6<3,false>", "seg4<4,true>", "ct6<16,false,false,true>":
// kernel<depth, N-aware, all rates in one workgroup, assembly walk>) and, after a -1, why it failed
const char* prune_last_form();
const char* prune_last_error();

// GTR eigendecomposition only (K0a's last role): eig[n][36]
void launch_gtr_setup(int n, const double* er, const double* pi, double* eig, hipStream_t stream);

// K3: ancestral-sequence sampling (lh_asr.hip).  site_lik / site_scal are K1's UNMIXED per-rate planes
// (launch_prune with allow_fused = false).  With `draws` = D the launch covers n * D virtual samples, v standing for tree
// sample v / D and draw v % D: what belongs to the tree sample (ops, brlen, rates, eig, pi, hdr, the planes, naive) is
// read at the row, what a draw owns lies at v: clv[n*D][T-2][2][asr_slots(L, R)][2] is scratch; anc[n*D][T-2][n_sites]
// receives the sampled state of inner node T + i at every site, rate_choice[n*D][n_sites] the drawn category (K3a ->
// K3b).  The Philox sample number of (row, d) is sample0 + row + (d << 32): draw 0 is the single draw of D = 1.
// K3s runs once per row (desc[n]).  Returns nonzero if the tree is too large for the kernel's LDS tables.
int launch_asr(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
               const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
               const uint8_t* naive, uint64_t seed, uint64_t sample0, double* clv, void* desc, uint8_t* anc,
               uint8_t* rate_choice, const int4* hdr /* K0c's verdicts, PruneWs::hdr */, hipStream_t stream,
               int draws = 1);
size_t asr_desc_bytes(int T);  // per sample, of the schedule descriptors `desc` (scratch, K3s -> K3b)
size_t asr_lds_bytes(int T, int L, int R, int n_prune);
size_t asr_slots(int L, int R);  // slots per sample in K3's CLV area: clv[n][T-2][2][asr_slots] double2

// One schedule op as the sampling kernel reads it (two int4, fetched with scalar loads): everything that K3b
// would otherwise have to derive per op from the K1 schedule with dependent look-ups.
//   a.x  kind | stack slot of the op << 4 | (slot + 1 the NEXT op pushes the accumulator to, or 0) << 8
//   a.y  MSA row of tip child y (cherry, tip-acc), else 0        a.z  MSA row of tip child z (cherry), else 0
//   a.w  op that produced the sibling a pop op takes from the stack, else 0
//   b.x  tip id y (tip table row)   b.y  tip id z   b.z  inner node (minus T) this op produces
//   b.w  inner node (minus T) of the popped sibling (pop), else 0
struct AsrOp {
  int4 a, b;
};

// K3s alone: desc[n][T - 2] from the schedules (K0c's verdicts in hdr: a rejected sample's descriptors are not written)
void launch_asr_sched(int n, int T, const int32_t* ops, const int4* hdr, void* desc, hipStream_t stream);

// K11: exact ancestral-state marginals along a lineage path (lh_ancestral.hip).  Inputs as launch_asr's, with
// naive_prob[n][n_sites][5] in place of the naive sequences and path[n][P] (seed's parent .. root, padding after).  marg
// [n][P][n_sites][4] (may be null: the rate posteriors alone) and rate_post [n][n_sites][R] (may be null).  A sample whose
// path is not a chain under its own schedule, or whose schedule K0c rejected, gets NaN in its marg row; the first raises
// *err_flag.  Scratch per sample: anc_ws_bytes.  Returns nonzero if the launch cannot be made (LDS tables, grid).
struct AncWs {
  double* clv;      // [n][R][T-2][2][patterns rounded up to 8] double2
  double* part;     // [n][R][P][n_sites][4]
  double* tvec;     // [n][n_sites][5]
  double* rho;      // [n][n_sites][R], used when rate_post is null
  int32_t* chain;   // [n][P]
  int32_t* plen;    // [n]
  void* desc;       // [n] asr_desc_bytes(T)
};
struct AncWsBytes {
  size_t clv, part, tvec, rho, chain;  // per sample (desc: asr_desc_bytes)
  size_t total() const { return clv + part + tvec + rho + chain; }
};
AncWsBytes anc_ws_bytes(int T, int L, int R, int n_prune, int P);
size_t anc_lds_bytes(int T);
int launch_ancestral(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                     const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                     const double* naive_prob, const int32_t* path, int P, const AncWs& ws, double* marg, double* rate_post,
                     const int4* hdr, int32_t* err_flag, hipStream_t stream);
// K11a: site_base[n][L][5] from K5's posteriors post[n][forward_size]; off[5 L + 1] / idx: per (site, base) the compact
// entries that write it.  A row whose loglik is not finite is NaN.
void launch_site_base(int n, int L, size_t forward_size, const int32_t* off, const int32_t* idx, const double* post,
                      const double* loglik, double* site_base, hipStream_t stream);
// For the weighted reduction: ends[n][2][L][4] = slot 0 and the last slot of every sample's marg (ends null: not wanted);
// ll_used[n] = loglik, NaN where plen is 0 (launch_ancestral found no path: the row's weight becomes 0).
void launch_ancestral_ends(int n, int P, int L, const int32_t* plen, const double* marg, const double* loglik, double* ends,
                           double* ll_used, hipStream_t stream);
// K11r, K3s and K11c alone: ws.tvec, rho (rate_post, or ws.rho where that is null), ws.desc, ws.chain, ws.plen.  What
// launch_ancestral runs in front of K11b; K12 (lh_substitutions.hip) runs its own kernels behind it.
void launch_ancestral_front(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* pi,
                            const double* site_lik, const int32_t* site_scal, const double* naive_prob, const int32_t* path,
                            int P, const AncWs& ws, double* rate_post, const int4* hdr, int32_t* err_flag, hipStream_t stream);
size_t anc_lp(int n_prune);  // patterns per CLV plane: n_prune + 1 rounded up to 8

// The R per-rate partial tables of every sample added in rate order, a thread per output cell (rate_sum_kernel,
// lh_ancestral.hip: K11m, K12m, K13m) -- fixed order, no atomics, the same bits whatever the batch.  part[n][R][slots][width]
// -> out[n][slots][width] (null: nothing is done).  Slot s of a sample is live if s < plen, or if it is the last and
// last_live; every other slot gets 0, a sample whose plen is 0 NaN.
void launch_rate_sum(int n, int R, int slots, size_t width, bool last_live, const int32_t* plen, const double* part,
                     double* out, hipStream_t stream);
// A table per pattern spread over the sites (site_gather_kernel, lh_ancestral.hip; K13's cond, K15's cond_edge):
// table[rows][n_prune + 1][width] -> out[rows][n_sites][width], width 20 (K13) or 80 (K15).
void launch_site_gather(const DevFamily& fam, long long rows, int width, const double* table, double* out,
                        hipStream_t stream);

// K12 (lh_substitutions.hip): exact joint posteriors of the two ends of every edge of a seed's lineage.  Inputs as
// launch_ancestral's plus seed_tip (1 .. T-1, the same for every sample): the tip must be a child of path[0] under the
// sample's own schedule, else the sample is treated as one with a bad path (NaN rows, *err_flag bit 1).  Every output may
// be null: edge[n][P][n_sites][4][4] (padding slots 0), naive_edge[n][n_sites][5][4], chain_counts[n][n_sites][4][4],
// seed_edge[n][n_sites][4][4] (slot 0 of edge), edge_load[n][P+1], rate_post[n][n_sites][R]; plen_out[n] (null: ws.plen)
// receives the path lengths, 0 for a sample without a valid path.  Tables are indexed [ancestor state][descendant state].
// Scratch per sample: sub_ws_bytes on top of anc_ws_bytes' clv, tvec, rho and chain (AncWs::part is not used).
struct SubWs {
  double* cc;    // [n][R][n_sites][16]
  double* ne;    // [n][R][n_sites][20]
  double* se;    // [n][R][n_sites][16]
  double* el;    // [n][R][P+1]
  double* edge;  // [n][R][P][n_sites][16], only where edge is asked for
};
struct SubWsBytes {
  size_t cc, ne, se, el, edge;  // per sample
  size_t total(bool with_edge) const { return cc + ne + se + el + (with_edge ? edge : 0); }
};
SubWsBytes sub_ws_bytes(int L, int R, int P);
size_t sub_lds_bytes(int T, int P);
struct SubOut {
  double *edge, *naive_edge, *chain_counts, *seed_edge, *edge_load, *rate_post;
};
int launch_substitutions(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                         const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                         const double* naive_prob, const int32_t* path, int P, int seed_tip, const AncWs& ws, const SubWs& sws,
                         const SubOut& out, const int4* hdr, int32_t* err_flag, hipStream_t stream);

// K13 (lh_ancestral_probs.hip): exact posterior probabilities of candidate ancestral sequences at one node of a seed's
// lineage, node 0 = the seed's parent (slot 0), 1 = the MRCA (the sample's last slot).
// K13b + K13m behind launch_ancestral_front (which takes naive_prob for K11r; its tvec and rho are not read here): table
// [n][n_prune + 1][5][4], P(x_node = c | column of the pattern, naive base b), NaN for a sample without a valid path (*err_flag
// raised, ws.plen 0); cond[n][n_sites][5][4] (may be null) is the same table per site.  Scratch: AncWs with `part` sized by
// cond_ws_bytes.  Returns nonzero if the launch cannot be made (LDS tables, grid).
// slot (may be null: `node` decides, and the launch is one of the two fixed forms): [n] device array, for every sample the
// slot of its own path the table is formed at; `node` is then not looked at.  A slot outside 0 .. plen - 1 leaves the sample
// without a path (ws.plen 0) and raises bit 2 of err_flag[0]; err_flag[1] keeps 0x7fffffff - (slot_row0 + the first such
// sample), slot_row0 being the launch group's first row in its call.
struct CondWsBytes {
  size_t part, table;  // per sample
};
CondWsBytes cond_ws_bytes(int R, int n_prune);
int launch_ancestral_cond(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen,
                          const double* rates, const double* eig, const double* pi, const double* site_lik,
                          const int32_t* site_scal, const double* naive_prob, const int32_t* path, int P, int node,
                          const AncWs& ws, double* table, double* cond, const int4* hdr, int32_t* err_flag,
                          hipStream_t stream, const int32_t* slot = nullptr, int slot_row0 = 0);
// em[n][C] = 0 in the rows whose plen is 0
void launch_row_mask(int n, int C, const int32_t* plen, double* em, hipStream_t stream);
// K13e for the pairs q0 .. q0 + count of a launch group, pair q = row * K + candidate: out[count][C] from the group's
// emissions em[rows][C] (caller columns), its tables and path lengths, seqs[K][L] and K6a's column -> (site, base) map
void launch_pair_emissions(const DevFamily& fam, int K, long long q0, int count, const uint8_t* seqs, const int32_t* col_site,
                           const uint8_t* col_base, const int32_t* plen, const double* em, const double* table, double* out,
                           hipStream_t stream);
// log_cand[q] = pair_ll[q - q0] - open_ll[row], NaN where the row has no path or open_ll is not finite; prob[q] = exp of it
// (either may be null)
void launch_pair_finish(int K, long long q0, int count, const double* pair_ll, const double* open_ll, const int32_t* plen,
                        double* log_cand, double* prob, hipStream_t stream);

// K14 (lh_node_codon.hip): exact codon marginals of a node of a seed's lineage, from K9's naive codon posteriors and K13b's
// tables.  NodeCodonTables says where every codon's naive posterior comes from: codon_src[c] >= 0 is its window in K9's
// output; -1 - k makes it germline codon k, a codon inside one germline region: germ[k] = (offset of its codes, the region's
// first gene in K9's genes, the region's gene count, 0) and codes[offset + g] the triple 25 b1 + 5 b2 + b3 gene g of the
// region writes on the codon's sites (N where it writes none).  Entry e of the codon is the sum of the posteriors of the
// genes whose code is e, in ascending gene order.
struct NodeCodonTables {
  int32_t n_codons, n_window, n_genes;
  const int32_t* codon_src;  // [n_codons]
  const int4* germ;          // [germline codons]
  const uint8_t* codes;
};
// Q[n][n_codons][125] from K9's windows[n][n_window][125] and genes[n][n_genes]
void launch_naive_codons(const NodeCodonTables& t, int n, const double* windows, const double* genes, double* Q,
                         hipStream_t stream);
// codons[n][n_codons][64] and change[n][n_codons][4] (either may be null) from Q and K13m's table[n][n_prune + 1][5][4];
// codon c covers the sites frame + 3 c ..; NaN for a row whose plen is 0 or whose loglik (null: not looked at) is not finite
void launch_node_codons(const DevFamily& fam, int n, int n_codons, int frame, const double* table, const double* Q,
                        const int32_t* plen, const double* loglik, double* codons, double* change, hipStream_t stream);
// out[125][64]: the class (0 identical, 1 synonymous, 2 replacement, 3 the naive triple holds an N) of every (naive
// triple, node triple) pair, from the kernel's compile-time relation
void node_codon_classes(uint8_t* out);

// K12c alone (lh_substitutions.hip), behind launch_ancestral_front: the seed tip must be a child of v_0 under the sample's own
// schedule; slot 0's chain word is marked with which child it is, a failure leaves plen 0 and raises bit 1 of *err_flag.
void launch_sub_seed(int n, int T, int P, int seed_tip, const void* desc, int32_t* chain, int32_t* plen, int32_t* err_flag,
                     hipStream_t stream);

// K15 (lh_codon_edges.hip): exact joint posteriors of a codon at the two ends of every edge of a seed's lineage, folded to
// amino-acid replacements.
// K15b + K15m behind launch_ancestral_front and K12c: table[n][P][n_prune + 1][5][4][4], H_s[pattern][naive base b][a][c] =
// P(x_{v_s} = a, x_below = c | column of the pattern, naive base b) (padding slots 0, NaN for a sample without a valid path
// or seed: *err_flag raised, ws.plen 0); cond_edge[n][P][n_sites][5][4][4] (may be null) is the same per site.  Scratch:
// AncWs with `part` sized by cond_edge_ws_bytes.  Returns nonzero if the launch cannot be made (LDS tables, grid).
struct CondEdgeWsBytes {
  size_t part, table;  // per sample
};
CondEdgeWsBytes cond_edge_ws_bytes(int R, int n_prune, int P);
int launch_cond_edges(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                      const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                      const double* naive_prob, const int32_t* path, int P, int seed_tip, const AncWs& ws, double* table,
                      double* cond_edge, const int4* hdr, int32_t* err_flag, hipStream_t stream);
// K15 from Q[n][n_codons][125] and K15m's table; every output may be null (edge_load needs edge_change):
// codon_counts[n][n_codons][4], aa_counts[n][n_codons][21][21], seed_change[n][n_codons][3], edge_change[n][P+1][n_codons][3]
// (entry P the naive edge, padding slots 0), edge_load[n][P+1][2].  NaN for a row whose plen is 0 or whose loglik (null: not
// looked at) is not finite.
void launch_codon_edges(const DevFamily& fam, int n, int n_codons, int frame, int P, const double* table, const double* Q,
                        const int32_t* plen, const double* loglik, double* codon_counts, double* aa_counts,
                        double* seed_change, double* edge_change, double* edge_load, hipStream_t stream);
// out[64]: the symbol 0 .. 20 (position in "ACDEFGHIKLMNPQRSTVWY*") of every triple 16 x1 + 4 x2 + x3, the kernel's
// compile-time map
void codon_edge_symbols(uint8_t* out);

// K2a + K2b.  site_lik != null: emissions are assembled from K1's output (rate mix and naive
// correction; optionally written to em_out[n][C]); site_lik == null: emissions are taken from
// em_in[n][C].  K2a leaves the germline/padding emission products in gem[n][gem_size], their scaler
// counts in gcnt[n][3] and the junction columns' emissions in jem[n][n_jcols]; K2b runs the scaled
// forward sweep over them -> loglik[n] (+ optional forward rows and scaler counts).
// dxf[n][32], dxc[n]: scratch between the two K2b kernels of the pair form (lh_forward.hip).
// extended: the opt-in extended-range mode (include/linearham_amd.h, lh_family_set_extended_range); jrs[n][rows
// of both junctions] is then the K2a -> K2b hand-off of the junction rows' emission scaler counts.
// fam_dev: the device copy of fam (K2a reads the descriptor from memory instead of taking it by value).
// lem: K6b's optional request (lh_naive_probs.hip), with site_lik only: K2a also writes out[sample][j], j < lem.n, the
// log emission of u-column cols[j] less 256 log 2 per 2^-256 count in the extended-range mode.
struct LogEmRequest {
  const int32_t* cols = nullptr;
  int n = 0;
  double* out = nullptr;
};
void launch_forward(const DevFamily& fam, const DevFamily* fam_dev, int n, int R, const double* site_lik,
                    const int32_t* site_scal, const double* pi, const double* em_in, double* em_out, double* gem,
                    int32_t* gcnt, double* jem,
                    int32_t* jrs, double* dxf, int32_t* dxc, double* loglik, double* forward_out, int32_t* scaler_out,
                    bool extended, hipStream_t stream, const LogEmRequest& lem = LogEmRequest{});
size_t forward_lds_bytes(const DevFamily& fam);
// what the calling thread's last launch_forward ran: "emission<1,site,byte> cons=2 small=wave | vd2<4>+dj" -- K2a's
// instantiation <gene slots per thread, site likelihoods or caller's emissions, byte offsets or indices[, ext][, lem]>,
// the sets it runs in consensus form (bits as lh_family_consensus_sets), whether the small sets walk a wave each
// (fill_segments_wave) or on the whole block, and K2b's kernels: vd2<GA>+dj, vd<GA>+dj or junction<GA,GB>
const char* forward_last_form();
// samples per wave of the D-J kernel that launch_forward ran: 4 (junction_dj4_kernel), 2 (junction_dj_kernel), 0 (K2b not
// in the pair form)
int forward_last_dj_samples();
int forward_last_dj_waves();

// K8 (lh_viterbi.hip): the most probable state path of each sample, from K2a's hand-off buffers as launch_forward has just
// left them (gem, gcnt, jem, jrs) and the log-likelihoods K2b wrote.  states[n][states_per_sample] in K4's layout,
// log_path[n] = log P(data, best path | tree); a sample whose loglik is NaN or +inf: states -1, log_path NaN; no path of
// positive probability (loglik -inf): states -1, log_path -inf.  bp[n][viterbi_bp_bytes] is scratch (the back-pointers).
size_t viterbi_bp_bytes(const DevFamily& fam);
size_t viterbi_lds_bytes(const DevFamily& fam);
void launch_viterbi(const DevFamily& fam, const DevSampler* smp_dev, int n, const double* gem, const int32_t* gcnt,
                    const double* jem, const int32_t* jrs, const double* loglik, uint8_t* bp, int32_t* states,
                    double* log_path, bool extended, hipStream_t stream);
// log_prior[K] = log P_HMM of the paths states[K][states_per_sample] (their weight with every emission 1), one thread per
// path; a vector that is not a path of the model (an index out of range, a transition of probability 0) gets NaN and
// lowers *first_bad (which the caller sets to INT32_MAX) to its index.
void launch_path_prior(const DevFamily& fam, const DevSampler* smp_dev, int K, const int32_t* states, double* log_prior,
                       int32_t* first_bad, hipStream_t stream);

// Every environment switch of the device library in one place: hooks that tests/ use to push a family onto a kernel
// form another shape takes by itself (timing experiments are built from a copy of csrc/, tools/build_asm_variant.sh);
// none of them part of the C ABI.  Read once per process (the first call of debug_options(), lh_capi.hip); a switch that is not set leaves the
// product behaviour.
struct DebugOptions {
  int chunk = 49152;           // LH_CHUNK=<n>: tree samples per launch group (tests: several groups inside one small call)
  int host_sub = 12288;        // LH_HOST_SUB=<n>: tree samples per staging sub-chunk of lh_eval_batch (host pointers)
  // (LH_K2A_DIRECT -- K2a walks every gene factor by factor, no consensus form -- is a property of a family and is read
  // when one is created: upload_consensus, lh_capi.hip)
  int eval_split = 0;          // LH_EVAL_SPLIT=<1..8>: sub-batches of every launch group of an evaluation, K2 of one beside K1
                               // of the next on the handle's two streams (1: the single-stream path; 0, unset: the
                               // product's choice, eval_sub_batch in lh_capi.hip)
  bool k0_serial = false;      // LH_K0_SERIAL: an evaluation's K0a -> K0c -> K1 in a row on one stream, not K0a beside K0c on the
                               // handle's two streams (eval_device in lh_capi.hip; tests compare the two bit for bit)
  int eval_fwd_priority = -1;  // LH_EVAL_FWD_PRIORITY=<0|1>: the K2 stream at default / at the highest priority (-1, unset:
                               // the product's choice)
  bool k2b_no_pair = false;    // LH_K2B_NO_PAIR: K2b with one sample per wave
  bool k2b_vd_single = false;  // LH_K2B_VD_SINGLE: one sample per V-D wave
  bool k2b_dj_pair = false;    // LH_K2B_DJ_PAIR: two samples per D-J wave (junction_dj_kernel) where four would run
  bool sample_timing = false;  // LH_SAMPLE_TIMING: stage times of every lh_eval_sample_batch call on stderr
  bool k4_no_save = false;     // LH_K4_NO_SAVE: K4 forms a draw's weights again in each pass (the form of families wider than
                               // 256 genes, launch_sample) whatever the family's width
  int k1_tile_cap = 0;         // LH_K1_TILE_CAP=<sites>: small K1 tiles, so that small families run the multi-tile path
  bool k1_cxx_walk = false;    // LH_K1_CXX_WALK: the cherry-table form with its C++ walk instead of the assembly one
  bool k1_tables = false;      // LH_K1_TABLES: the cherry-table form for large trees too (which take the segmented register-stack form)
  bool k1_stack = false;       // LH_K1_STACK: the register-stack form for fused shapes (which take the cherry-table form by themselves)
  bool k1_no_tables = false;   // LH_K1_NO_TABLES: the cherry-table form's kernels without tables
  bool k1_segments = false;    // LH_K1_SEGMENTS: the segmented tip table (large trees) on small trees too
  int k1_seg_waves = 4;        // LH_K1_SEG_WAVES=<4|5>: register budget of the segmented kernels
  bool k1_no_fuse = false;     // LH_K1_NO_FUSE: one workgroup per (sample, rate)
  int codon_blocks = 2048;     // LH_CODON_BLOCKS=<n>: K9's workgroup cap (tests: a lane group walks several samples in a small call)
  int events_blocks = 1024;    // LH_EVENTS_BLOCKS=<n>: K10's workgroup cap (as LH_CODON_BLOCKS)
  int anc_out_mb = 4096;       // LH_ANC_OUT_MB=<n>: MiB of device copies of lh_eval_ancestral_batch's per-row outputs (host
                               // pointers) above which a batch is refused with the largest n (tests: the refusal on a small family)
  int edge_out_mb = 4096;      // LH_EDGE_OUT_MB=<n>: the same bound for lh_asr_edges_batch and lh_eval_edges_batch
  int anc_pairs = 0;           // LH_ANC_PAIRS=<n>: (row, candidate) pairs per sweep of lh_eval_ancestral_candidates_batch (0,
                               // unset: by memory; tests: a group cuts rows and candidates in a small call)
  int codon_edges_mb = 0;      // LH_CODON_EDGES_MB=<n>: MiB of scratch a launch group of lh_eval_codon_edges_batch and
                               // lh_asr_codon_edges_batch may take (0, unset: 8 GiB; tests: several groups in a small call)
  int collect_hash_bits = 64;  // LH_COLLECT_HASH_BITS=<n>: K6c's row hashes masked to n bits (tests: collisions common,
                               // the exact resolution runs; results unchanged)
};
const DebugOptions& debug_options();

}  // namespace lh
