/* linearham_amd.h -- C ABI of the MI355X phylo-HMM log-likelihood hot path.
 *
 * This is the drop-in boundary for linearham's per-tree-sample evaluation.  The reference has no
 * FFI layer; the seam these entry points replace is the libptpll `pt::pll::Partition` interface
 * plus the forward-pass free functions, as called from PhyloHMM/HMM member functions
 * (citations are file:line into matsengrp/linearham):
 *
 *   lh_family_create      <- PhyloHMM::InitializeXmsaStructs (src/PhyloHMM.cpp:45-89) +
 *                            HMM::InitializeTransition (src/HMM.cpp:190-246): everything that is
 *                            constant for one clonal family, uploaded once.
 *   lh_schedule_tree      <- pt::pll::GetVirtualRoot + the traversal order built inside
 *                            Partition::TraversalUpdate(root, FULL) (src/PhyloHMM.cpp:224-225).
 *   lh_eval_batch[_device]<- pll_compute_gamma_cats (src/PhyloHMM.cpp:425-426) +
 *                            PhyloHMM::InitializePhyloEmission (src/PhyloHMM.cpp:366-383: Partition
 *                            ctor, TraversalUpdate, LogLikelihood, naive correction, exp, the five
 *                            FillGermlinePaddingEmission and two FillJunctionEmission calls) +
 *                            HMM::LogLikelihood / RunForwardAlgorithm (src/HMM.cpp:254-287,345-354),
 *                            for a whole batch of RevBayes tree samples at once.
 *   lh_forward_batch      <- HMM::LogLikelihood on caller-supplied emissions (SimpleHMM,
 *                            src/SimpleHMM.cpp:26-39 + src/HMM.cpp:345-354).
 *   lh_asr_batch[_device] <- the per-tree body of scripts/run_bootstrap_asr_ess.R:48-104
 *   lh_asr_marginals_batch[_device]  the same step's exact per-node marginals along a lineage (no counterpart)
 *                            (phylomd::phylo.likelihood per rate, rate draw, phylomd::asr.sim).
 *
 * All functions return 0 on success and a nonzero status otherwise; lh_last_error() gives the
 * message (the C++ host wrapper turns it into std::runtime_error, mirroring
 * src/linearham.cpp:447-454).  Plain pointers and sizes only.  A handle is bound to the HIP device
 * that was current at lh_family_create and must be used by one host thread at a time.
 */
#ifndef LINEARHAM_AMD_H_
#define LINEARHAM_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH_ABI_VERSION 1

typedef struct lh_family lh_family; /* opaque: device-resident family constants + workspaces */

/* One running product per gene over its xMSA columns
 * (PhyloHMM::FillGermlinePaddingEmission, src/PhyloHMM.cpp:158-193).  Genes are in std::map
 * (sorted gene name) order, as `*_ggene_ranges_` is iterated (src/PhyloHMM.cpp:169). */
typedef struct {
  int32_t n_genes;
  const int32_t* offsets;   /* [n_genes + 1] into xmsa_inds */
  const int32_t* xmsa_inds; /* [offsets[n_genes]] */
} lh_segments;

/* One junction region (V-D, D-J or V-J) in structured form: exactly the nonzero pattern that
 * FillTransition (src/HMM.cpp:964-1089) writes into the dense germline->junction, junction->junction
 * and junction->germline matrices, indexed by (row = junction site, gene).  "left" genes are the
 * genes whose 3' end lies in the junction (V in V-D), "right" genes own the four NTI states and
 * their 5' germline positions (D in V-D).  A zero/-1 entry means "no such state at this row". */
typedef struct {
  int32_t n_rows;            /* W = junction sites */
  int32_t n_left;            /* nL */
  int32_t n_right;           /* nR */
  const double* enter_trans; /* [nL] transition[last germline-region idx] if a row-0 state exists */
  const double* enter_lo;    /* [nL] landing_out[last germline-region idx] */
  const double* left_trans;  /* [W][nL] transition[p-1] into the row-i state (row 0: 0) */
  const double* left_lo;     /* [W][nL] landing_out[p] of the row-i state */
  const int32_t* left_xmsa;  /* [W][nL] xMSA column of the row-i state, or -1 */
  const double* right_gp_nli;/* [nR][4] gene_prob * nti_landing_in[b] */
  const double* right_ntt;   /* [nR][4][4] nti_transition[b_from][b_to] */
  const double* right_nlo;   /* [W][nR][4] nti_landing_out[b_from][q] of the row-i germline state */
  const double* right_trans; /* [W][nR] transition[q-1] when rows i-1 and i both hold a state */
  const double* right_gp_li; /* [W][nR] gene_prob * landing_in[q] of the row-i germline state */
  const int32_t* right_xmsa; /* [W][nR] xMSA column of the row-i germline state, or -1 */
  const int32_t* nti_xmsa;   /* [W][nR][4] emission column of NTI base b of right gene r at row i
                              * (PhyloHMM: the same for every r; SimpleHMM: per-gene nti_emission) */
  const double* exit_nlo;    /* [nR][4] nti_landing_out[b][q0] * prod(in-region transitions) */
  const double* exit_trans;  /* [nR]    transition[q0-1] * prod (0 if no last-row state) */
  const double* exit_gp_li;  /* [nR]    gene_prob * landing_in[q0] * prod */
} lh_junction;

/* Everything that is constant for one clonal family (host pointers; copied to the device). */
typedef struct {
  int32_t abi_version;    /* LH_ABI_VERSION */
  int32_t has_d;          /* 1: igh (V-D and D-J junctions); 0: igk/igl (single V-J junction in `vd`) */
  int32_t n_seqs;         /* n: MSA rows = tips other than `naive` (0 => forward-only family) */
  int32_t n_sites;        /* L: MSA columns */
  const uint8_t* msa;     /* [n_seqs][L], A,C,G,T,N = 0..4 (HMM::msa_, src/HMM.cpp:71-83) */
  int32_t n_xmsa;         /* C: xMSA columns */
  const int32_t* xmsa_site;       /* [C] MSA site of each xMSA column */
  const uint8_t* xmsa_naive_base; /* [C] naive base 0..4 of each xMSA column (xmsa_ row 0) */
  lh_segments vpadding, vgerm, dgerm, jgerm, jpadding;
  const double* vgerm_gene_prob;     /* [nV] */
  const double* vpadding_transition; /* [nV] (HMM::vpadding_transition_) */
  const double* vgerm_trans_prod;    /* [nV] prod transition[germ_ind_start ... ) (src/HMM.cpp:310-313) */
  const double* jpadding_transition; /* [nJ] */
  lh_junction vd, dj;
} lh_family_desc;

/* Optional per-sample outputs of an evaluation (any pointer may be NULL). Host pointers for
 * lh_eval_batch / lh_forward_batch, device pointers for lh_eval_batch_device. */
typedef struct {
  double* rates;          /* [n][R]   discrete-Gamma category rates (PhyloHMM::sr_) */
  double* xmsa_emission;  /* [n][C]   PhyloHMM::xmsa_emission_ */
  double* forward;        /* [n][lh_forward_size()] compact forward arrays, see lh_forward_layout */
  int32_t* scaler_counts; /* [n][lh_scaler_size()]  vgerm, vd rows..., dgerm, dj rows..., jgerm */
} lh_eval_outputs;

const char* lh_last_error(void);
int lh_device_count(void);

/* Optional helpers for a host that wants its start-up and its copies off the critical path (no reference
 * counterpart): lh_warmup() initialises the HIP runtime and the current device's context (callable from a side
 * thread while the caller parses its inputs); lh_host_alloc / lh_host_free hand out page-locked host memory,
 * which the host-pointer entry points copy to and from at full PCIe rate (any host pointer is accepted). */
int lh_warmup(void);
/* Makes `device` (0 .. lh_device_count() - 1) the calling thread's current device (hipSetDevice, for hosts that do
 * not link the HIP runtime themselves).  A handle belongs to the device that is current when lh_family_create
 * runs, and every entry point that takes a handle switches to that device for its duration: a host with several
 * GPUs creates one handle per device and drives each from its own thread (tree samples dealt
 * i mod N; reference loop src/PhyloHMM.cpp:414-442). */
int lh_set_device(int32_t device);
void* lh_host_alloc(size_t bytes);
void lh_host_free(void* p);

int lh_family_create(const lh_family_desc* desc, lh_family** out);
void lh_family_destroy(lh_family* fam);

/* Number of doubles / ints per sample in lh_eval_outputs.forward / .scaler_counts.
 * forward layout: vgerm[nV] | vd rows i<W: left[nL], nti[nR][4], right[nR] | dgerm[nD] |
 *                 dj rows likewise | jgerm[nJ]   (dgerm/dj absent when has_d == 0). */
int64_t lh_forward_size(const lh_family* fam);
int64_t lh_scaler_size(const lh_family* fam);

/* What lh_family_create reduced the family to: the number of distinct alignment columns (site patterns;
 * the pruning kernel evaluates each once) and of distinct (naive base, pattern) pairs among the xMSA
 * columns (the emission kernels evaluate each once).  Either pointer may be NULL.  Results are per
 * xMSA column / per site all the same. */
int lh_family_info(const lh_family* fam, int32_t* n_patterns, int32_t* n_unique_columns);

/* Which germline / padding sets lh_family_create put into consensus form (bit 0 vpadding, 1 vgerm, 2 dgerm,
 * 3 jgerm, 4 jpadding): when the alleles of a set are site-aligned and alike, a gene's emission product
 * (FillGermlinePaddingEmission, src/PhyloHMM.cpp:158-193) is formed from the prefix products of the set's
 * consensus columns and the few factors where the gene departs from it, instead of factor by factor; values
 * agree to rounding, ScaleMatrix counts exactly.  Environment variable LH_K2A_DIRECT (read at create time)
 * turns the form off. */
int lh_family_consensus_sets(const lh_family* fam);

/* Diagnostic: the pruning-kernel form the handle's last evaluation ran, as "<kernel><stack depth, N-aware[, all rates
 * in one workgroup, assembly walk]>" -- e.g. "w6<3,false>", "seg4<4,true>", "ct6<16,false,false,true>" -- or "" before
 * the first one.  Which form a family takes is a function of its shape (tips, site patterns, rates, stack depth, N
 * inside alignment columns); the parity tests assert that every form is reached by a family that is compared with the
 * oracle.  The string lives as long as the handle and changes with the next evaluation. */
const char* lh_family_prune_form(const lh_family* fam);

/* Diagnostic: the K2 kernels the handle's last forward sweep ran (every entry point that evaluates, lh_forward_batch
 * included), as "emission<slots,site|caller,byte|index[,ext][,lem]> cons=<sets> small=wave|block | <K2b kernels>" --
 * e.g. "emission<1,site,byte> cons=2 small=wave | vd2<4>+dj" -- or "" before the first one.  K2a: gene slots per thread,
 * emissions from the site likelihoods or from the caller, column byte offsets or indices, extended-range mode, log
 * emissions requested; the sets it runs in consensus form (bits as lh_family_consensus_sets; 0 in the extended-range
 * mode) and whether the small sets (D, J, J padding) walk a wave each or on the whole workgroup -- both for a sample
 * whose emissions all lie in (0, 1]; any other sample walks every set factor by factor.  K2b: "vd2<GA>+dj" (two
 * samples per wave on both junctions), "vd<GA>+dj" (one sample per V-D wave: more than 256 V alleles) or
 * "junction<GA,GB>" (one wave per sample: light chains, more than 32 D or J alleles); GA, GB = 64-gene register
 * chunks of the V side and of the D / J sides.  Lives and changes like lh_family_prune_form's string. */
const char* lh_family_forward_form(const lh_family* fam);

/* Diagnostic: samples per wave of the D-J kernel in the handle's last forward sweep, where K2b ran in the pair form
 * ("vd2<GA>+dj" / "vd<GA>+dj"): 4 (one DPP row of 16 lanes per sample: at most 32 D and 16 J alleles, and LDS for four
 * emission slices per wave at the pair form's occupancy) or 2 (lanes 0-31 / 32-63); 0 for "junction<GA,GB>" and before
 * the first sweep.  Both layouts compute the same bits. */
int lh_family_forward_dj_samples(const lh_family* fam);

/* Diagnostic: waves per workgroup of that D-J kernel in the handle's last forward sweep: 4, 8 or 16 with four samples
 * per wave (the smallest workgroup whose four emission slices per wave keep the pair form's occupancy within 160 KB of
 * LDS per CU: it grows with the family's junction columns), the two-sample kernel's fixed workgroup otherwise; 0 for
 * "junction<GA,GB>" and before the first sweep. */
int lh_family_forward_dj_waves(const lh_family* fam);

/* Opt-in extended-range mode (default off = the reference's arithmetic, overflows included).  The reference
 * loses a tree sample in two places: exp(lnL - log pi) underflows to 0 when a column's likelihood is below
 * 1e-308 (src/PhyloHMM.cpp:237), and the 2^(256 d) equalisation of a region's emission products to the LARGEST
 * ScaleMatrix count overflows to inf when two alleles' counts differ by 4 or more (src/PhyloHMM.cpp:190-192;
 * acknowledged at scripts/run_bootstrap_asr_ess.R:37-39).  With the mode on, emissions are carried as
 * (value, 2^-256 count) pairs into the products and the junction rows, a region is equalised to its SMALLEST
 * count (negligible alleles underflow to 0 instead of likely ones overflowing), and a forward row is rescaled
 * by its largest entry instead of its smallest positive one.  Every such step is an exact power-of-two
 * rescaling, so the log-likelihood equals the default mode's wherever that is finite (tests: 1e-10) and stays
 * finite where the reference returns inf / NaN; the forward arrays and scaler counts of lh_eval_outputs are
 * then in this mode's scaling (value x 2^(-256 count) is what agrees), which is the documented divergence. */
int lh_family_set_extended_range(lh_family* fam, int enable);

/* ---- naive-sequence sampling on the device (HMM::SampleNaiveSequence's draws, src/HMM.cpp:323-341,358-431,
 * 1222-1353) ----
 * One junction in the unfused form FillTransition (src/HMM.cpp:964-1089) multiplies together, so that the
 * sampler's weights carry the bits of the reference's dense transition matrices.  [W][nL] / [W][nR] tables,
 * unpadded; "dense" = index in the junction's state vector (HMM::*_junction_state_strs_). */
typedef struct {
  int32_t n_rows, n_left, n_right, n_states;
  const int32_t* left_rows;    /* [nL] junction rows the gene has states on (rows 0 .. left_rows-1) */
  const int32_t* left_dense;   /* [nL] dense index of its row-0 state */
  const double* left_lo;       /* [W][nL] landing_out[p] of the row-i state */
  const double* left_trans;    /* [W][nL] transition[p-1] into the row-i state; row 0: out of the germline region */
  const double* enter_lo;      /* [nL] landing_out of the last germline-region position */
  const int32_t* right_dense;  /* [nR] dense index of the gene's NTI state A */
  const int32_t* right_first;  /* [nR] first row with a germline state of the gene (W: none) */
  const double* gene_prob;     /* [nR] */
  const double* nti_landing_in;  /* [nR][4] */
  const double* nti_transition;  /* [nR][4][4] from a to b */
  const double* nti_landing_out; /* [W][nR][4] into the row-i germline state */
  const double* landing_in;    /* [W][nR] of the row-i germline state */
  const double* right_trans;   /* [W][nR] transition[q-1] into the row-i germline state from the row before */
  const double* exit_nlo;      /* [nR][4] nti_landing_out[b][q0] * prod */
  const double* exit_trans;    /* [nR] transition[q0-1] * prod (0 if the gene has no last-row state) */
  const double* exit_li;       /* [nR] landing_in[q0] */
  const double* prod;          /* [nR] product of the in-region transitions (src/HMM.cpp:872-876) */
} lh_sampler_junction;

typedef struct {
  lh_sampler_junction vd, dj; /* dj unused when has_d == 0 */
} lh_sampler_desc;

/* Registers the sampler tables of a family (copied to the device).  Fails if the genes of a junction are not laid
 * out as two blocks in its state vector (all left genes before all right genes or the reverse: true of every IG
 * locus, whose gene names sort by segment). */
int lh_family_set_sampler(lh_family* fam, const lh_sampler_desc* desc);

/* std::mt19937 outputs one sample consumes (two per draw; a draw per junction row and per germline region with
 * more than one allele) and ints per sample in `states`. */
int32_t lh_sample_words(const lh_family* fam);
int32_t lh_sample_states(const lh_family* fam);

/* lh_eval_batch followed by the draws of SampleNaiveSequence for every sample, the forward arrays staying on the
 * device.  words [n][lh_sample_words()]: each sample's slice of the engine's output stream, in the order the
 * reference's loop would consume it.  states [n][lh_sample_states()]: J gene | D-J junction rows 0..W-1 | D gene |
 * V-D junction rows | V gene (light chains: J gene | V-J rows | V gene), as indices into the reference's state
 * vectors -- the values HMM::*_state_ind_samp(s)_ take.  rates [n][R] may be NULL. */
int lh_eval_sample_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                         const double* brlen, const double* er, const double* pi, const double* alpha,
                         int32_t num_rates, const uint32_t* words, double* loglik, double* rates, int32_t* states);

/* The same with every array resident on the handle's device (words, loglik, rates [may be NULL], states too);
 * enqueued on `hip_stream` without synchronising.  What a host calls that keeps its tree samples on the GPU. */
int lh_eval_sample_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha,
                                int32_t num_rates, const uint32_t* words, double* loglik, double* rates,
                                int32_t* states, void* hip_stream);

/* ---- exact posterior state marginals (K5: forward filtering / backward smoothing over the forward arrays) ----
 * Every member may be NULL.  log_offset is an input: lw_i = loglik_i - log_offset_i (0 when NULL), e.g. the
 * RevBayes log-likelihood of the row, so that w_i = exp(lw_i - max lw) is the row's importance weight
 * (scripts/run_bootstrap_asr_ess.R:29-32).
 *   loglik       [n]                   as lh_eval_batch
 *   posterior    [n][lh_forward_size]  posterior of every state, in the layout of lh_eval_outputs.forward:
 *                                      V genes | V-D rows x (left | NTI x 4 | right) | D genes | D-J rows | J genes;
 *                                      entries of states that do not exist are 0.  NaN for a sample whose loglik is
 *                                      not finite (an overflowed row in the active mode, or a rejected schedule)
 *   weighted_sum [lh_forward_size]     sum_i w_i posterior_i, in a fixed order; samples with w_i = 0 or a
 *                                      non-finite lw_i are left out
 *   weight_stats [3]                   max lw (-inf if none is finite), sum w_i, sum w_i^2
 * Batches combine exactly: rescale each one's sums by exp(max_b - max). */
typedef struct {
  const double* log_offset;
  double* loglik;
  double* posterior;
  double* weighted_sum;
  double* weight_stats;
} lh_posterior_outputs;

/* lh_eval_batch followed by K5.  Needs lh_family_set_sampler (the junction tables K5 reads).  Host pointers; a
 * malformed schedule fails the call as in lh_eval_sample_batch. */
int lh_eval_posterior_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                            const double* brlen, const double* er, const double* pi, const double* alpha,
                            int32_t num_rates, const lh_posterior_outputs* outs);

/* The same with every array (outs' members included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising.  A schedule K0c rejects gives that sample NaN posteriors, leaves it out of weighted_sum and
 * raises the handle's error word (lh_family_status). */
int lh_eval_posterior_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                   const double* brlen, const double* er, const double* pi, const double* alpha,
                                   int32_t num_rates, const lh_posterior_outputs* outs, void* hip_stream);

/* Time of K5 (smoothing and reduction) over the lh_eval_posterior_batch[_device] calls made while profiling was
 * enabled (HIP events on the launch stream); resets the counters. */
int lh_posterior_profile_read(lh_family* fam, double* ms_posterior, int64_t* n_launches);

/* ---- exact posterior probabilities of candidate naive sequences (K6) ----
 * Every state writes a fixed naive base on a fixed site and its emission depends on that pair only, so for a naive
 * sequence s and a tree sample t:  log P(s | data, t) = log P_HMM(s) + sum_i log E_t[s_i, i] - loglik_t, with
 * P_HMM(s) the probability of the state paths whose naive sequence is s (HMM::SampleNaiveSequence's naive_bases_,
 * src/HMM.cpp:358-431; padding writes N).  This is the exact form of the probabilities scripts/tabulate_naive_probs.py
 * counts from sampled naive sequences.
 *
 * Registers K candidates seqs[K][n_sites] (A,C,G,T,N = 0..4; 1 <= K <= 65536) on the handle, replacing any earlier
 * set, and computes log P_HMM(s_k) on the device: the forward sweep over the family's tables with indicator emissions
 * (K6a).  log_prior [K] (may be NULL) receives them; a candidate no state path produces gets -inf, which is a result,
 * not an error.  Fails for a byte above 4 or a family without an MSA. */
int lh_family_set_candidates(lh_family* fam, int32_t K, const uint8_t* seqs, double* log_prior);

/* Every member may be NULL.  log_offset is an input, as for K5: lw_i = loglik_i - log_offset_i.
 *   loglik       [n]     as lh_eval_batch
 *   log_cand     [n][K]  log P(s_k | data, t_i); NaN for a row whose loglik is not finite (an overflowed row in the
 *                        active mode, or a rejected schedule)
 *   weighted_sum [K]     sum_i w_i P(s_k | data, t_i) in a fixed order, rows with w_i = 0 or a non-finite lw_i left out;
 *                        divided by weight_stats[1] it is the posterior probability of s_k
 *   weight_stats [3]     max lw, sum w_i, sum w_i^2 (the same as lh_eval_posterior_batch's for the same rows)
 * Batches combine exactly: rescale each one's sums by exp(max_b - max). */
typedef struct {
  const double* log_offset;
  double* loglik;
  double* log_cand;
  double* weighted_sum;
  double* weight_stats;
} lh_candidate_outputs;

/* lh_eval_batch followed by K6b for the handle's candidates (lh_family_set_candidates first).  Host pointers; a
 * malformed schedule fails the call as in lh_eval_batch. */
int lh_eval_candidates_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                             const double* brlen, const double* er, const double* pi, const double* alpha,
                             int32_t num_rates, const lh_candidate_outputs* outs);

/* The same with every array (outs' members included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising.  A schedule K0c rejects gives that row NaN, leaves it out of the sums and raises the
 * handle's error word (lh_family_status). */
int lh_eval_candidates_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* alpha,
                                    int32_t num_rates, const lh_candidate_outputs* outs, void* hip_stream);

/* The number of candidates registered on the handle (0: none, or the last lh_family_set_candidates failed) and the
 * number of sites every candidate has (the alignment's).  Either pointer may be NULL. */
int lh_candidates_info(const lh_family* fam, int32_t* n_candidates, int32_t* n_sites);

/* Read-only layout of the registered candidate tables (all 0 when none are registered): n_var_sites = the sites where
 * the candidates do not all agree (V), n_lem = the u-columns K2a writes log emissions for, n_vlem = the first n_lem
 * entries that belong to variable sites (K6b's LDS row holds n_vlem doubles).  Any pointer may be NULL. */
int lh_candidates_layout(const lh_family* fam, int32_t* n_var_sites, int32_t* n_lem, int32_t* n_vlem);

/* Times while profiling was enabled (HIP events): ms[0] = K6a over the lh_family_set_candidates calls, ms[1] = K6b
 * (weights, scoring, reduction) over the evaluation calls, whose number goes to n_launches; resets the counters. */
int lh_candidates_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- naive sequences of sampled states (K6c) ----
 * The naive sequence a row of lh_eval_sample_batch's states stands for -- what HMM::ApplySampledStates writes into the
 * row's naive_seq -- as bytes seqs[n][n_sites] (A,C,G,T,N = 0..4; sites no state covers are N), and a 64-bit hash of
 * each: equal sequences have equal hashes, bit for bit on every run and batch split (LH_COLLECT_HASH_BITS=n masks them
 * to n bits, a test hook).  Needs lh_family_set_sampler and a family with an MSA.
 *
 * lh_eval_sample_batch followed by K6c: loglik [n] and hash [n]; states [n][lh_sample_states()] may be NULL.  The
 * batch's sequences stay in the handle's workspace for lh_draws_resolve / lh_draws_rows_read.  Host pointers. */
int lh_eval_draw_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                       const double* brlen, const double* er, const double* pi, const double* alpha,
                       int32_t num_rates, const uint32_t* words, double* loglik, uint64_t* hash, int32_t* states);

/* The same with every array resident on the handle's device (states may be NULL: the handle's workspace); enqueued on
 * `hip_stream` without synchronising. */
int lh_eval_draw_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                              const double* brlen, const double* er, const double* pi, const double* alpha,
                              int32_t num_rates, const uint32_t* words, double* loglik, uint64_t* hash,
                              int32_t* states, void* hip_stream);

/* K6c on caller-given states [n][lh_sample_states()] (host pointers): seqs [n][n_sites] and hash [n] (either may be
 * NULL).  The rows become the handle's last batch, as after lh_eval_draw_batch. */
int lh_naive_sequences(lh_family* fam, int32_t n, const int32_t* states, uint8_t* seqs, uint64_t* hash);

/* The handle's candidate store: rows of the last batch assigned to candidates.  cand [n] (n = the last batch's rows)
 * holds each row's candidate id, -1 for a row left out; ids at or above the store's count are new and must be
 * consecutive, each with a row of the batch: the first such row's bytes are appended to the store.  Every assigned row
 * is then compared with its candidate's stored bytes; the rows that differ (hash collisions) go to mismatch_rows [n]
 * in row order, their number to *n_mismatch.  Either output may be NULL. */
int lh_draws_resolve(lh_family* fam, int32_t n, const int32_t* cand, int32_t* n_mismatch, int32_t* mismatch_rows);
/* seqs [n_rows][n_sites]: the bytes of rows[k] of the last batch. */
int lh_draws_rows_read(lh_family* fam, int32_t n_rows, const int32_t* rows, uint8_t* seqs);
/* *K: the number of stored candidates; seqs [K][n_sites] (may be NULL) their bytes. */
int lh_draws_candidates_read(lh_family* fam, int32_t* K, uint8_t* seqs);
/* Empties the candidate store. */
int lh_draws_reset(lh_family* fam);
/* Time of K6c (assembly and hash) over the draw / lh_naive_sequences calls made while profiling was enabled (HIP
 * events); resets the counters. */
int lh_collect_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- the lineage of a seed sequence (K7) ----
 * The lineage of tree sample i is the chain of inner nodes from the seed tip's parent up to the tree's root (naive's
 * neighbour): path[i][0..P) in lh_schedule_tree numbering (T + k), padded with -1; P = the batch's longest chain.  Its
 * slots are s < P: row anc[i][path[i][s] - T][0..L) of the sampled states; s = P: the sample's naive sequence.  A flat
 * slot is i * (P + 1) + s (with lh_eval_lineage_batch's draws: (i * draws + d) * (P + 1) + s).  Per slot the kernel writes a 64-bit hash of the bases and one of their translation
 * (standard code, frame 0, truncated to whole codons, stop = '*', a codon with N = the one symbol all its resolutions
 * give, else 'X').  Hash bits depend on the sequence alone -- a naive sequence gets lh_naive_sequences' hash -- and
 * LH_COLLECT_HASH_BITS masks them too.  Padding slots get LH_LINEAGE_PAD_HASH; a sample whose (device-resident)
 * schedule the sampling kernel refused gets all-ones in every slot, and the handle's error word is raised.
 *
 * lh_asr_batch followed by K7 (host pointers): lh_asr_batch's inputs and random numbers, path [n][P]; nt_hash, aa_hash
 * [n][P+1].  The sampled states are not copied back: they stay in the handle's workspace, whole, for
 * lh_lineage_resolve / lh_lineage_rows_read, so a batch with more than 1 GiB of them is refused (the message names
 * the largest n).  The next lh_asr_batch or lh_lineage_batch on the handle overwrites them. */
#define LH_LINEAGE_PAD_HASH 0ull
int lh_lineage_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                     const double* brlen, const double* er, const double* pi, const double* rates, int32_t num_rates,
                     const uint8_t* naive, uint64_t seed, uint64_t first_sample, const int32_t* path,
                     int32_t path_len, uint64_t* nt_hash, uint64_t* aa_hash);

/* K7 alone, every array resident on the handle's device (anc [n][T-2][L] as lh_asr_batch_device leaves it, naive
 * [n][L], path [n][P]); enqueued on `hip_stream` without synchronising.  Path entries outside T .. 2T-3 count as
 * padding.  The arrays become the handle's last lineage batch and must stay as they are while it is resolved. */
int lh_lineage_collect_device(lh_family* fam, int32_t n, int32_t n_tips, const uint8_t* anc, const uint8_t* naive,
                              const int32_t* path, int32_t path_len, uint64_t* nt_hash, uint64_t* aa_hash,
                              void* hip_stream);

/* The handle's lineage store: slots of the last lineage batch assigned to sequences.  ids [n_slots] (n_slots = the
 * last batch's n * (P + 1), flat slot order) holds each slot's sequence id, -1 for a slot left out (padding); ids at
 * or above the store's count are new and must be consecutive, each with a slot of the batch: the first such slot's
 * bases are appended to the store.  Every assigned slot is then compared with its id's stored bases; the slots that
 * differ (hash collisions) go to mismatch_slots [n_slots] in order, their number to *n_mismatch.  Either may be NULL. */
int lh_lineage_resolve(lh_family* fam, int32_t n_slots, const int32_t* ids, int32_t* n_mismatch,
                       int32_t* mismatch_slots);
/* seqs [n_slots][n_sites]: the bases of flat slots slots[k] of the last lineage batch (padding slots read as N). */
int lh_lineage_rows_read(lh_family* fam, int32_t n_slots, const int32_t* slots, uint8_t* seqs);
/* *K: the number of stored sequences; seqs [count][n_sites] (may be NULL) the bases of ids first .. first+count-1. */
int lh_lineage_store_read(lh_family* fam, int32_t first, int32_t count, int32_t* K, uint8_t* seqs);
/* Empties the lineage store and forgets the last batch. */
int lh_lineage_reset(lh_family* fam);
/* Time of K7 over the lineage calls made while profiling was enabled (HIP events); resets the counters. */
int lh_lineage_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- the chain: evaluation, naive draw, ancestral draws and lineage hashes in one pass ----
 * What lh_eval_batch (rates), lh_eval_draw_batch, lh_draws_rows_read and lh_lineage_batch give when composed, without the
 * host round trips and with one pruning launch per group: K0a (rates kept on the device), K0c, K1 once with unmixed rate
 * planes, K2 on those planes, K4 with `words`, K6c (naive bases and hash), K3 with `draws` ancestral draws per row reading
 * K6c's bases and K0a's full-precision rates, K7.  Draw d of row i is virtual sample i * draws + d; its Philox sample
 * number is first_sample + i + (d << 32), so draw 0 is lh_lineage_batch's draw (with draws > 1, first_sample + n must not
 * exceed 2^32).  The flat lineage slot is ((i * draws) + d) * (P + 1) + s; slot s = P is the row's naive sequence, the same
 * for every d, with lh_naive_sequences' hash.  The batch becomes the handle's last lineage batch (lh_lineage_resolve,
 * _rows_read and _store_read work on its n * draws * (P + 1) slots) and its last draw batch.  Refused: what
 * lh_lineage_batch and lh_eval_draw_batch refuse (the 1 GiB bound on resident sampled states applies to n * draws samples;
 * the message names the largest n), and draws outside 1 .. 64.  A row whose log-likelihood is not finite has unspecified
 * hashes (its naive bytes are still 0 .. 4); a row whose schedule is rejected has a NaN log-likelihood and all-ones hashes
 * in all its draws.  Honours lh_family_set_extended_range. */
typedef struct {
  double* loglik;       /* [n]                       required */
  double* rates;        /* [n][R]                    or NULL  */
  int32_t* states;      /* [n][lh_sample_states()]   or NULL  */
  uint8_t* naive;       /* [n][L]  A,C,G,T,N = 0..4  or NULL  */
  uint64_t* naive_hash; /* [n]                       or NULL  */
  uint64_t* nt_hash;    /* [n][draws][P+1]           required */
  uint64_t* aa_hash;    /* [n][draws][P+1]           required */
} lh_lineage_eval_outputs;

int lh_eval_lineage_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                          const double* brlen, const double* er, const double* pi, const double* alpha,
                          int32_t num_rates, const uint32_t* words, uint64_t seed, uint64_t first_sample, int32_t draws,
                          const int32_t* path, int32_t path_len, const lh_lineage_eval_outputs* outs);

/* The same with every array (outs' members included) resident on the handle's device; enqueued on `hip_stream` without
 * synchronising.  `path` must stay as it is while the batch is resolved. */
int lh_eval_lineage_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                 const double* brlen, const double* er, const double* pi, const double* alpha,
                                 int32_t num_rates, const uint32_t* words, uint64_t seed, uint64_t first_sample,
                                 int32_t draws, const int32_t* path, int32_t path_len,
                                 const lh_lineage_eval_outputs* outs, void* hip_stream);

/* Times of the chain's stages over the lh_eval_lineage_batch[_device] calls made while profiling was enabled (HIP events):
 * ms[5] = K0a, K0c + K1, K2 + K4 + K6c, K3, K7; resets the counters. */
int lh_lineage_eval_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* Tree in rooted-at-naive form: tips are nodes 0..T-1 (0 = `naive`, i = MSA row i-1), inner nodes
 * T..2T-3.  children[2*(v-T)+{0,1}] are the two children of inner node v when the tree is rooted at
 * `root`, the inner node adjacent to `naive`.  Writes the kernel's post-order schedule:
 * ops[4*k+{0..3}] for k < T-2 (the last op computes the root; word 0 = kind | flags | running matrix count,
 * words 1-2 = children, word 3 = stack slot: an internal format, validated by lh_eval_batch).  *max_depth receives the number of
 * stack slots the schedule needs.  Pure host integer work. */
int lh_schedule_tree(int32_t n_tips, const int32_t* children, int32_t root, int32_t* ops,
                     int32_t* max_depth);

/* Evaluate n tree samples (host pointers).
 *   ops    [n][T-2][4]  schedules from lh_schedule_tree
 *   brlen  [n][2T-2]    branch length above each node (root entry ignored)
 *   er [n][6] (AC,AG,AT,CG,CT,GT), pi [n][4], alpha [n]; num_rates = R
 *   loglik [n]          HMM::LogLikelihood() per sample */
int lh_eval_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                  const double* brlen, const double* er, const double* pi, const double* alpha,
                  int32_t num_rates, double* loglik, const lh_eval_outputs* outs);

/* Same with every array already resident on the handle's device; enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream) without synchronising.  Device-resident schedules are not trusted: a
 * kernel (K0c) checks every op on the device before anything is indexed with it; a malformed schedule leaves NaN
 * in that sample's results and raises the handle's error word, which lh_family_status reports.  (The reference
 * checks nothing here: src/PhyloHMM.cpp:421 uses the parsed tree unchecked.) */
int lh_eval_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth,
                         const int32_t* ops, const double* brlen, const double* er, const double* pi,
                         const double* alpha, int32_t num_rates, double* loglik,
                         const lh_eval_outputs* outs, void* hip_stream);

/* Synchronises the handle's device, then reports and clears its asynchronous error state: nonzero (message in
 * lh_last_error) if a launch since the previous call met a malformed schedule, a lineage path that is not a chain, or
 * (the `_at` entry points of K13 and K14) a slot outside its path: that message names the first such row of its call and
 * takes the place of the path's.  The host-pointer entry points call it themselves before they return. */
int lh_family_status(lh_family* fam);

/* Forward pass only, on caller-supplied per-column emissions em[n][C] (host pointers). */
int lh_forward_batch(lh_family* fam, int32_t n, const double* em, double* loglik,
                     const lh_eval_outputs* outs);

/* K4 on caller-supplied per-column emissions em[n][C] (host pointers), beside lh_forward_batch: the forward sweep with the
 * forward arrays kept on the device, then the draws of lh_eval_sample_batch from words [n][lh_sample_words()] into states
 * [n][lh_sample_states()] (its layout and encoding).  loglik [n] may be NULL; outs may be NULL, and of its members forward
 * and scaler_counts are written: the arrays K4 drew from.  Honours lh_family_set_extended_range; needs
 * lh_family_set_sampler. */
int lh_sample_forward_batch(lh_family* fam, int32_t n, const double* em, const uint32_t* words, double* loglik,
                            int32_t* states, const lh_eval_outputs* outs);

/* K5 on caller-supplied per-column emissions em[n][C] (host pointers): loglik [n] and posterior [n][lh_forward_size()] as
 * lh_posterior_outputs describes them (either may be NULL).  The twin of lh_viterbi_forward_batch; honours
 * lh_family_set_extended_range; needs lh_family_set_sampler. */
int lh_posterior_forward_batch(lh_family* fam, int32_t n, const double* em, double* loglik, double* posterior);

/* Ancestral-sequence sampling (scripts/run_bootstrap_asr_ess.R:48-104) for n tree samples of the family:
 * per alignment site, draw a rate category with the likelihoods of the column (naive base on the `naive`
 * tip) on the rate-scaled trees, then draw the states of all inner nodes jointly given the tips on the
 * chosen tree.
 *   ops, brlen, er, pi   as for lh_eval_batch
 *   rates  [n][R]        the site rates of the sample (the sr[] columns of the pipeline output)
 *   naive  [n][L]        the sample's NaiveSequence, A,C,G,T,N = 0..4
 *   seed, first_sample   random numbers are Philox4x32-10 with key = seed and counter =
 *                        (site, draw, first_sample + i): draw 0 = rate category, 1 = root (naive's
 *                        neighbour), 2 + (v - T) = inner node v; a draw picks the first category whose
 *                        running weight sum exceeds u * total
 *   anc    [n][T-2][L]   state 0..3 of inner node T + i (lh_schedule_tree numbering) at every site
 *   rate_choice [n][L]   drawn category per site (may be NULL)
 * A sample whose (device-resident) schedule is rejected gets 0xff in every byte of its anc and rate_choice rows --
 * bytes have no NaN -- and raises the handle's error word (lh_family_status).
 * The extra root node that ape::root(..., resolve.root = TRUE) puts on the naive branch (:53) lies at
 * distance 0 from naive's neighbour and has that node's state.  Tips keep their observed characters. */
int lh_asr_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                 const double* brlen, const double* er, const double* pi, const double* rates,
                 int32_t num_rates, const uint8_t* naive, uint64_t seed, uint64_t first_sample,
                 uint8_t* anc, uint8_t* rate_choice);

/* Same with every array resident on the handle's device; enqueued on `hip_stream` without synchronising. */
int lh_asr_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                        const double* brlen, const double* er, const double* pi, const double* rates,
                        int32_t num_rates, const uint8_t* naive, uint64_t seed, uint64_t first_sample,
                        uint8_t* anc, uint8_t* rate_choice, void* hip_stream);

/* ---- K11: exact ancestral-state marginals along a seed's lineage ----
 * What lh_asr_batch draws and the lineage tables count, as probabilities: per node of a lineage path and alignment site
 * the posterior of the node's state, marginalised over the rate category and over the naive base,
 *   marg[s][j][c] = sum_b naive_prob[j][b] sum_r [lik_r(j, b) / sum_r' lik_r'(j, b)] P(x_{v_s, j} = c | column j, naive_j = b, rate r)
 * from one upward pass of the pruning recursion and one downward pass along the path (no random numbers).
 *   ops, brlen, er, pi, rates   as for lh_asr_batch
 *   naive_prob [n][L][5]  the distribution of the naive base at every site (A,C,G,T,N; rows sum to 1).  A one-hot row
 *                         conditions on a fixed naive sequence: the tables are then the distributions lh_asr_batch draws
 *                         from.  A base of probability 0 contributes nothing; a NaN row gives NaN at that site.
 *   path  [n][P]          the lineage of a tip in lh_lineage_batch's convention: slot 0 the tip's parent, every entry
 *                         the child of the next, the last one the root (naive's neighbour); entries outside T .. 2T-3
 *                         (-1) are padding and come only after them.  1 <= P <= T - 2.
 *   marg  [n][P][L][4]    the tables (may be NULL); a padding slot's tables are 0
 *   rate_post [n][L][R]   the posterior of the site's rate category (may be NULL)
 * The path is checked against the sample's own schedule.  The host-pointer form refuses a batch with a path that is not
 * such a chain, as it refuses malformed schedules.  The device form gives that sample NaN in its whole marg row and raises
 * the handle's error word (lh_family_status), as for a rejected schedule; no index is formed from an unchecked entry.
 * The same sample gives the same bits whatever the batch around it. */
int lh_asr_marginals_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                           const double* brlen, const double* er, const double* pi, const double* rates,
                           int32_t num_rates, const double* naive_prob, const int32_t* path, int32_t path_len,
                           double* marg, double* rate_post);

/* Same with every array resident on the handle's device; enqueued on `hip_stream` without synchronising. */
int lh_asr_marginals_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                  const double* brlen, const double* er, const double* pi, const double* rates,
                                  int32_t num_rates, const double* naive_prob, const int32_t* path, int32_t path_len,
                                  double* marg, double* rate_post, void* hip_stream);

/* The evaluation with the exact ancestral marginals behind it: lh_eval_posterior_batch's inputs plus path, and per tree
 * sample K0-K2 (one unmixed K1 serves the forward sweep and K11), K5's posterior on the forward arrays, its push-forward
 * onto the naive base of every site, and lh_asr_marginals_batch fed that distribution and the sample's rates.  Needs
 * lh_family_set_sampler; honours lh_family_set_extended_range.  Every member may be NULL:
 *   log_offset   [n]           (input) as in lh_posterior_outputs
 *   loglik       [n]
 *   site_base    [n][L][5]     posterior of the naive base (A,C,G,T,N); what no state writes stays N; NaN for a row
 *                              without a posterior (non-finite log-likelihood, rejected schedule)
 *   marg         [n][P][L][4]  as lh_asr_marginals_batch
 *   rate_post    [n][L][R]
 *   weighted_sum [2][L][4]     sum_i w_i marg_i of the two slots that mean the same in every tree: [0] the seed's parent
 *                              (slot 0), [1] the MRCA (the sample's last slot); w_i = exp(loglik_i - log_offset_i - max)
 *   weighted_rate [L][R]       sum_i w_i rate_post_i
 *   weight_stats [3]           max, sum w, sum w^2 as in lh_posterior_outputs
 * The sums run in sample order (K5's slab scheme: no atomics, bit-stable); rows with w = 0 or a non-finite
 * log-likelihood are left out of the sums and of the statistics, so batches combine exactly as
 * lh_eval_posterior_batch's do.  So are rows without a valid path (device form) whenever the call looks at the paths,
 * which it does when marg or weighted_sum is asked for; a call for weighted_rate and weight_stats alone forms neither
 * and weighs every row.  The host-pointer form refuses a batch whose device copies of site_base, marg and rate_post
 * would exceed 4 GiB, naming the largest n. */
typedef struct lh_ancestral_outputs {
  const double* log_offset;
  double* loglik;
  double* site_base;
  double* marg;
  double* rate_post;
  double* weighted_sum;
  double* weighted_rate;
  double* weight_stats;
} lh_ancestral_outputs;

int lh_eval_ancestral_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                            const double* brlen, const double* er, const double* pi, const double* alpha,
                            int32_t num_rates, const int32_t* path, int32_t path_len, const lh_ancestral_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_eval_ancestral_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                   const double* brlen, const double* er, const double* pi, const double* alpha,
                                   int32_t num_rates, const int32_t* path, int32_t path_len,
                                   const lh_ancestral_outputs* outs, void* hip_stream);

/* Times of K11 over the launches made while profiling was enabled (HIP events on the launch stream), ms[3]: the
 * naive-base posteriors, the marginals kernel with its rate weights, path check and rate combination, the weighted
 * reduction (lh_asr_marginals_batch runs the second only); resets the counters. */
int lh_ancestral_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K12: exact substitution posteriors along the edges of a seed's lineage ----
 * The two ends of an edge are strongly dependent, so which substitution happened on which edge is not the product of two
 * of K11's per-node tables.  For a sample with path v_0 (the seed's parent) .. v_{len-1} (the root, naive's neighbour) the
 * lineage of seed tip u has len + 1 edges; every table is indexed [ancestor state][descendant state], naive the oldest node.
 *   lh_asr_marginals_batch's inputs, plus
 *   seed_tip              the seed's tip id, 1 .. T-1, one value per call; it must be a child of path[i][0] in every sample
 * and an output struct, every member of which may be NULL:
 *   edge [n][P][L][4][4]      edge[s][j][a][c] = P(x_{v_s, j} = a, x_{below, j} = c | data), below = v_{s-1} for s >= 1 and
 *                             the seed tip for s = 0 (an N seed tip: what the model says about the unobserved base).
 *                             A padding slot's tables are 0.
 *   naive_edge [n][L][5][4]   P(naive_j = b, x_{root, j} = i | data), b over A,C,G,T,N
 *   chain_counts [n][L][4][4] naive_edge (rows b < 4) + sum_s edge[s]: the expected number of lineage edges, naive to
 *                             seed, on which site j goes from a to c.  An off-diagonal cell counts edges whose ends are a
 *                             and c, not substitutions inside a branch.  The cells of a site sum to len + 1 - q_j(N).
 *   edge_load [n][P+1]        the expected number of sites whose two ends differ on the edge: [s] slot s (padding slots 0),
 *                             [P] the naive edge (rows b < 4)
 *   rate_post [n][L][R]       as lh_asr_marginals_batch
 * Margins: sum_c edge[s] = marg[s], sum_a edge[s] = marg[s-1], sum_i naive_edge = naive_prob, sum_b naive_edge = marg[len-1].
 * chain_counts, edge_load and naive_edge have the same bits whether or not edge is asked for (without it a leaner kernel
 * runs), and the same sample gives the same bits whatever the batch around it: every sum runs in a fixed order.
 * The host-pointer form refuses a batch whose device copies of the per-row outputs would exceed 4 GiB, naming the largest n,
 * a seed_tip outside 1 .. T-1, a path that is not a chain (as lh_asr_marginals_batch) and a
 * seed_tip that is not a child of path[i][0].  The device form refuses only the first; for the other two the sample gets NaN
 * in all its rows and the handle's error word is raised (bit 1), and no index is formed from an unchecked value. */
typedef struct lh_edges_outputs {
  double* edge;
  double* naive_edge;
  double* chain_counts;
  double* edge_load;
  double* rate_post;
} lh_edges_outputs;

int lh_asr_edges_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                       const double* brlen, const double* er, const double* pi, const double* rates, int32_t num_rates,
                       const double* naive_prob, const int32_t* path, int32_t path_len, int32_t seed_tip,
                       const lh_edges_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_asr_edges_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                              const double* brlen, const double* er, const double* pi, const double* rates,
                              int32_t num_rates, const double* naive_prob, const int32_t* path, int32_t path_len,
                              int32_t seed_tip, const lh_edges_outputs* outs, void* hip_stream);

/* The evaluation with K12 behind it, K11's chain: lh_eval_ancestral_batch's inputs plus seed_tip, and per tree sample K0-K2
 * (one unmixed K1 serves the forward sweep and K12), K5's posterior on the forward arrays, its push-forward onto the naive
 * base of every site, and lh_asr_edges_batch fed that distribution and the sample's rates.  Needs lh_family_set_sampler;
 * honours lh_family_set_extended_range.  Every member may be NULL:
 *   log_offset, loglik, site_base            as in lh_ancestral_outputs
 *   edge, naive_edge, chain_counts, edge_load, rate_post   as in lh_edges_outputs
 *   seed_edge [n][L][4][4]                   slot 0 of edge, the edge above the seed tip, without the other slots
 *   weighted_counts [L][4][4]                sum_i w_i chain_counts_i,  w_i = exp(loglik_i - log_offset_i - max)
 *   weighted_seed_edge [L][4][4]             sum_i w_i seed_edge_i
 *   weighted_naive_edge [L][5][4]            sum_i w_i naive_edge_i
 *   weight_stats [3]                         max, sum w, sum w^2 as in lh_posterior_outputs
 * The three weighted tables are of quantities that mean the same in every tree.  The sums run in sample order (K5's slab
 * scheme: no atomics, bit-stable); rows with w = 0 or a non-finite log-likelihood are left out, and so are rows without a
 * valid path (device form) whenever a table is asked for, so batches combine exactly as lh_eval_posterior_batch's do.
 * Without edge the lean kernel runs.  The host-pointer form refuses as lh_asr_edges_batch does, and a batch whose device
 * copies of the per-row outputs would exceed 4 GiB, naming the largest n. */
typedef struct lh_eval_edges_outputs {
  const double* log_offset;
  double* loglik;
  double* site_base;
  double* edge;
  double* naive_edge;
  double* chain_counts;
  double* seed_edge;
  double* edge_load;
  double* rate_post;
  double* weighted_counts;
  double* weighted_seed_edge;
  double* weighted_naive_edge;
  double* weight_stats;
} lh_eval_edges_outputs;

int lh_eval_edges_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                        const double* brlen, const double* er, const double* pi, const double* alpha, int32_t num_rates,
                        const int32_t* path, int32_t path_len, int32_t seed_tip, const lh_eval_edges_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_eval_edges_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                               const double* brlen, const double* er, const double* pi, const double* alpha,
                               int32_t num_rates, const int32_t* path, int32_t path_len, int32_t seed_tip,
                               const lh_eval_edges_outputs* outs, void* hip_stream);

/* Times of K12 over the launches made while profiling was enabled (HIP events on the launch stream), ms[3]: the
 * naive-base posteriors (lh_eval_edges_batch only), the edge kernel with its rate weights, path and seed checks and rate
 * combination, the weighted reduction (lh_eval_edges_batch only); resets the counters. */
int lh_edges_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K13: exact posterior probabilities of candidate ancestral sequences ----
 * K11's per-site tables cannot give the probability of a whole sequence at a node of the lineage: the node's sites are
 * coupled through the naive sequence, whose sites the HMM couples.  For a tree sample t, a node v and a candidate x
 *   P(X_v = x | data, t) = sum_paths prior(path) prod_j E_t[b_j, j] G_t[j][b_j][x_j] / P(data | t),
 * b_j the naive base the path writes on site j, E_t the xMSA emission and G_t[j][b][c] = P(x_{v,j} = c | column j,
 * naive_j = b), K11's table for a one-hot naive distribution.  Every (row, candidate) pair takes one forward sweep.
 *
 * lh_family_set_ancestral_candidates registers K candidates (1 <= K <= 65536) of n_sites bytes each: 0..3 = A, C, G, T,
 * 4 = the site is left open (any base).  They are kept apart from lh_family_set_candidates' naive candidates, which stay
 * registered.  A call that fails leaves no candidates.  Refused for a family without an MSA or without the constrained
 * forward sweep (as lh_family_set_candidates). */
int lh_family_set_ancestral_candidates(lh_family* fam, int32_t K, const uint8_t* seqs);

/* (candidates registered, sites each has) */
int lh_ancestral_candidates_info(const lh_family* fam, int32_t* n_candidates, int32_t* n_sites);

/* The evaluation with K13 behind it: lh_eval_ancestral_batch's inputs plus node, 0 = the seed's parent (slot 0 of the
 * path), 1 = the MRCA (the sample's last slot).  Needs lh_family_set_sampler and lh_family_set_ancestral_candidates; a handle
 * in the extended-range mode is refused (the candidates' sweeps run on plain doubles).  Every member may be NULL:
 *   log_offset   [n]           (input) as in lh_posterior_outputs
 *   loglik       [n]
 *   cond         [n][L][5][4]  G: P(x_{node,j} = c | column j, naive_j = b), b = A,C,G,T,N
 *   log_cand     [n][K]        log P(X_node = x_k | data, t_i); an all-open candidate gives exactly 0
 *   weighted_sum [K]           sum_i w_i P(x_k | data, t_i), w_i = exp(loglik_i - log_offset_i - max)
 *   weight_stats [3]           max, sum w, sum w^2 as in lh_posterior_outputs
 * A row with a non-finite log-likelihood, a rejected schedule or (device form) a bad path gets NaN in cond and log_cand
 * and no weight; the path is checked, the error word raised and the host-pointer form's device copies of cond and
 * log_cand bounded (4 GiB) as for lh_eval_ancestral_batch.  The sums run in sample order (K5's slab scheme); the same
 * sample gives the same bits whatever the batch around it. */
typedef struct lh_ancestral_candidates_outputs {
  const double* log_offset;
  double* loglik;
  double* cond;
  double* log_cand;
  double* weighted_sum;
  double* weight_stats;
} lh_ancestral_candidates_outputs;

int lh_eval_ancestral_candidates_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                       const double* brlen, const double* er, const double* pi, const double* alpha,
                                       int32_t num_rates, const int32_t* path, int32_t path_len, int32_t node,
                                       const lh_ancestral_candidates_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_eval_ancestral_candidates_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth,
                                              const int32_t* ops, const double* brlen, const double* er, const double* pi,
                                              const double* alpha, int32_t num_rates, const int32_t* path, int32_t path_len,
                                              int32_t node, const lh_ancestral_candidates_outputs* outs, void* hip_stream);

/* The same at a node per row: slot[n] names, for every sample, the entry of its own path the tables are formed at,
 * 0 <= slot[i] < the length of path i (0 is the seed's parent, the last one the MRCA; both give the bits of node 0 and 1).
 * The use is a node that means the same in every tree sample though its slot does not: the most recent common ancestor of
 * the seed and other tips (lhh_clade_slot gives the slot).  K13b's walk down the lineage stops at the row's slot.  The
 * host-pointer form refuses a batch with a slot outside its path, naming the row; the device form gives that row NaN and
 * no weight and raises a bit of its own in the handle's error word (lh_family_status names the first such row).
 * Everything else, the refusal of an extended-range handle included, is lh_eval_ancestral_candidates_batch's. */
int lh_eval_ancestral_candidates_at_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                          const double* brlen, const double* er, const double* pi, const double* alpha,
                                          int32_t num_rates, const int32_t* path, int32_t path_len,
                                          const int32_t* slot /* [n] */, const lh_ancestral_candidates_outputs* outs);
int lh_eval_ancestral_candidates_at_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth,
                                                 const int32_t* ops, const double* brlen, const double* er, const double* pi,
                                                 const double* alpha, int32_t num_rates, const int32_t* path,
                                                 int32_t path_len, const int32_t* slot /* [n] */,
                                                 const lh_ancestral_candidates_outputs* outs, void* hip_stream);

/* Times of K13 over the launches made while profiling was enabled (HIP events on the launch stream), ms[3]: the tables
 * (rate weights, path check, K13b, rate combination), the pair emissions with their sweeps, the weighted reduction; resets
 * the counters. */
int lh_ancestral_candidates_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K14: exact codon marginals of a node of a seed's lineage ----
 * The three bases of a node's codon are coupled through the naive codon, whose bases the HMM couples in the junctions, so
 * K11's per-site tables do not give the node's codon.  Given the naive base of a site the node's base there is independent
 * of everything else, so with K9's naive codon posterior Q (125 entries, 25 b1 + 5 b2 + b3 over A,C,G,T,N) and K13's G
 *   T_t[c][x1 x2 x3] = sum_b Q_t[c][b1 b2 b3] G_t[j1][b1][x1] G_t[j2][b2][x2] G_t[j3][b3][x3]
 * for codon c over the sites j1, j2, j3 = frame + 3 c .. of lh_family_set_codons' frame; the node triple is indexed
 * 16 x1 + 4 x2 + x3 over A,C,G,T.  change folds the joint P(b, x) per codon:
 *   [0] the naive triple has no N and x equals it        [1] no N, x != b, the same translation
 *   [2] no N, a different translation                    [3] the naive triple holds an N
 * (the standard code, the stop codons a symbol of their own); the four sum to 1.
 *
 * The evaluation with K14 behind it: lh_eval_ancestral_candidates_batch's inputs (node 0 = the seed's parent, 1 = the
 * MRCA).  Needs lh_family_set_sampler and lh_family_set_codons, no candidates; the extended-range mode is honoured.  With
 * C = n_codons of lh_codon_layout, every member may be NULL:
 *   log_offset      [n]         (input) as in lh_posterior_outputs
 *   loglik          [n]
 *   codons          [n][C][64]  T
 *   change          [n][C][4]
 *   weighted_codons [C][64]     sum_i w_i T_i, w_i = exp(loglik_i - log_offset_i - max)
 *   weighted_change [C][4]
 *   weight_stats    [3]         max, sum w, sum w^2 as in lh_posterior_outputs
 * A row with a non-finite log-likelihood, a rejected schedule or (device form) a bad path gets NaN in codons and change
 * and no weight; the path is checked, the error word raised and the host-pointer form's device copies of codons and change
 * bounded (4 GiB) as for lh_eval_ancestral_batch.  The sums run in sample order (K5's slab scheme); the same sample gives
 * the same bits whatever the batch around it. */
typedef struct lh_node_codons_outputs {
  const double* log_offset;
  double* loglik;
  double* codons;
  double* change;
  double* weighted_codons;
  double* weighted_change;
  double* weight_stats;
} lh_node_codons_outputs;

int lh_eval_node_codons_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                              const double* brlen, const double* er, const double* pi, const double* alpha,
                              int32_t num_rates, const int32_t* path, int32_t path_len, int32_t node,
                              const lh_node_codons_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_eval_node_codons_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                     const double* brlen, const double* er, const double* pi, const double* alpha,
                                     int32_t num_rates, const int32_t* path, int32_t path_len, int32_t node,
                                     const lh_node_codons_outputs* outs, void* hip_stream);

/* The contraction alone behind one pruning pass: lh_asr_marginals_batch's trees and given rates[n][num_rates], with the
 * caller's naive codon posteriors naive_codons[n][C][125] in place of naive_prob; codons[n][C][64] and change[n][C][4]
 * (either may be NULL).  Needs lh_family_set_codons (for the frame). */
int lh_asr_node_codons_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                             const double* brlen, const double* er, const double* pi, const double* rates,
                             int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                             int32_t node, double* codons, double* change);
int lh_asr_node_codons_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* rates,
                                    int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                                    int32_t node, double* codons, double* change, void* hip_stream);

/* K14 at a node per row, slot[n] as lh_eval_ancestral_candidates_at_batch takes it (the same checks and error word);
 * everything else is the `node` forms'.  They honour lh_family_set_extended_range as those do. */
int lh_eval_node_codons_at_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                 const double* brlen, const double* er, const double* pi, const double* alpha,
                                 int32_t num_rates, const int32_t* path, int32_t path_len, const int32_t* slot /* [n] */,
                                 const lh_node_codons_outputs* outs);
int lh_eval_node_codons_at_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                        const double* brlen, const double* er, const double* pi, const double* alpha,
                                        int32_t num_rates, const int32_t* path, int32_t path_len,
                                        const int32_t* slot /* [n] */, const lh_node_codons_outputs* outs, void* hip_stream);
int lh_asr_node_codons_at_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* rates,
                                int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                                const int32_t* slot /* [n] */, double* codons, double* change);
int lh_asr_node_codons_at_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                       const double* brlen, const double* er, const double* pi, const double* rates,
                                       int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                                       const int32_t* slot /* [n] */, double* codons, double* change, void* hip_stream);

/* classes[125][64]: the class 0 .. 3 (the entries of change) of every (naive triple, node triple) pair, as the kernel's
 * compile-time table has it. */
int lh_node_codon_classes(uint8_t* classes);

/* Times of K14 over the launches made while profiling was enabled (HIP events on the launch stream), ms[3]: K9 with the
 * tables (rate weights, path check, K13b, rate combination, the naive codons of every codon), the contraction, the
 * weighted reduction (lh_eval_node_codons_batch only); resets the counters. */
int lh_node_codons_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K15: exact amino-acid replacement posteriors along the edges of a seed's lineage ----
 * Which residue was replaced on which step of the lineage.  Neither K12's per-site edge tables nor K14's node tables give
 * it: a codon's three sites are coupled through the naive codon at both ends of an edge, and the two ends are dependent.
 * Given the naive base b of a site everything at that site is independent of the rest, so with
 *   H_s[j][b][a][c] = P(x_{v_s,j} = a, x_{below,j} = c | column j, naive_j = b)
 * (path, seed tip and "below" as for lh_asr_edges_batch, tables [ancestor][descendant]) and K9's Q, the joint of codon c
 * over the sites j1, j2, j3 = frame + 3 c .. at the two ends of edge s is
 *   E_s[c][x][y] = sum_b Q[c][b1 b2 b3] H_s[j1][b1][x1][y1] H_s[j2][b2][x2][y2] H_s[j3][b3][x3][y3]
 * and the naive edge is K14's joint at the MRCA.  An edge's classes: [0] the lower codon equals the upper, [1] another
 * codon with the same translation, [2] a different translation (the standard code, the stop codons a symbol of their own:
 * 21 symbols, lh_codon_edge_symbols); on the naive edge only the N-free naive triples count, [3] is the rest.
 * With C = n_codons of lh_codon_layout and P = path_len, every member may be NULL:
 *   log_offset            [n]             (input) as in lh_posterior_outputs
 *   loglik                [n]
 *   codon_counts          [n][C][4]       expected number of lineage edges, naive to seed, on which the codon stays, changes
 *                                         silently, changes by replacement; [3] the naive-edge mass of naive triples with an N.
 *                                         The four sum to the chain length + 1.
 *   aa_counts             [n][C][21][21]  expected number of edges on which the translation goes from X (upper end) to Y
 *                                         (lower end); trace = codon_counts [0] + [1], off-diagonal sum = [2]
 *   seed_change           [n][C][3]       the three classes on the edge into the seed alone
 *   edge_change           [n][P+1][C][3]  per edge (slot s: v_s to below; entry P: the naive edge, K14's change [0..2] at the
 *                                         MRCA); padding slots 0
 *   edge_load             [n][P+1][2]     expected number of codons changing silently / by replacement on each edge
 *   weighted_codon_counts [C][4], weighted_aa_counts [C][21][21], weighted_seed_change [C][3]
 *                                         sum_i w_i row_i, w_i = exp(loglik_i - log_offset_i - max)
 *   weight_stats          [3]             max, sum w, sum w^2 as in lh_posterior_outputs
 * Needs lh_family_set_sampler and lh_family_set_codons; the extended-range mode is honoured.  A row with a non-finite
 * log-likelihood, a rejected schedule or (device form) a bad path or seed gets NaN and no weight; path and seed are checked,
 * the error word raised and the host-pointer form's device copies bounded (4 GiB) as for lh_eval_edges_batch.  The sums run
 * in sample order (K5's slab scheme); the same sample gives the same bits whatever the batch around it. */
typedef struct lh_codon_edges_outputs {
  const double* log_offset;
  double* loglik;
  double* codon_counts;
  double* aa_counts;
  double* seed_change;
  double* edge_change;
  double* edge_load;
  double* weighted_codon_counts;
  double* weighted_aa_counts;
  double* weighted_seed_change;
  double* weight_stats;
} lh_codon_edges_outputs;

int lh_eval_codon_edges_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                              const double* brlen, const double* er, const double* pi, const double* alpha,
                              int32_t num_rates, const int32_t* path, int32_t path_len, int32_t seed_tip,
                              const lh_codon_edges_outputs* outs);

/* Same with every array (the members of outs included) resident on the handle's device; enqueued on `hip_stream`
 * without synchronising. */
int lh_eval_codon_edges_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                     const double* brlen, const double* er, const double* pi, const double* alpha,
                                     int32_t num_rates, const int32_t* path, int32_t path_len, int32_t seed_tip,
                                     const lh_codon_edges_outputs* outs, void* hip_stream);

/* The tables alone behind one pruning pass: lh_asr_node_codons_batch's trees, given rates[n][num_rates] and the caller's
 * naive codon posteriors naive_codons[n][C][125], with seed_tip; the five per-row tables above (each may be NULL) and
 * cond_edge[n][P][L][5][4][4] (may be NULL), H spread over the sites.  Needs lh_family_set_codons (for the frame). */
int lh_asr_codon_edges_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                             const double* brlen, const double* er, const double* pi, const double* rates,
                             int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                             int32_t seed_tip, double* codon_counts, double* aa_counts, double* seed_change,
                             double* edge_change, double* edge_load, double* cond_edge);
int lh_asr_codon_edges_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                    const double* brlen, const double* er, const double* pi, const double* rates,
                                    int32_t num_rates, const double* naive_codons, const int32_t* path, int32_t path_len,
                                    int32_t seed_tip, double* codon_counts, double* aa_counts, double* seed_change,
                                    double* edge_change, double* edge_load, double* cond_edge, void* hip_stream);

/* sym[64]: the symbol 0 .. 20 (its position in "ACDEFGHIKLMNPQRSTVWY*") of every triple 16 x1 + 4 x2 + x3 over A,C,G,T,
 * as the kernel's compile-time map has it. */
int lh_codon_edge_symbols(uint8_t* sym);

/* Times of K15 over the launches made while profiling was enabled (HIP events on the launch stream), ms[3]: K9 with the
 * tables (rate weights, path and seed check, K15b, rate combination, the naive codons of every codon), the contraction, the
 * weighted reduction (lh_eval_codon_edges_batch only); resets the counters. */
int lh_codon_edges_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* Timing of the kernels of the last lh_eval_batch_device call sequence, measured with HIP events
 * on the launch stream when enabled (ms per kernel family: model, prune, forward). */
int lh_profile_enable(lh_family* fam, int enable);
int lh_profile_read(lh_family* fam, double* ms_model, double* ms_prune, double* ms_forward,
                    int64_t* n_launches);

/* Time of the sampling kernel (K3) over the lh_asr_batch_device launches made while profiling was
 * enabled (HIP events on the launch stream); resets the counters. */
int lh_asr_profile_read(lh_family* fam, double* ms_sampling, int64_t* n_launches);

/* ---- K8: the most probable state path (Viterbi), exact annotation probabilities ----
 * The max-product counterpart of the forward sweep: per tree sample the most probable V(D)J state path a* given the
 * data and the tree, and log P(data, a* | t).  Needs lh_family_set_sampler (the path is written in K4's layout).
 *   log_offset   [n]      as in lh_posterior_outputs; may be NULL
 *   loglik       [n]      the sample's log-likelihood (may be NULL)
 *   states       [n][lh_sample_states()]  the path in lh_eval_sample_batch's layout and encoding: J gene | D-J rows |
 *                         D gene | V-D rows | V gene, dense state indices (may be NULL)
 *   log_path     [n]      log P(data, a* | t); log_path - loglik <= 0 is the path's posterior given the tree (may be NULL)
 *   weight_stats [3]      max lw, sum w_i, sum w_i^2 as in lh_posterior_outputs; may be NULL
 * A sample whose log-likelihood is NaN or +inf in the active range mode, or whose schedule the device rejected (which
 * raises the handle's error word as everywhere else), gets states = -1 and log_path = NaN.  A sample no path of which
 * has positive probability (log-likelihood -inf) gets states = -1 and log_path = -inf.
 * Ties are broken by the values alone, so a row's result does not depend on its place in a batch or on the range mode:
 * the lowest left gene in a junction's cross-gene term; among a state's predecessors the cross-gene term before the
 * gene's own NTI states A, C, G, T before its own previous germline position; the lowest gene of the last J vector. */
typedef struct {
  const double* log_offset;
  double* loglik;
  int32_t* states;
  double* log_path;
  double* weight_stats;
} lh_viterbi_outputs;

/* Host pointers. */
int lh_eval_viterbi_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                          const double* brlen, const double* er, const double* pi, const double* alpha,
                          int32_t num_rates, const lh_viterbi_outputs* outs);
/* Every array resident on the handle's device; enqueued on `hip_stream` without synchronising. */
int lh_eval_viterbi_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                 const double* brlen, const double* er, const double* pi, const double* alpha,
                                 int32_t num_rates, const lh_viterbi_outputs* outs, void* hip_stream);

/* K8 on caller-supplied per-column emissions em[n][C] (host pointers), beside lh_forward_batch:
 * log_path[n] and states[n][lh_sample_states()] (either may be NULL). */
int lh_viterbi_forward_batch(lh_family* fam, int32_t n, const double* em, double* log_path, int32_t* states);

/* Registers K state paths states[K][lh_sample_states()] as the handle's candidates, in the slot lh_family_set_candidates
 * fills: their naive sequences (K6c) with log P_HMM(a_k) -- the path's weight with every emission 1, returned in
 * log_prior[K] (may be NULL) -- as the candidates' priors.  lh_eval_candidates_batch[_device] then returns
 * log P(a_k | data, t_i) and the weighted sums.  A vector that is not a path of the model (an index out of range, a
 * transition of probability 0) is refused and leaves the handle without candidates. */
int lh_family_set_candidate_paths(lh_family* fam, int32_t K, const int32_t* states, double* log_prior);

/* Time of K8 over the lh_eval_viterbi_batch[_device] launch groups made while profiling was enabled. */
int lh_viterbi_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K9: exact posterior distributions of the naive sequence's codons ----
 * For a reading frame f, codon c covers alignment sites f + 3c .. f + 3c + 2, c = 0 .. floor((L - f) / 3) - 1.  The three
 * bases of a codon are dependent wherever a junction is involved, so per-site marginals (K5) do not give the codon's
 * distribution: K9 forms the joint posterior of the (at most three) consecutive chain positions -- V genes | V-D rows |
 * D genes | D-J rows | J genes -- that write the codon's sites and pushes it forward onto (b1, b2, b3) in {A,C,G,T,N}^3,
 * 125 entries per codon, index 25 b1 + 5 b2 + b3.  The device writes the "window" codons, those with a site in a junction
 * row, and the sample's gene posteriors; a codon that lies inside one germline region is a linear map of that region's
 * gene posterior, which the host applies (linearham_amd/posterior.py codon_table, PhyloHMM::ExpandCodons).
 *
 * lh_family_set_codons fixes the frame and builds the window tables on the device (replacing an earlier frame's).  Needs
 * lh_family_set_sampler and a family with an MSA.  Refused: a frame outside 0 .. 2, and a family whose D region has no
 * alignment site of its own between the two junctions (a codon would then span more than three chain positions). */
int lh_family_set_codons(lh_family* fam, int32_t frame);

/* The layout lh_family_set_codons built: the number of codons of the frame, the number of window codons, their codon
 * indices window_codon[n_window] (ascending) and the number of gene posteriors nV + nD + nJ.  Any pointer may be NULL. */
int lh_codon_layout(const lh_family* fam, int32_t* n_codons, int32_t* n_window, int32_t* window_codon, int32_t* n_genes);

/* Every member may be NULL.  log_offset is an input, as in lh_posterior_outputs.
 *   loglik           [n]
 *   windows          [n][n_window][125]  the window codons' distributions; NaN for a sample whose loglik is not finite
 *                                        (an overflowed row in the active mode, or a rejected schedule)
 *   genes            [n][n_genes]        V | D | J gene posteriors, as in the forward layout; NaN likewise
 *   weighted_windows [n_window][125]     sum_i w_i windows_i, in a fixed order; samples with w_i = 0 are left out
 *   weighted_genes   [n_genes]           sum_i w_i genes_i
 *   weight_stats     [3]                 max lw, sum w_i, sum w_i^2, as lh_eval_posterior_batch's for the same rows
 * Batches combine exactly: rescale each one's sums by exp(max_b - max). */
typedef struct {
  const double* log_offset;
  double* loglik;
  double* windows;
  double* genes;
  double* weighted_windows;
  double* weighted_genes;
  double* weight_stats;
} lh_codon_outputs;

/* lh_eval_batch followed by K9 (lh_family_set_codons first).  Host pointers; a malformed schedule fails the call as in
 * lh_eval_posterior_batch. */
int lh_eval_codons_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                         const double* brlen, const double* er, const double* pi, const double* alpha,
                         int32_t num_rates, const lh_codon_outputs* outs);

/* The same with every array (outs' members included) resident on the handle's device; enqueued on `hip_stream` without
 * synchronising.  A schedule K0c rejects gives that sample NaN, leaves it out of the weighted sums and raises the
 * handle's error word (lh_family_status). */
int lh_eval_codons_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha,
                                int32_t num_rates, const lh_codon_outputs* outs, void* hip_stream);

/* Time of K9 (smoothing and reduction) over the lh_eval_codons_batch[_device] calls made while profiling was enabled
 * (HIP events on the launch stream); resets the counters. */
int lh_codon_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

/* ---- K10: exact posteriors of the recombination events (deletion and insertion lengths) ----
 * Every state path of non-zero probability reads  left germline* NTI* right germline*  on a junction's W rows (the rows
 * of lh_forward_layout).  For a path let  a = the number of junction rows its left gene l occupies (0 .. W)  and
 * b = the first row that holds a germline state of its right gene r (W: none);  a <= b, and b - a is the insertion's
 * length.  Per tree sample and junction K10 writes three tables, each summing to 1:
 *   exit [nL][W+1]   P(l, a | data, tree)
 *   enter[nR][W+1]   P(r, b | data, tree)
 *   span [W+1][W+1]  P(a, b | data, tree): zero below the diagonal; its row and column sums are the gene sums of exit and
 *                    enter; its k-th diagonal sums to P(insertion length = k)
 * as one flat row of lh_events_size doubles: the V-D junction's  exit | enter | span,  then (heavy chains) the D-J
 * junction's.  exit and enter are differences of K5's posteriors; span comes from a backward chain through K5's
 * conditional steps.  Only ratios inside one forward row appear: the results do not depend on the range mode.
 *
 * lh_events_layout: per junction j < *n_junctions (1 or 2) the arrays receive rows[j] = W, n_left[j], n_right[j] and
 * the offsets of its three tables in the row; *size the row's length, *n_genes = nV + nD + nJ.  Every array holds two
 * entries; any pointer may be NULL.  Needs lh_family_set_sampler. */
int lh_events_layout(const lh_family* fam, int32_t* n_junctions, int32_t* rows, int32_t* n_left, int32_t* n_right,
                     int64_t* exit_off, int64_t* enter_off, int64_t* span_off, int64_t* size, int32_t* n_genes);

/* Every member may be NULL.  log_offset is an input, as in lh_posterior_outputs.
 *   loglik          [n]
 *   events          [n][size]     the tables; NaN for a sample whose loglik is not finite (an overflowed row in the active
 *                                 mode, or a rejected schedule)
 *   genes           [n][n_genes]  V | D | J gene posteriors (K5's); NaN likewise
 *   weighted_events [size]        sum_i w_i events_i, in a fixed order; samples with w_i = 0 are left out
 *   weighted_genes  [n_genes]     sum_i w_i genes_i
 *   weight_stats    [3]           max lw, sum w_i, sum w_i^2, as lh_eval_posterior_batch's for the same rows
 * Batches combine exactly: rescale each one's sums by exp(max_b - max). */
typedef struct {
  const double* log_offset;
  double* loglik;
  double* events;
  double* genes;
  double* weighted_events;
  double* weighted_genes;
  double* weight_stats;
} lh_events_outputs;

/* lh_eval_batch followed by K5 (on a copy of the forward arrays) and K10.  Host pointers; a malformed schedule fails the
 * call as in lh_eval_posterior_batch. */
int lh_eval_events_batch(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                         const double* brlen, const double* er, const double* pi, const double* alpha,
                         int32_t num_rates, const lh_events_outputs* outs);

/* The same with every array (outs' members included) resident on the handle's device; enqueued on `hip_stream` without
 * synchronising.  A schedule K0c rejects gives that sample NaN, leaves it out of the weighted sums and raises the
 * handle's error word (lh_family_status). */
int lh_eval_events_batch_device(lh_family* fam, int32_t n, int32_t n_tips, int32_t max_depth, const int32_t* ops,
                                const double* brlen, const double* er, const double* pi, const double* alpha,
                                int32_t num_rates, const lh_events_outputs* outs, void* hip_stream);

/* K10 on caller-supplied emissions em[n][n_xmsa] (lh_forward_batch's), without a tree: loglik[n] and events[n][size]
 * (either may be NULL).  The twin of lh_viterbi_forward_batch. */
int lh_events_forward_batch(lh_family* fam, int32_t n, const double* em, double* loglik, double* events);

/* Times of K5's pass and of K10 (with the reduction) over the lh_eval_events_batch[_device] calls made while profiling
 * was enabled: ms[2] = smoothing, events; resets the counters. */
int lh_events_profile_read(lh_family* fam, double* ms, int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* LINEARHAM_AMD_H_ */
