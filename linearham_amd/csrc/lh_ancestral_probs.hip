// K13: exact posterior probabilities of candidate ancestral sequences at a node of a seed's lineage (gfx950).
//
// What K3 draws and K7 counts for whole sequences, as probabilities.  For a tree sample t, a node v of the seed's path (the
// seed's parent, slot 0, or the MRCA, the last slot) and a candidate x of L bytes (A, C, G, T, or 4 = the site is left open)
//   P(X_v = x | data, t) = sum_paths prior(path) prod_j E_t[b_j, j] G_t[j][b_j][x_j] / P(data | t),
// b_j the naive base the path writes on site j, E_t the xMSA emission of the evaluation and
//   G_t[j][b][c] = P(x_{v,j} = c | column j, naive_j = b) = sum_r [lik_r(j, b) / Z_j(b)] P(x_{v,j} = c | column j, b, rate r),
// G = 1 at an open site.  G is K11's marg for a one-hot naive distribution at b; it depends on the site only through its
// pattern.  The sites of a node are coupled through the naive sequence, so the sum over paths does not factorise: every
// (row, candidate) pair takes a forward sweep, K2a + K2b on the family's caller-column twin (K6a's) with the emissions
// em'[col] = em[col] G[site(col)][base(col)][x[site(col)]].
//
// Kernels:
//  * K11r, K3s and K11c (launch_ancestral_front) run in front: the path is checked against the sample's own schedule.
//  * K13b (cond_kernel), a workgroup per (rate category, sample) as K11b, with K11b's prologue, upward pass and step
//    down the lineage (lh_treepass.h); a lane per PATTERN in both passes, so a lane reads back only the CLVs it stored
//    itself.  The joint P(x = c, column | b, r) is linear in the naive tip's vector: the down pass carries the message
//    from above for the five basis vectors (A, C, G, T, N) at once, a 4 x 5 block, each column divided by its own
//    largest entry after every step.  At the node the table is normalised per (basis, rate) and weighted by lik_r(j, b)
//    / Z_j(b) from K1's unmixed planes (scaler counts aligned to the smallest, RatePlanes as K11r):
//    part[sample][rate][pattern][5][4].  Z = 0, a dead category or an all-zero table gives 0. The all-N pattern takes
//    K11's convention: likelihood pi_b under base b, sum pi under N, so the weight is 1 / R.
//    The node is a template switch.  kMrca: no down step, the root's CLV stays in the lane's registers and the upward
//    pass stores only what a later op pops from its stack.  Otherwise (the seed's parent): K11b's walk down the chain.
//  * K13m (K11m's rate_sum_kernel, lh_ancestral.hip), a thread per cell: the R partial tables added in rate order
//    (fixed order, no atomics); NaN for a sample without a valid path.  site_gather_kernel spreads the patterns' tables
//    over the sites for a caller who takes them: cond[n][L][5][4].
//  * K13e (pair_emission_kernel), a thread per (pair, caller column) of a group of (row, candidate) pairs, pair q = row * K
//    + candidate: the emissions above.  Rows without a path get 0 (row_mask_kernel does the same to the rows' own
//    emissions), so the sweeps see what K6a's see; pair_finish_kernel turns the sweeps' log-likelihoods into
//    log_cand = ll'(x) - ll'(open), the denominator being the twin's own sweep of the row's unmodified emissions: both
//    terms share their arithmetic, and an all-open candidate gives exactly 0.
// No private array is reached by a dynamic index: 4-vectors and the 4 x 5 block are indexed by unrolled loops only.
#include <algorithm>

#include "lh_treepass.h"

namespace lh {

namespace {

// kForm: kCondParent (the walk down the chain ends at slot 0), kCondMrca (no down step) or kCondSlot (the walk ends at
// slot[sample] of the sample's own path; a workgroup serves one (sample, rate), so the slot is uniform over it).
enum { kCondParent = 0, kCondMrca = 1, kCondSlot = 2 };

template <int kForm>
__global__ void __launch_bounds__(256) cond_kernel(int R, int T, int n_prune, int P, const uint8_t* __restrict__ msa,
                                                   const AsrOp* __restrict__ desc, const double* __restrict__ brlen,
                                                   const double* __restrict__ rates, const double* __restrict__ eig,
                                                   const double* __restrict__ pi, const double* __restrict__ site_lik,
                                                   const int32_t* __restrict__ site_scal, const int32_t* __restrict__ chain,
                                                   const int32_t* __restrict__ plen, double2* clv, int Lp,
                                                   double* __restrict__ part, const int32_t* __restrict__ slot) {
  constexpr bool kMrca = kForm == kCondMrca;
  extern __shared__ double2 cond_smem[];
  const TreeTables tt = tree_prologue(cond_smem, R, T, desc, brlen, rates, eig, plen, clv, Lp);
  const int len = tt.len;
  if (len == 0) return;  // K13m writes the row's NaN
  const int NP = n_prune + 1;
  const int sample = blockIdx.y, rate = blockIdx.x;
  const double* tiptab = tt.tiptab;
  const size_t plane = tt.plane;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_waves = blockDim.x >> 6;
  const double* __restrict__ p4 = pi + (size_t)sample * 4;
  const int32_t* __restrict__ ch = chain + (size_t)sample * P;
  double* part_s = part + ((size_t)sample * R + rate) * (size_t)NP * 20;
  // (slot_check_kernel has left len 0 where the slot lies outside the path)
  const int stop = kForm == kCondSlot ? slot[sample] : 0;

  for (int s0 = wave * 64; s0 < NP; s0 += n_waves * 64) {
    const bool live = s0 + lane < NP;
    const int pat = min(s0 + lane, NP - 1);
    const bool all_n = pat >= n_prune;
    double node[4];  // the node's CLV
    tree_upward_pattern<!kMrca>(T - 2, n_prune, pat, msa, tt.dsc, tiptab, tt.pin, tt.clv_s, plane, node);

    // the weight of this category under each naive base
    double w[5];
    tree_rate_weights(site_scal, site_lik, sample, rate, R, n_prune, pat, all_n, w);

    // the message into the root from above, per basis vector of the naive tip
    double A[5][4];
    tree_root_messages(tiptab, p4, A);
    if (!kMrca) {
      for (int s = len - 1; s > stop; --s) {
        // the message into v_{s-1}: the sibling off the path times the message from above, through v_{s-1}'s branch
        double m[4];
        const int kc = tree_sibling_message(tt, ch[s], msa, n_prune, pat, all_n, m);
#pragma unroll
        for (int b = 0; b < 5; ++b) tree_descend(tt.pin, kc, m, A[b]);
      }
      tree_load_clv(tt.clv_s, plane, chain_op(ch[stop]), pat, node);
    }
    if (live) {
      double2* o = reinterpret_cast<double2*>(part_s + (size_t)pat * 20);
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        const double post[4] = {A[b][0] * node[0], A[b][1] * node[1], A[b][2] * node[2], A[b][3] * node[3]};
        const double sum = (post[0] + post[1]) + (post[2] + post[3]);
        // a category of weight 0 or an all-zero table contributes 0, not NaN
        const double f = (sum == 0.0 || w[b] == 0.0) ? 0.0 : w[b] / sum;
        o[2 * b] = make_double2(f == 0.0 ? 0.0 : f * post[0], f == 0.0 ? 0.0 : f * post[1]);
        o[2 * b + 1] = make_double2(f == 0.0 ? 0.0 : f * post[2], f == 0.0 ? 0.0 : f * post[3]);
      }
    }
  }
}

// Beside K11c: a sample whose slot lies outside its path becomes a sample without a path (plen 0: NaN tables, no weight).
// Bit 2 of err[0] is raised and err[1] keeps 0x7fffffff - (the first such row of the call), 0 while there is none.
__global__ void __launch_bounds__(256) slot_check_kernel(int n, int row0, const int32_t* __restrict__ slot, int32_t* plen,
                                                         int32_t* err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int len = plen[i], s = slot[i];
  if (len == 0 || (s >= 0 && s < len)) return;
  plen[i] = 0;
  atomicOr(err, 4);
  atomicMax(err + 1, 0x7fffffff - (row0 + i));
}

__global__ void __launch_bounds__(256) row_mask_kernel(int n, int C, const int32_t* __restrict__ plen, double* __restrict__ em) {
  const size_t total = (size_t)n * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    if (plen[i / C] == 0) em[i] = 0.0;
}

// K13e
__global__ void __launch_bounds__(256) pair_emission_kernel(int K, int L, int C, int n_prune, long long q0, int count,
                                                            const uint8_t* __restrict__ seqs,
                                                            const int32_t* __restrict__ col_site,
                                                            const uint8_t* __restrict__ col_base,
                                                            const int32_t* __restrict__ site_pat,
                                                            const int32_t* __restrict__ plen, const double* __restrict__ em,
                                                            const double* __restrict__ table, double* __restrict__ out) {
  const size_t total = (size_t)count * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / C, c = i - p * C;
    const long long q = q0 + (long long)p;
    const size_t row = (size_t)(q / K), k = (size_t)(q - (long long)row * K);
    const int site = col_site[c];
    const int x = seqs[k * L + site];
    double v = 0.0;
    if (plen[row] != 0) {
      v = em[row * C + c];
      if (x < 4) v *= table[((row * (size_t)(n_prune + 1) + min(site_pat[site], n_prune)) * 5 + col_base[c]) * 4 + x];
    }
    out[i] = v;
  }
}

__global__ void __launch_bounds__(256) pair_finish_kernel(int K, long long q0, int count, const double* __restrict__ pair_ll,
                                                          const double* __restrict__ open_ll, const int32_t* __restrict__ plen,
                                                          double* log_cand, double* prob) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= count) return;
  const long long q = q0 + p;
  const size_t row = (size_t)(q / K);
  const double den = open_ll[row];
  const double v = (plen[row] == 0 || !isfinite(den)) ? __builtin_nan("") : pair_ll[p] - den;
  if (log_cand) log_cand[q] = v;
  if (prob) prob[q] = exp(v);
}

unsigned strided_blocks(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, 8192); }

}  // namespace

CondWsBytes cond_ws_bytes(int R, int n_prune) {
  return {sizeof(double) * (size_t)R * (n_prune + 1) * 20, sizeof(double) * (size_t)(n_prune + 1) * 20};
}

int launch_ancestral_cond(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen,
                          const double* rates, const double* eig, const double* pi, const double* site_lik,
                          const int32_t* site_scal, const double* naive_prob, const int32_t* path, int P, int node,
                          const AncWs& ws, double* table, double* cond, const int4* hdr, int32_t* err_flag,
                          hipStream_t stream, const int32_t* slot, int slot_row0) {
  const int L = fam.n_sites, NP = fam.n_prune + 1;
  if (n < 1 || n > 65535 || L < 1 || P < 1 || (!slot && (node < 0 || node > 1))) return 1;  // (one grid row per sample)
  const size_t lds = anc_lds_bytes(T);
  if (lds > 160 * 1024) return 1;
  launch_ancestral_front(fam, n, R, T, ops, pi, site_lik, site_scal, naive_prob, path, P, ws, nullptr, hdr, err_flag, stream);
  auto run = [&](auto kernel) {
    launch_lds(kernel, dim3(R, n), dim3(256), lds, stream, R, T, fam.n_prune, P, fam.msa,
               static_cast<const AsrOp*>(ws.desc), brlen, rates, eig, pi, site_lik, site_scal, ws.chain, ws.plen,
               reinterpret_cast<double2*>(ws.clv), (int)anc_lp(fam.n_prune), ws.part, slot);
  };
  if (slot) {
    hipLaunchKernelGGL(slot_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, slot_row0, slot, ws.plen,
                       err_flag);
    run(cond_kernel<kCondSlot>);
  } else if (node == 1) {
    run(cond_kernel<kCondMrca>);
  } else {
    run(cond_kernel<kCondParent>);
  }
  launch_rate_sum(n, R, 1, (size_t)NP * 20, false, ws.plen, ws.part, table, stream);
  if (cond) launch_site_gather(fam, n, 20, table, cond, stream);
  return 0;
}

void launch_row_mask(int n, int C, const int32_t* plen, double* em, hipStream_t stream) {
  hipLaunchKernelGGL(row_mask_kernel, dim3(strided_blocks((size_t)n * C)), dim3(256), 0, stream, n, C, plen, em);
}

void launch_pair_emissions(const DevFamily& fam, int K, long long q0, int count, const uint8_t* seqs, const int32_t* col_site,
                           const uint8_t* col_base, const int32_t* plen, const double* em, const double* table, double* out,
                           hipStream_t stream) {
  hipLaunchKernelGGL(pair_emission_kernel, dim3(strided_blocks((size_t)count * fam.n_xmsa)), dim3(256), 0, stream, K,
                     fam.n_sites, fam.n_xmsa, fam.n_prune, q0, count, seqs, col_site, col_base, fam.site_pat, plen, em, table,
                     out);
}

void launch_pair_finish(int K, long long q0, int count, const double* pair_ll, const double* open_ll, const int32_t* plen,
                        double* log_cand, double* prob, hipStream_t stream) {
  hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, K, q0, count, pair_ll,
                     open_ll, plen, log_cand, prob);
}

}  // namespace lh
