// K6: exact posterior probabilities of candidate naive sequences on the device (gfx950, FP64).
//
// Every HMM state writes one fixed naive base on one fixed site, and the xMSA emission of a state depends only on that
// (naive base, site) pair.  So for a naive sequence s of the alignment's L sites and a tree sample t
//   P(data, s | t)   = P_HMM(s) * prod_i E_t[s_i, i]
//   log P(s | data, t) = log P_HMM(s) + sum_i log E_t[s_i, i] - loglik_t,
// where P_HMM(s), the total probability of the state paths whose naive sequence is s, does not depend on the tree.
//
// K6a (lh_family_set_candidates) computes log P_HMM(s) once per candidate: the forward sweep K2a/K2b run, on the
// caller-column twin of the family (lh_capi.hip), with every emission replaced by the indicator that the column's naive
// base is the candidate's base at the column's site (launch_candidate_indicators).  Same tables, same rescaling; a
// candidate no path produces ends at log 0 = -inf.
//
// K6b runs after K0-K2 of a batch.  K2a writes the log emissions of the u-columns the candidates touch (LogEmRequest,
// lh_device.h), the values it assembles itself, 2^-256 counts included in the extended-range mode.  Sites where every
// candidate has the same base fold into one per-row constant (const_kernel); what is left is a gather per (row,
// candidate) over the V variable sites (score_kernel), then exp and the importance weight of the row, summed over the
// rows of a slab in order and over the slabs in order (K5's launch_slab_sum): no atomics, the same batch gives the same
// bits.  A row whose loglik is not finite gets NaN and weight 0 (K5's weight_kernel), so it is left out of the sums.
#include <algorithm>
#include <cmath>

#include "lh_device.h"

namespace lh {

namespace {

constexpr int kThreads = 256;  // candidates per scoring workgroup, one per thread
constexpr int kSlab = 256;     // rows per partial sum
constexpr size_t kLdsLimit = 160 * 1024;

__global__ void __launch_bounds__(kThreads)
    indicator_kernel(int K, int L, int C, const uint8_t* __restrict__ seqs, const int32_t* __restrict__ col_site,
                     const uint8_t* __restrict__ col_base, double* __restrict__ em) {
  const size_t total = (size_t)K * C;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
    const size_t k = i / C, c = i % C;
    em[i] = seqs[k * L + col_site[c]] == col_base[c] ? 1.0 : 0.0;
  }
}

// One wave per row: base[i] = sum_j agree[j] lem[i][j] - loglik[i] (terms with agree[j] = 0 skipped: their log emission
// may be -inf), lane-strided partial sums and a fixed butterfly; NaN where loglik is not finite.
__global__ void __launch_bounds__(kThreads)
    const_kernel(int n, int n_lem, const double* __restrict__ lem, const double* __restrict__ agree,
                 const double* __restrict__ loglik, double* __restrict__ base) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  const double* l = lem + (size_t)i * n_lem;
  double acc = 0.0;
  for (int j = lane; j < n_lem; j += 64) {
    const double a = agree[j];
    if (a != 0.0) acc += a * l[j];
  }
  acc = wave_sum(acc);
  if (lane == 0) base[i] = isfinite(loglik[i]) ? acc - loglik[i] : __builtin_nan("");
}

// Grid (candidate blocks, slabs).  Thread k of a block owns one candidate; TB rows at a time have the log emissions of
// the variable sites' u-columns in LDS, lv[TB][n_vlem], and each thread gathers its V entries from them.
template <int TB>
__global__ void __launch_bounds__(kThreads)
    score_kernel(CandidateTables t, int n, const double* __restrict__ lem, const double* __restrict__ base,
                 const double* __restrict__ w, double* __restrict__ log_cand, double* __restrict__ partial) {
  extern __shared__ double lv[];
  const int k = blockIdx.x * kThreads + threadIdx.x;
  const int i0 = blockIdx.y * kSlab, i1 = min(n, i0 + kSlab);
  const int K = t.K, V = t.V, nv = t.n_vlem;
  const bool live = k < K;
  const double prior = live ? t.log_prior[k] : 0.0;
  double part = 0.0;
  for (int r = i0; r < i1; r += TB) {
    const int m = min(TB, i1 - r);
    __syncthreads();  // (the previous rows' gathers are done)
    for (int x = threadIdx.x; x < m * nv; x += kThreads) {
      const int q = x / nv, j = x - q * nv;
      lv[q * nv + j] = lem[(size_t)(r + q) * t.n_lem + j];
    }
    __syncthreads();
    if (!live) continue;
    double acc[TB];
#pragma unroll
    for (int q = 0; q < TB; ++q) acc[q] = 0.0;
    for (int v = 0; v < V; ++v) {
      const int u = t.idx[(size_t)v * K + k];
#pragma unroll
      for (int q = 0; q < TB; ++q)
        if (q < m) acc[q] += lv[q * nv + u];
    }
#pragma unroll
    for (int q = 0; q < TB; ++q) {
      if (q >= m) break;
      const int i = r + q;
      const double lc = prior + (base[i] + acc[q]);
      if (log_cand) log_cand[(size_t)i * K + k] = lc;
      if (w) {
        const double wi = w[i];
        if (wi != 0.0) part += wi * exp(lc);
      }
    }
  }
  if (w && live) partial[(size_t)blockIdx.y * K + k] = part;
}

}  // namespace

void launch_candidate_indicators(int K, int L, int C, const uint8_t* seqs, const int32_t* col_site, const uint8_t* col_base,
                                 double* em, hipStream_t stream) {
  const size_t total = (size_t)K * C;
  const unsigned blocks = (unsigned)std::min<size_t>((total + kThreads - 1) / kThreads, 8192);
  hipLaunchKernelGGL(indicator_kernel, dim3(std::max(blocks, 1u)), dim3(kThreads), 0, stream, K, L, C, seqs, col_site,
                     col_base, em);
}

int candidate_slabs(int n) { return (n + kSlab - 1) / kSlab; }

size_t candidate_lds_limit() { return kLdsLimit; }

void launch_candidates(const CandidateTables& t, int n, const double* lem, const double* loglik, const double* w,
                       double* base, double* log_cand, double* partial, hipStream_t stream) {
  const int per_block = kThreads / 64;
  hipLaunchKernelGGL(const_kernel, dim3((n + per_block - 1) / per_block), dim3(kThreads), 0, stream, n, t.n_lem, lem,
                     t.agree, loglik, base);
  const dim3 grid((t.K + kThreads - 1) / kThreads, candidate_slabs(n));
  // eight rows per LDS fill while they fit in 64 KB (two workgroups per CU at least), else one
  const size_t lds8 = (size_t)8 * t.n_vlem * sizeof(double), lds1 = (size_t)t.n_vlem * sizeof(double);
  if (lds8 <= 64 * 1024) {
    hipLaunchKernelGGL(score_kernel<8>, grid, dim3(kThreads), lds8, stream, t, n, lem, base, w, log_cand, partial);
  } else {
    launch_lds(score_kernel<1>, grid, dim3(kThreads), lds1, stream, t, n, lem, base, w, log_cand, partial);
  }
}

}  // namespace lh
