// K12: exact substitution posteriors along the edges of a seed's lineage (gfx950).
//
// K11 (lh_ancestral.hip) gives, per node of the path from a seed tip to naive, the posterior of the node's base.  The two
// ends of an edge are strongly dependent, so which substitution happened on which edge is not the product of two of those
// tables.  K11b's down pass holds the answer and sums it away: at slot s it multiplies the message from above A_s, the
// off-path sibling's message m_s and the on-path child's P-matrix and CLV, and keeps the 4-vector.  K12 keeps the 4 x 4 table.
//
// Notation as in lh_ancestral.hip: path v_0 (the seed's parent) .. v_{len-1} (the root, naive's neighbour), seed tip u, so
// the lineage has len + 1 edges.  Every table is indexed [ancestor state][descendant state], naive the oldest node.
//   inner and seed edges, per rate r:   J_s(a, c) = A_s(a) m_s(a) P_below[a][c] L_below(c)          s = 0 .. len-1
//     below = v_{s-1} with its stored CLV for s >= 1; for s = 0 the seed tip with its one-hot vector, or all ones for N:
//     with an N seed tip the table says what the model says about the unobserved base
//   naive edge, per rate r:             J(b, i) = t_j(b) pi_i P_naive[i][b] L_root(i)               b over A, C, G, T, N
//     (rowsum_i in place of P_naive[i][b] for N)
//   edge[s][j] = sum_r rho_r(j) J_s^(r) / sum_{a,c} J_s^(r),   naive_edge[j] likewise
// normalised per (slot, site, rate) before the weighting, exactly as K11 does; a category with rho_r = 0 or an all-zero J
// contributes 0, not NaN.  Margins: sum_c edge[s] = marg[s], sum_a edge[s] = marg[s-1], sum_i naive_edge = q, sum_b
// naive_edge = marg[len-1].
//
// Per-row reductions, formed here so that a pipeline never takes the per-slot tables back:
//   chain_counts[j][a][c] = naive_edge[j][a][c] (a < 4) + sum_s edge[s][j][a][c]
//     the expected number of lineage edges, naive to seed, on which site j goes from a to c.  An off-diagonal cell counts
//     EDGES whose two ends are a and c; it is not a count of substitutions inside a branch (multiple hits on one branch
//     show as one difference or none).  The cells of a site sum to len + 1 - q_j(N).
//     Summation order: per rate the naive edge first, then the slots len-1 down to 0; then the rates in order.
//   edge_load[e] = the expected number of sites whose two ends differ on edge e; e < P the slots (padding slots 0), e = P
//     the naive edge (rows b < 4 only).  Summation order: per rate and wave of the workgroup the 64-site chunks wave,
//     wave + 4, .. in order, each chunk reduced across its lanes by a butterfly of shuffles; then the four waves in order;
//     then the rates in order.  None of it depends on the batch.
//
// Kernels:
//  * K11r, K3s, K11c (launch_ancestral_front) as K11 runs them.
//  * K12c (sub_seed_kernel), a thread per sample: the seed tip must be a child of v_0 under the sample's own schedule (a
//    child of the cherry or the tip of the tip-accumulate op that produced v_0).  It marks in the chain word of slot 0 which
//    child it is; a failure leaves length 0 and raises bit 1 of the error word, as a bad path does.  seed_tip itself is
//    checked on the host (1 .. T-1) and only compared, never used as an index, before this verdict.
//  * K12b (sub_kernel<kWriteEdges>), a workgroup per (rate category, sample): K11b's prologue, upward pass and step down
//    the lineage, the seed edge at slot 0 included (shared code, lh_treepass.h; the message into the root is written
//    here), a lane per site in the down pass.  Per step: the 16 cells, their sum, the weight rho_r / sum.
//    The site's chain_counts partial lives in 16 registers; the step's off-diagonal mass is reduced across the wave with
//    shuffles and added to the wave's row of an LDS table by one lane.  Only the kWriteEdges form writes [slot][site][16]
//    per rate; the lean form writes [site][16] (chain_counts), [site][20] (naive edge), [P+1] (edge_load) and, where the
//    caller wants the slot-0 table without the others, one more [site][16].
//    Both forms do the same arithmetic in the same order (floating-point contraction is off in the down pass, fma is
//    written where it is meant), so the reductions have the same bits in both.
//  * K12m (K11m's rate_sum_kernel, lh_ancestral.hip), a thread per output cell: the R partials added in rate order -- no
//    atomics, the same bits whatever the batch.  NaN for a sample without a valid path, 0 in padding slots.
// No private array is reached by a dynamic index: the 4- and 16-vectors are indexed by unrolled loops only.
#include "lh_treepass.h"

namespace lh {

namespace {

constexpr int kSubWaves = 4;

// K12c
__global__ void __launch_bounds__(256) sub_seed_kernel(int n, int T, int P, int seed_tip, const AsrOp* __restrict__ desc,
                                                       int32_t* __restrict__ chain, int32_t* __restrict__ plen,
                                                       int32_t* err_flag) {
  const int sample = blockIdx.x * blockDim.x + threadIdx.x;
  if (sample >= n) return;
  if (plen[sample] == 0) return;  // K11c (or K0c) has refused the sample
  int32_t* ch = chain + (size_t)sample * P;
  const int k = chain_op(ch[0]);  // K11c took it from its own table: 0 <= k < T - 2
  const AsrOp d = desc[(size_t)sample * (T - 2) + k];
  const int kind = d.a.x & 15;
  int which = -1;
  if (kind == OP_CHERRY)
    which = d.b.x == seed_tip ? 0 : d.b.y == seed_tip ? 1 : -1;
  else if (kind == OP_TIP_ACC)
    which = d.b.x == seed_tip ? 0 : -1;
  if (which < 0) {
    plen[sample] = 0;
    atomicOr(err_flag, 2);
  } else {
    ch[0] = k | (which << 30);
  }
}

// One edge's table: J[a*4+c] = M[a] * p[a*SA + c*SC] * Lb[c], weighted by rj / sum.  Adds the weighted cells to cc, returns
// the weighted off-diagonal mass, leaves the weighted cells in J.
template <int SA, int SC>
__device__ __forceinline__ double sub_edge(const double (&M)[4], const double* p, const double (&Lb)[4], double rj,
                                           double (&J)[16], double (&cc)[16]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) J[a * 4 + c] = (M[a] * p[a * SA + c * SC]) * Lb[c];
  double row[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) row[a] = (J[a * 4] + J[a * 4 + 1]) + (J[a * 4 + 2] + J[a * 4 + 3]);
  const double sum = (row[0] + row[1]) + (row[2] + row[3]);
  const double f = (sum == 0.0 || rj == 0.0) ? 0.0 : rj / sum;
  double off = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double v = f == 0.0 ? 0.0 : f * J[a * 4 + c];
      J[a * 4 + c] = v;
      cc[a * 4 + c] += v;
      if (a != c) off += v;
    }
  return off;
}

__device__ __forceinline__ void sub_store16(double* o, const double (&J)[16]) {
  double2* o2 = reinterpret_cast<double2*>(o);
#pragma unroll
  for (int i = 0; i < 8; ++i) o2[i] = make_double2(J[2 * i], J[2 * i + 1]);
}

// K12b
template <bool kWriteEdges>
__global__ void __launch_bounds__(kSubWaves * 64) sub_kernel(int R, int T, int L, int n_prune, int P, int seed_tip,
                                                             const uint8_t* __restrict__ msa,
                                                             const int32_t* __restrict__ site_pat,
                                                             const AsrOp* __restrict__ desc, const double* __restrict__ brlen,
                                                             const double* __restrict__ rates, const double* __restrict__ eig,
                                                             const double* __restrict__ pi, const double* __restrict__ tvec,
                                                             const double* __restrict__ rho, const int32_t* __restrict__ chain,
                                                             const int32_t* __restrict__ plen, double2* clv, int Lp,
                                                             double* __restrict__ cc_part, double* __restrict__ ne_part,
                                                             double* __restrict__ se_part, double* __restrict__ el_part,
                                                             double* __restrict__ edge_part) {
  extern __shared__ double2 sub_smem[];
  const TreeTables tt = tree_prologue(sub_smem, R, T, desc, brlen, rates, eig, plen, clv, Lp);
  const int len = tt.len;
  if (len == 0) return;  // K12m writes the row's NaN
  const int n_ops = T - 2;
  const int sample = blockIdx.y, rate = blockIdx.x;
  const double *tiptab = tt.tiptab, *pin = tt.pin;
  const size_t plane = tt.plane;
  double* load = tt.pin + (size_t)n_ops * 16;  // [kSubWaves][P + 1] edge_load partials of the waves
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < kSubWaves * (P + 1); i += blockDim.x) load[i] = 0.0;

  tree_upward(n_ops, n_prune, msa, tt.dsc, tiptab, pin, tt.clv_s, plane, wave, kSubWaves, lane);
  // the sites' lanes below read CLVs that other lanes and waves of this workgroup stored above, and the zeroed load table
  __threadfence_block();
  __syncthreads();

  // ---- downward pass along the path, a lane per site
  const double* __restrict__ p4 = pi + (size_t)sample * 4;
  const int32_t* __restrict__ ch = chain + (size_t)sample * P;
  const size_t sr = (size_t)sample * R + rate;
  double* load_w = load + (size_t)wave * (P + 1);
  for (int s0 = wave * 64; s0 < L; s0 += kSubWaves * 64) {
#pragma clang fp contract(off)
    const bool live = s0 + lane < L;
    const int site = min(s0 + lane, L - 1);
    const int pat = min(site_pat[site], n_prune);
    const bool all_n = pat >= n_prune;
    const double* __restrict__ tj = tvec + ((size_t)sample * L + site) * 5;
    const double rj = rho[((size_t)sample * L + site) * R + rate];
    double cc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) cc[i] = 0.0;
    double A[4];
    {
      // the naive edge: J(b, i) = t(b) pi_i P_naive[i][b] L_root(i), 20 cells; A(i) = sum_b of the first three factors
      double Lr[4], n4[4];
      tree_load_clv(tt.clv_s, plane, chain_op(ch[len - 1]), pat, Lr);
      tree_tip_col(tiptab, 0, 4, n4);
      const double t[5] = {tj[0], tj[1], tj[2], tj[3], tj[4]};
      double J[20];
#pragma unroll
      for (int b = 0; b < 5; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) J[b * 4 + i] = ((t[b] * p4[i]) * (b < 4 ? tiptab[b * 4 + i] : n4[i])) * Lr[i];
      double row[5];
#pragma unroll
      for (int b = 0; b < 5; ++b) row[b] = (J[b * 4] + J[b * 4 + 1]) + (J[b * 4 + 2] + J[b * 4 + 3]);
      const double sum = ((row[0] + row[1]) + (row[2] + row[3])) + row[4];
      const double f = (sum == 0.0 || rj == 0.0) ? 0.0 : rj / sum;
      double off = 0.0;
#pragma unroll
      for (int b = 0; b < 5; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double v = f == 0.0 ? 0.0 : f * J[b * 4 + i];
          J[b * 4 + i] = v;
          if (b < 4) {
            cc[b * 4 + i] += v;
            if (b != i) off += v;
          }
        }
      if (live) {
        double2* o = reinterpret_cast<double2*>(ne_part + (sr * L + site) * 20);
#pragma unroll
        for (int i = 0; i < 10; ++i) o[i] = make_double2(J[2 * i], J[2 * i + 1]);
      }
      const double tot = wave_sum(live ? off : 0.0);
      if (lane == 0) load_w[P] += tot;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        A[i] = p4[i] * (t[0] * tiptab[i] + t[1] * tiptab[4 + i] + t[2] * tiptab[8 + i] + t[3] * tiptab[12 + i] + t[4] * n4[i]);
    }
    for (int s = len - 1; s >= 0; --s) {
      const int word = ch[s];
      double m[4], M[4], J[16];
      double off;
      if (s == 0) {
        double Lb[4];
        const int useed = tree_seed_edge(tt, word, msa, n_prune, pat, all_n, m, Lb);
        tree_join(A, m, M);
        // the tip table holds columns: P_u[a][c] at [c * 4 + a]
        off = sub_edge<1, 4>(M, tiptab + (size_t)useed * 16, Lb, rj, J, cc);
        if (se_part && live) sub_store16(se_part + (sr * L + site) * 16, J);
      } else {
        const int kc = tree_sibling_message(tt, word, msa, n_prune, pat, all_n, m);
        tree_join(A, m, M);
        double Lb[4];
        tree_load_clv(tt.clv_s, plane, kc, pat, Lb);
        off = sub_edge<4, 1>(M, pin + (size_t)kc * 16, Lb, rj, J, cc);
        tree_push_down(pin, kc, M, A);  // the message into v_{s-1}
      }
      if (kWriteEdges && live) sub_store16(edge_part + ((sr * P + s) * L + site) * 16, J);
      const double tot = wave_sum(live ? off : 0.0);
      if (lane == 0) load_w[s] += tot;
    }
    if (live) sub_store16(cc_part + (sr * L + site) * 16, cc);
  }
  __syncthreads();
  // the waves' partial loads in wave order (a padding slot keeps its 0)
  for (int s = tid; s <= P; s += blockDim.x) {
    double v = load[s];
#pragma unroll
    for (int w = 1; w < kSubWaves; ++w) v += load[(size_t)w * (P + 1) + s];
    el_part[sr * (P + 1) + s] = v;
  }
}

}  // namespace

size_t sub_lds_bytes(int T, int P) { return anc_lds_bytes(T) + sizeof(double) * kSubWaves * ((size_t)P + 1); }

SubWsBytes sub_ws_bytes(int L, int R, int P) {
  SubWsBytes b;
  b.cc = sizeof(double) * (size_t)R * L * 16;
  b.ne = sizeof(double) * (size_t)R * L * 20;
  b.se = sizeof(double) * (size_t)R * L * 16;
  b.el = sizeof(double) * (size_t)R * (P + 1);
  b.edge = sizeof(double) * (size_t)R * P * L * 16;
  return b;
}

void launch_sub_seed(int n, int T, int P, int seed_tip, const void* desc, int32_t* chain, int32_t* plen, int32_t* err_flag,
                     hipStream_t stream) {
  hipLaunchKernelGGL(sub_seed_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, T, P, seed_tip,
                     static_cast<const AsrOp*>(desc), chain, plen, err_flag);
}

int launch_substitutions(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                         const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                         const double* naive_prob, const int32_t* path, int P, int seed_tip, const AncWs& ws, const SubWs& sws,
                         const SubOut& out, const int4* hdr, int32_t* err_flag, hipStream_t stream) {
  const int L = fam.n_sites;
  if (n < 1 || n > 65535 || L < 1 || P < 1 || P > T - 2 || seed_tip < 1 || seed_tip > T - 1) return 1;
  const size_t lds = sub_lds_bytes(T, P);
  if (lds > 160 * 1024) return 1;
  const bool tables = out.edge || out.naive_edge || out.chain_counts || out.seed_edge || out.edge_load;
  double* rho = out.rate_post ? out.rate_post : ws.rho;
  launch_ancestral_front(fam, n, R, T, ops, pi, site_lik, site_scal, naive_prob, tables ? path : nullptr, P, ws, out.rate_post,
                         hdr, err_flag, stream);
  if (!tables) return 0;
  hipLaunchKernelGGL(sub_seed_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, T, P, seed_tip,
                     static_cast<const AsrOp*>(ws.desc), ws.chain, ws.plen, err_flag);
  auto run = [&](auto kernel, double* edge_part) {
    launch_lds(kernel, dim3(R, n), dim3(kSubWaves * 64), lds, stream, R, T, L, fam.n_prune, P, seed_tip, fam.msa,
               fam.site_pat, static_cast<const AsrOp*>(ws.desc), brlen, rates, eig, pi, ws.tvec, rho, ws.chain, ws.plen,
               reinterpret_cast<double2*>(ws.clv), (int)anc_lp(fam.n_prune), sws.cc, sws.ne,
               out.seed_edge ? sws.se : nullptr, sws.el, edge_part);
  };
  if (out.edge)
    run(sub_kernel<true>, sws.edge);
  else
    run(sub_kernel<false>, nullptr);
  const size_t l = (size_t)L;
  launch_rate_sum(n, R, P, l * 16, false, ws.plen, sws.edge, out.edge, stream);
  launch_rate_sum(n, R, 1, l * 20, false, ws.plen, sws.ne, out.naive_edge, stream);
  launch_rate_sum(n, R, 1, l * 16, false, ws.plen, sws.cc, out.chain_counts, stream);
  launch_rate_sum(n, R, 1, l * 16, false, ws.plen, sws.se, out.seed_edge, stream);
  launch_rate_sum(n, R, P + 1, 1, true, ws.plen, sws.el, out.edge_load, stream);
  return 0;
}

}  // namespace lh
