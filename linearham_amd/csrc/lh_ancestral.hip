// K11: exact ancestral-state marginals along a seed's lineage (gfx950).
//
// What K3 (lh_asr.hip) draws and K7 counts, as probabilities: for every node v_s of the lineage path (slot 0 = the seed's
// parent, the last slot = the root, naive's neighbour) and every alignment site j
//   marg[s][j][c] = P(x_{v_s, j} = c | data) = sum_b q_j(b) sum_r [lik_r(j, b) / Z_j(b)] P(x = c | column j, naive_j = b, rate r),
// q_j = the posterior of the naive base (a one-hot row conditions on a fixed naive sequence, K3's setting), lik_r = K1's
// unmixed per-rate planes, Z_j(b) = sum_r lik_r(j, b).  The joint P(x = c, column | b, r) is linear in the naive tip's
// vector, so with t_j(b) = q_j(b) / Z_j(b) one down pass per (site, rate) serves all five naive bases:
//   rho_r(j) = sum_b t_j(b) lik_r(j, b)                                   the rate posterior (sums to 1 over r)
//   A_{P-1}(i) = pi_i (sum_{b<4} P_naive[i][b] t_j(b) + t_j(N) rowsum_i)  the message into the root from above
//   post_s(c) = A_s(c) L_{v_s}(c)
//   A_{s-1}(c) = sum_i A_s(i) (P_{w_s} L_{w_s})(i) P_{v_{s-1}}[i][c]      w_s = the child of v_s off the path
//   marg[s][j][c] = sum_r rho_r(j) post_s^(r)(c) / sum_c' post_s^(r)(c')
// Normalising per (slot, site, rate) before the weighting makes the result independent of every rescaling of the CLVs.
//
// Kernels:
//  * K11a (site_base_kernel), a thread per (sample, site): K5's posterior (compact forward layout) pushed onto (site, base).
//    Every compact entry writes its naive base on its sites (a germline gene on all of its sites, a junction entry on its
//    row's site); the table, built once per family, lists per (site, base) the entries that write it, in ascending order,
//    so a cell is a sum in a fixed order.  What no state writes stays N: N takes 1 - (the five sums).  A row without a
//    posterior (non-finite log-likelihood) is NaN.
//  * K11r (anc_rate_kernel), a thread per (sample, site): t_j[5] and rho_j[R] from the planes, scaler counts aligned to the
//    smallest (RatePlanes, lh_treepass.h).
//  * K3s (lh_asr.hip) writes the schedule descriptors; K11c (anc_chain_kernel), a workgroup per sample, checks the path against
//    them -- entries outside T .. 2T-3 are padding and come last, each entry is a child of the next, the last one is the
//    root -- and writes per slot the op that produced the node and which of that op's children continues the path.  No index
//    is formed from a path entry before it is checked.  A path that fails leaves length 0: the sample's row is NaN and the
//    handle's error word is raised.
//  * K11b (anc_kernel), a workgroup per (rate category, sample) so that P-matrices are wave-uniform: K3b's LDS tables (tip
//    table, inner P-matrices by op), K3b's upward pass over ALL site patterns of the family (a lane per pattern, every
//    inner CLV stored: clv[sample][rate][op][2][pattern] of 16-byte entries), then the downward pass along the path, a lane
//    per site: P mat-vecs, not T - 2.  The message from above is divided by its largest entry after every step.  The lane
//    writes rho_r * post / sum into part[sample][rate][slot][site][4].  The kernel's prologue (tables, CLV area), the
//    upward pass and the step down the lineage (sibling message, descent) are lh_treepass.h's, shared with K12b and K13b;
//    the message into the root is written here (its sum may be contracted, and is in this kernel).
//  * K11m (rate_sum_kernel, launch_rate_sum), a thread per output cell: the R partial tables added in rate order -- fixed
//    order, no atomics, the same bits whatever the batch.  K12 and K13 sum their partial tables with the same kernel.
// No private array is reached by a dynamic index: 4-vectors are indexed by unrolled loops only.
#include "lh_treepass.h"

namespace lh {

namespace {

// K11a
__global__ void __launch_bounds__(256) site_base_kernel(int n, int L, size_t forward_size, const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ idx, const double* __restrict__ post,
                                                        const double* __restrict__ loglik, double* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)n * L) return;
  const int sample = (int)(gid / L), j = (int)(gid - (long long)sample * L);
  double* __restrict__ o = out + (size_t)gid * 5;
  if (!isfinite(loglik[sample])) {
#pragma unroll
    for (int b = 0; b < 5; ++b) o[b] = __builtin_nan("");
    return;
  }
  const double* __restrict__ p = post + (size_t)sample * forward_size;
  const int32_t* __restrict__ oj = off + (size_t)j * 5;
  double s[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    double acc = 0.0;
    for (int x = oj[b]; x < oj[b + 1]; ++x) acc += p[idx[x]];
    s[b] = acc;
  }
  s[4] += 1.0 - ((((s[0] + s[1]) + s[2]) + s[3]) + s[4]);
#pragma unroll
  for (int b = 0; b < 5; ++b) o[b] = s[b];
}

// The two slots that mean the same in every tree, for the weighted reduction: ends[sample][0] = slot 0 (the seed's parent),
// ends[sample][1] = the sample's last slot (the MRCA); and the log-likelihood the weights are formed from, NaN for a
// sample without a path, so that its NaN row is left out.
__global__ void __launch_bounds__(256) anc_ends_kernel(int n, int P, int L, const int32_t* __restrict__ plen,
                                                       const double* __restrict__ marg, const double* __restrict__ loglik,
                                                       double* __restrict__ ends, double* __restrict__ ll_used) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = 2ll * L * 4;
  if (gid >= (long long)n * per) return;
  const int sample = (int)(gid / per);
  const int cell = (int)(gid - (long long)sample * per);
  const int which = cell / (L * 4), rest = cell - which * (L * 4);
  const int len = plen[sample];
  const int slot = which == 0 ? 0 : max(len - 1, 0);
  if (ends) ends[gid] = marg[((size_t)sample * P + slot) * L * 4 + rest];
  if (cell == 0) ll_used[sample] = len == 0 ? __builtin_nan("") : loglik[sample];
}

// K11r.  t = q / Z where q != 0 (a NaN q stays NaN), 0 where q == 0 -- also where Z == 0.
__global__ void __launch_bounds__(256) anc_rate_kernel(int n, int R, int L, int n_prune, const int32_t* __restrict__ site_pat,
                                                       const double* __restrict__ site_lik,
                                                       const int32_t* __restrict__ site_scal,
                                                       const double* __restrict__ naive_prob,
                                                       const double* __restrict__ pi, double* __restrict__ tvec,
                                                       double* __restrict__ rho) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)n * L) return;
  const int sample = (int)(gid / L), j = (int)(gid - (long long)sample * L);
  const int pat = site_pat[j];
  const double* __restrict__ q = naive_prob + (size_t)gid * 5;
  double* __restrict__ t_out = tvec + (size_t)gid * 5;
  double* __restrict__ r_out = rho + (size_t)gid * R;
  double t[5];
  if (pat >= n_prune) {
    // all-N column: K1 has no plane for it.  In the planes' units (sum_i pi_i L_root(i) P_naive[i][b], L_root all ones) its
    // likelihood is pi_b under a naive base b, by stationarity, and sum_i pi_i under N (1 up to the digits pi was given
    // with), whatever the category.
    const double* __restrict__ p4 = pi + (size_t)sample * 4;
    const double psum = ((p4[0] + p4[1]) + p4[2]) + p4[3];
    double total = 0.0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      const double qb = q[b];
      t[b] = qb == 0.0 ? 0.0 : qb / ((double)R * (b < 4 ? p4[b] : psum));
      total += qb == 0.0 ? 0.0 : qb / (double)R;
    }
#pragma unroll
    for (int b = 0; b < 5; ++b) t_out[b] = t[b];
    for (int k = 0; k < R; ++k) r_out[k] = total;
    return;
  }
  const RatePlanes planes = rate_planes(site_scal, site_lik, sample, R, n_prune, pat);
  double z[5];
  planes.totals(R, z);
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    const double qb = q[b];
    t[b] = qb == 0.0 ? 0.0 : qb / z[b];
    t_out[b] = t[b];
  }
  for (int k = 0; k < R; ++k) {
    double v[5];
    planes.values(k, v);
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 5; ++b)
      if (t[b] != 0.0) acc += t[b] * v[b];
    r_out[k] = acc;
  }
}

// K11c.  chain[sample][s] = op that produced v_s | (1 << 30 if v_{s-1} is the child that op popped, else its accumulator
// child); plen[sample] = the path's length, 0 if the sample has no valid path (or K0c rejected its schedule).
__global__ void __launch_bounds__(64) anc_chain_kernel(int T, int P, const AsrOp* __restrict__ desc,
                                                       const int4* __restrict__ hdr, const int32_t* __restrict__ path,
                                                       int32_t* __restrict__ chain, int32_t* __restrict__ plen,
                                                       int32_t* err_flag) {
  extern __shared__ int32_t chain_smem[];
  const int sample = blockIdx.x, tid = threadIdx.x, n_ops = T - 2;
  if (hdr[sample].w != 0) {  // (K0c has raised the error word)
    if (tid == 0) plen[sample] = 0;
    return;
  }
  int32_t* op_of_node = chain_smem;  // [n_ops]
  const AsrOp* __restrict__ dsc = desc + (size_t)sample * n_ops;
  for (int k = tid; k < n_ops; k += blockDim.x) op_of_node[k] = -1;
  __syncthreads();
  for (int k = tid; k < n_ops; k += blockDim.x) {
    const int z = dsc[k].b.z;
    if (z >= 0 && z < n_ops) op_of_node[z] = k;
  }
  __syncthreads();
  if (tid != 0) return;
  const int32_t* __restrict__ p = path + (size_t)sample * P;
  int32_t* __restrict__ ch = chain + (size_t)sample * P;
  bool ok = true, ended = false;
  int len = 0;
  for (int s = 0; s < P; ++s) {
    const int v = p[s];
    if (v < T || v > 2 * T - 3)
      ended = true;
    else if (ended)
      ok = false;
    else
      ++len;
  }
  ok = ok && len >= 1;
  int prev = -1;
  for (int s = 0; s < len && ok; ++s) {
    const int k = op_of_node[p[s] - T];
    if (k < 0) {
      ok = false;
      break;
    }
    int word = k;
    if (s > 0) {
      const int4 a = dsc[k].a;
      const int kind = a.x & 15;
      if (kind != OP_CHERRY && prev == k - 1) {
      } else if (kind == OP_POP_ACC && a.w == prev) {
        word |= 1 << 30;
      } else {
        ok = false;
      }
    }
    ch[s] = word;
    prev = k;
  }
  ok = ok && prev == n_ops - 1;  // the last entry is the root
  plen[sample] = ok ? len : 0;
  if (!ok) atomicOr(err_flag, 2);  // bit 1: a path, bit 0: a schedule (K0c)
}

// K11b
__global__ void __launch_bounds__(256) anc_kernel(int R, int T, int L, int n_prune, int P, const uint8_t* __restrict__ msa,
                                                  const int32_t* __restrict__ site_pat, const AsrOp* __restrict__ desc,
                                                  const double* __restrict__ brlen, const double* __restrict__ rates,
                                                  const double* __restrict__ eig, const double* __restrict__ pi,
                                                  const double* __restrict__ tvec, const double* __restrict__ rho,
                                                  const int32_t* __restrict__ chain, const int32_t* __restrict__ plen,
                                                  double2* clv, int Lp, double* __restrict__ part) {
  extern __shared__ double2 anc_smem[];
  const TreeTables tt = tree_prologue(anc_smem, R, T, desc, brlen, rates, eig, plen, clv, Lp);
  const int len = tt.len;
  if (len == 0) return;  // K11m writes the row's NaN
  const int sample = blockIdx.y, rate = blockIdx.x;
  const double* tiptab = tt.tiptab;
  const size_t plane = tt.plane;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_waves = blockDim.x >> 6;

  // ---- upward pass, a lane per pattern
  tree_upward(T - 2, n_prune, msa, tt.dsc, tiptab, tt.pin, tt.clv_s, plane, wave, n_waves, lane);
  // the sites' lanes below read CLVs that other lanes and waves of this workgroup stored above
  __threadfence_block();
  __syncthreads();

  // ---- downward pass along the path, a lane per site
  const double* __restrict__ p4 = pi + (size_t)sample * 4;
  const int32_t* __restrict__ ch = chain + (size_t)sample * P;
  double* part_s = part + ((size_t)sample * R + rate) * (size_t)P * L * 4;
  for (int s0 = wave * 64; s0 < L; s0 += n_waves * 64) {
    const bool live = s0 + lane < L;
    const int site = min(s0 + lane, L - 1);
    const int pat = min(site_pat[site], n_prune);
    const bool all_n = pat >= n_prune;
    const double* __restrict__ tj = tvec + ((size_t)sample * L + site) * 5;
    const double rj = rho[((size_t)sample * L + site) * R + rate];
    double A[4];
    {
      double n4[4];
      tree_tip_col(tiptab, 0, 4, n4);
      const double t0 = tj[0], t1 = tj[1], t2 = tj[2], t3 = tj[3], t4 = tj[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        A[i] = p4[i] * (t0 * tiptab[i] + t1 * tiptab[4 + i] + t2 * tiptab[8 + i] + t3 * tiptab[12 + i] + t4 * n4[i]);
    }
    for (int s = len - 1; s >= 0; --s) {
      const int word = ch[s];
      double c[4];
      tree_load_clv(tt.clv_s, plane, chain_op(word), pat, c);
      const double post[4] = {A[0] * c[0], A[1] * c[1], A[2] * c[2], A[3] * c[3]};
      const double sum = (post[0] + post[1]) + (post[2] + post[3]);
      // a category with rho = 0 or an all-zero post contributes 0, not NaN
      const double f = (sum == 0.0 || rj == 0.0) ? 0.0 : rj / sum;
      if (live) {
        double2* o = reinterpret_cast<double2*>(part_s + ((size_t)s * L + site) * 4);
        o[0] = make_double2(f == 0.0 ? 0.0 : f * post[0], f == 0.0 ? 0.0 : f * post[1]);
        o[1] = make_double2(f == 0.0 ? 0.0 : f * post[2], f == 0.0 ? 0.0 : f * post[3]);
      }
      if (s == 0) break;
      // the message into v_{s-1}: the sibling off the path times the message from above, through v_{s-1}'s branch
      double m[4];
      const int kc = tree_sibling_message(tt, word, msa, n_prune, pat, all_n, m);
      tree_descend(tt.pin, kc, m, A);
    }
  }
}

// K11m, K12m, K13m.  part[n][R][slots][width], out[n][slots][width]; slot s of a sample is live if s < plen, or if it is
// the last and last_live (edge_load's naive edge).
__global__ void __launch_bounds__(256) rate_sum_kernel(int n, int R, int slots, long long width, bool last_live,
                                                       const int32_t* __restrict__ plen, const double* __restrict__ part,
                                                       double* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)slots * width;
  if (gid >= (long long)n * per) return;
  const int sample = (int)(gid / per);
  const long long cell = gid - (long long)sample * per;
  const int s = (int)(cell / width);
  const int len = plen[sample];
  double v = 0.0;
  if (len == 0) {
    v = __builtin_nan("");
  } else if (s < len || (last_live && s == slots - 1)) {
    // (unrolled: four categories' loads in flight per thread, the sum still in rate order; with one 8-byte load in flight
    // the kernel was 10 % slower on K11's tables, profiles/r22_treepass_shared.txt)
#pragma unroll 4
    for (int k = 0; k < R; ++k) v += part[((size_t)sample * R + k) * per + cell];
  }
  out[gid] = v;
}

// out[rows][L][2 W2] from table[rows][n_prune + 1][2 W2], a thread per double2 of the output (W2 a constant: the index
// arithmetic divides by it)
template <int W2>
__global__ void __launch_bounds__(256) site_gather_kernel(long long total, int L, int n_prune,
                                                          const int32_t* __restrict__ site_pat,
                                                          const double* __restrict__ table, double* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const long long cell = gid / W2;  // (row, site)
  const int q = (int)(gid - cell * W2);
  const long long row = cell / L;
  const int site = (int)(cell - row * L);
  const int pat = min(site_pat[site], n_prune);
  reinterpret_cast<double2*>(out)[gid] = reinterpret_cast<const double2*>(table)[(row * (n_prune + 1) + pat) * W2 + q];
}

}  // namespace

void launch_rate_sum(int n, int R, int slots, size_t width, bool last_live, const int32_t* plen, const double* part,
                     double* out, hipStream_t stream) {
  if (!out) return;
  const long long cells = (long long)n * slots * (long long)width;
  hipLaunchKernelGGL(rate_sum_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, n, R, slots,
                     (long long)width, last_live, plen, part, out);
}

void launch_site_gather(const DevFamily& fam, long long rows, int width, const double* table, double* out,
                        hipStream_t stream) {
  const long long total = rows * fam.n_sites * (width / 2);
  auto run = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, fam.n_sites, fam.n_prune,
                       fam.site_pat, table, out);
  };
  if (width == 20)
    run(site_gather_kernel<10>);  // K13's cond
  else
    run(site_gather_kernel<40>);  // K15's cond_edge
}

size_t anc_lp(int n_prune) { return ((size_t)n_prune + 1 + 7) & ~(size_t)7; }

void launch_site_base(int n, int L, size_t forward_size, const int32_t* off, const int32_t* idx, const double* post,
                      const double* loglik, double* site_base, hipStream_t stream) {
  const long long cells = (long long)n * L;
  hipLaunchKernelGGL(site_base_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, n, L, forward_size, off,
                     idx, post, loglik, site_base);
}

void launch_ancestral_ends(int n, int P, int L, const int32_t* plen, const double* marg, const double* loglik, double* ends,
                           double* ll_used, hipStream_t stream) {
  const long long cells = (long long)n * 2 * L * 4;
  hipLaunchKernelGGL(anc_ends_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, n, P, L, plen, marg, loglik,
                     ends, ll_used);
}

size_t anc_lds_bytes(int T) { return ((size_t)T + (size_t)(T - 2)) * 16 * sizeof(double); }

AncWsBytes anc_ws_bytes(int T, int L, int R, int n_prune, int P) {
  AncWsBytes b;
  b.clv = sizeof(double2) * (size_t)R * (T - 2) * 2 * anc_lp(n_prune);
  b.part = sizeof(double) * (size_t)R * P * L * 4;
  b.tvec = sizeof(double) * (size_t)L * 5;
  b.rho = sizeof(double) * (size_t)L * R;
  b.chain = sizeof(int32_t) * (size_t)P;
  return b;
}

void launch_ancestral_front(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* pi,
                            const double* site_lik, const int32_t* site_scal, const double* naive_prob, const int32_t* path,
                            int P, const AncWs& ws, double* rate_post, const int4* hdr, int32_t* err_flag, hipStream_t stream) {
  const int L = fam.n_sites;
  double* rho = rate_post ? rate_post : ws.rho;
  const long long cells = (long long)n * L;
  hipLaunchKernelGGL(anc_rate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, n, R, L, fam.n_prune,
                     fam.site_pat, site_lik, site_scal, naive_prob, pi, ws.tvec, rho);
  if (!path) return;
  launch_asr_sched(n, T, ops, hdr, ws.desc, stream);
  hipLaunchKernelGGL(anc_chain_kernel, dim3(n), dim3(64), sizeof(int32_t) * (size_t)(T - 2), stream, T, P,
                     static_cast<const AsrOp*>(ws.desc), hdr, path, ws.chain, ws.plen, err_flag);
}

int launch_ancestral(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                     const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                     const double* naive_prob, const int32_t* path, int P, const AncWs& ws, double* marg, double* rate_post,
                     const int4* hdr, int32_t* err_flag, hipStream_t stream) {
  const int L = fam.n_sites;
  if (n < 1 || n > 65535 || L < 1 || P < 1) return 1;  // (one grid row per sample)
  const size_t lds = anc_lds_bytes(T);
  if (lds > 160 * 1024) return 1;
  double* rho = rate_post ? rate_post : ws.rho;
  launch_ancestral_front(fam, n, R, T, ops, pi, site_lik, site_scal, naive_prob, marg ? path : nullptr, P, ws, rate_post, hdr,
                         err_flag, stream);
  if (!marg) return 0;
  launch_lds(anc_kernel, dim3(R, n), dim3(256), lds, stream, R, T, L, fam.n_prune, P, fam.msa, fam.site_pat,
             static_cast<const AsrOp*>(ws.desc), brlen, rates, eig, pi, ws.tvec, rho, ws.chain, ws.plen,
             reinterpret_cast<double2*>(ws.clv), (int)anc_lp(fam.n_prune), ws.part);
  launch_rate_sum(n, R, P, (size_t)L * 4, false, ws.plen, ws.part, marg, stream);
  return 0;
}

}  // namespace lh
