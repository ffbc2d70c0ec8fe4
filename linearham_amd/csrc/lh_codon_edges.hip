// K15: exact amino-acid replacement posteriors along the edges of a seed's lineage (gfx950).
//
// K14 (lh_node_codon.hip) gives a node's codon against the naive one; K12 (lh_substitutions.hip) gives the two ends of an
// edge per site.  Which residue was replaced on which edge needs the codon at both ends of the edge at once: a codon's three
// sites are coupled through the naive codon at both ends, and the two ends are strongly dependent.
//
// Notation of K12 / K13: path v_0 (the seed's parent) .. v_{len-1} (the root), seed tip u, tables [ancestor][descendant].
// Given the naive base b of a site everything at that site is independent of the rest of the alignment, so per pattern j
//   J_s^(b,r)(a, c) = A_s^(b,r)(a) m_s(a) P_below[a][c] L_below(c)
//   H_s[j][b][a][c] = sum_r w_r(j, b) J_s^(b,r)(a, c) / sum_{a,c} J_s^(b,r),     w_r(j, b) = lik_r(j, b) / Z_j(b)
// with A^(b) K13b's 4 x 5 block, m_s, below and the seed edge as K12b forms them.  sum_c H_s is K13's table at v_s.  For
// codon c over the sites j1 j2 j3 = frame + 3 c .. and Q K9's naive codon posterior, the joint of the codon at the two ends
// of edge s is
//   E_s[c][x][y] = sum over b in {A,C,G,T,N}^3 of Q[c][b] prod_k H_s[j_k][b_k][x_k][y_k],   x = 16 x1 + 4 x2 + x3
// and the naive edge is K14's joint at the MRCA, Q[c][b] prod_k G[j_k][b_k][y_k] with G = sum_c H_{len-1}.
// Classes of an inner edge: [0] y = x, [1] y != x with the same translation, [2] a different translation; of the naive edge
// K14's four ([3]: the naive triple holds an N).  Translation is the standard code, the stop codons a symbol of their own.
//
// Kernels:
//  * K11r, K3s, K11c (launch_ancestral_front) and K12c (launch_sub_seed) run in front, unchanged.
//  * K15b (cond_edge_kernel), a workgroup per (rate category, sample) as K13b's cond_kernel<false>: its prologue, its
//    upward pass with a lane per pattern, its category weights and its 4 x 5 block (tree_rate_weights, tree_root_messages)
//    down the chain.  Per step tree_sibling_message once (at slot 0 K12b's tree_seed_edge), then per basis the 16 cells
//    M(a) P_below(a, c) L_below(c) from tree_join's M, normalised by their sum and weighted by w_r:
//    part[sample][rate][slot][pattern][5][16].  Contraction is off in the down pass, fma is written where it is meant.
//    All of the tree pass is lh_treepass.h's; the kernel's own are the cells (cond_edge_below, cond_edge_cells).
//  * K15m (K11m's rate_sum_kernel): the R partials in rate order; NaN for a row without a path, 0 in padding slots.
//    K13's site_gather_kernel (lh_ancestral.hip) spreads the table over the sites for a caller who takes cond_edge.
//  * K15 (codon_edge_kernel), a wave per (row, codon), lane = the upper triple x of an inner edge (the MRCA's triple on
//    the naive edge).  Q is read at wave-uniform addresses, a zero entry skipped by a uniform branch.  Per non-zero b the
//    lane forms the 64 products of its three 4-vectors H[j_k][b_k][x_k][.] (an edge's 3 x 80 doubles are staged in LDS by a
//    coalesced load, the next edge's fetched while this one is contracted) and folds them into 21 register accumulators by
//    a compile-time triple -> symbol map (template indices: no private array is reached by a dynamic index; the loops over
//    b stay rolled, which keeps the kernel at two waves per SIMD).  Per edge:
//    `same` and the lane's diagonal-symbol and total masses are reduced over the wave by a fixed butterfly.  The lanes'
//    rows are folded by x -> symbol once per wave through LDS ([64][21]), each cell summed in ascending x by one lane: the
//    naive edge first, then the inner edges (whose accumulators ran over the slots len-1 .. 0).  No atomics, one fixed order.
//  * codon_edge_load_kernel, a thread per (row, edge, class): edge_change summed over the codons in order.
// A row with plen 0 or a non-finite log-likelihood gets NaN.  A row's bits do not depend on its batch.
#include <utility>

#include "lh_treepass.h"

namespace lh {

namespace {

constexpr int kSymbols = 21;

// sym[x]: the symbol 0 .. 20 (position in "ACDEFGHIKLMNPQRSTVWY*") of the triple x = 16 x1 + 4 x2 + x3 over A, C, G, T
struct CodonSymbols {
  uint8_t sym[64];
};
constexpr CodonSymbols make_symbols() {
  const char code[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";  // over T, C, A, G
  const char letters[] = "ACDEFGHIKLMNPQRSTVWY*";
  const int tcag[4] = {2, 1, 3, 0};  // A, C, G, T -> position in TCAG
  CodonSymbols t{};
  for (int x = 0; x < 64; ++x) {
    const char aa = code[tcag[x >> 4] * 16 + tcag[(x >> 2) & 3] * 4 + tcag[x & 3]];
    for (int k = 0; k < kSymbols; ++k)
      if (letters[k] == aa) t.sym[x] = (uint8_t)k;
  }
  return t;
}
constexpr CodonSymbols kSym = make_symbols();
__device__ const CodonSymbols kSymDev = make_symbols();

// What the bases of an edge share: t[a] = sum_c p[a*SA + c*SC] * Lb[c], the branch below times the likelihood below summed
// over the lower end.
template <int SA, int SC>
__device__ __forceinline__ void cond_edge_below(const double* p, const double (&Lb)[4], double (&t)[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 4; ++a)
    t[a] = (p[a * SA] * Lb[0] + p[a * SA + SC] * Lb[1]) + (p[a * SA + 2 * SC] * Lb[2] + p[a * SA + 3 * SC] * Lb[3]);
}

// The 16 cells of one basis at one edge, J(a, c) = M[a] p[a][c] Lb[c], normalised by their sum M . t and weighted by w (0
// where the sum or the weight is 0), stored at o.  (The factor of the basis goes first: nothing but p and Lb is shared by
// the bases, and the kernel keeps its three waves per SIMD.)
template <int SA, int SC>
__device__ __forceinline__ void cond_edge_cells(const double (&M)[4], const double* p, const double (&Lb)[4],
                                                const double (&t)[4], double w, bool live, double* o) {
#pragma clang fp contract(off)
  const double sum = fma(M[3], t[3], fma(M[2], t[2], fma(M[1], t[1], M[0] * t[0])));
  const double f = (sum == 0.0 || w == 0.0) ? 0.0 : w / sum;
  if (live) {
    double2* o2 = reinterpret_cast<double2*>(o);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double g = f == 0.0 ? 0.0 : f * M[a];
      o2[2 * a] = make_double2((g * p[a * SA]) * Lb[0], (g * p[a * SA + SC]) * Lb[1]);
      o2[2 * a + 1] = make_double2((g * p[a * SA + 2 * SC]) * Lb[2], (g * p[a * SA + 3 * SC]) * Lb[3]);
    }
  }
}

// K15b.  Three waves per SIMD (at most 168 vector registers) is what the five bases' cells are ordered for; the bound is
// declared because the kernel lies within a few registers of it.
__global__ void __launch_bounds__(256, 3) cond_edge_kernel(int R, int T, int n_prune, int P, const uint8_t* __restrict__ msa,
                                                        const AsrOp* __restrict__ desc, const double* __restrict__ brlen,
                                                        const double* __restrict__ rates, const double* __restrict__ eig,
                                                        const double* __restrict__ pi, const double* __restrict__ site_lik,
                                                        const int32_t* __restrict__ site_scal,
                                                        const int32_t* __restrict__ chain, const int32_t* __restrict__ plen,
                                                        double2* clv, int Lp, double* __restrict__ part) {
  extern __shared__ double2 cond_edge_smem[];
  const TreeTables tt = tree_prologue(cond_edge_smem, R, T, desc, brlen, rates, eig, plen, clv, Lp);
  const int len = tt.len;
  if (len == 0) return;  // K15m writes the row's NaN
  const int NP = n_prune + 1;
  const int sample = blockIdx.y, rate = blockIdx.x;
  const double *tiptab = tt.tiptab, *pin = tt.pin;
  const size_t plane = tt.plane;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_waves = blockDim.x >> 6;
  const double* __restrict__ p4 = pi + (size_t)sample * 4;
  const int32_t* __restrict__ ch = chain + (size_t)sample * P;
  double* part_s = part + ((size_t)sample * R + rate) * (size_t)P * NP * 80;

  for (int s0 = wave * 64; s0 < NP; s0 += n_waves * 64) {
    const bool live = s0 + lane < NP;
    const int pat = min(s0 + lane, NP - 1);
    const bool all_n = pat >= n_prune;
    {
      double root[4];  // every inner CLV is stored: the down pass reads the lane's own back
      tree_upward_pattern<true>(T - 2, n_prune, pat, msa, tt.dsc, tiptab, pin, tt.clv_s, plane, root);
    }

    // the weight of this category under each naive base
    double w[5];
    tree_rate_weights(site_scal, site_lik, sample, rate, R, n_prune, pat, all_n, w);

    // the message into the root from above, per basis vector of the naive tip
    double A[5][4];
    tree_root_messages(tiptab, p4, A);
    for (int s = len - 1; s >= 0; --s) {
#pragma clang fp contract(off)
      const int word = ch[s];
      double* o = part_s + ((size_t)s * NP + pat) * 80;
      double m[4];
      if (s == 0) {
        double Lb[4];
        const int useed = tree_seed_edge(tt, word, msa, n_prune, pat, all_n, m, Lb);
        // the tip table holds columns: P_u[a][c] at [c * 4 + a]
        const double* pu = tiptab + (size_t)useed * 16;
        double tb[4];
        cond_edge_below<1, 4>(pu, Lb, tb);
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          double M[4];
          tree_join(A[b], m, M);
          cond_edge_cells<1, 4>(M, pu, Lb, tb, w[b], live, o + b * 16);
        }
      } else {
        const int kc = tree_sibling_message(tt, word, msa, n_prune, pat, all_n, m);
        double Lb[4];
        tree_load_clv(tt.clv_s, plane, kc, pat, Lb);
        const double* pc = pin + (size_t)kc * 16;
        double tb[4];
        cond_edge_below<4, 1>(pc, Lb, tb);
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          double M[4];
          tree_join(A[b], m, M);
          cond_edge_cells<4, 1>(M, pc, Lb, tb, w[b], live, o + b * 16);
          tree_push_down(pin, kc, M, A[b]);  // the message into v_{s-1}
        }
      }
    }
  }
}

__device__ __forceinline__ double pick4(const double (&h)[4], int i) {
  return i == 0 ? h[0] : i == 1 ? h[1] : i == 2 ? h[2] : h[3];
}

__device__ __forceinline__ void load4(const double* p, double (&h)[4]) {
  const double2 lo = reinterpret_cast<const double2*>(p)[0], hi = reinterpret_cast<const double2*>(p)[1];
  h[0] = lo.x;
  h[1] = lo.y;
  h[2] = hi.x;
  h[3] = hi.y;
}

template <int X>
struct SymbolOf {
  static constexpr int value = kSym.sym[X];
};

// acc[symbol of y] += qv * (p12[y1 y2] * h3[y3]) over the 64 lower triples y, the symbol a template constant
template <int... Y>
__device__ __forceinline__ void fold_lower(double (&acc)[kSymbols], const double (&p12)[16], const double (&h3)[4], double qv,
                                           std::integer_sequence<int, Y...>) {
  ((acc[SymbolOf<Y>::value] += qv * (p12[Y >> 2] * h3[Y & 3])), ...);
}

// The naive edge's N-free terms Q[b] G1[b1][y1] G2[b2][y2] G3[b3][y3], y the lane's triple, into acc[symbol of b]; the term
// of b = y into ident.  A zero entry of Q is skipped by a uniform branch.
template <int B>
__device__ __forceinline__ void naive_term(double (&acc)[kSymbols], const double (&g)[3][5], const double* __restrict__ q,
                                           int lane, double& ident) {
  constexpr int b1 = B >> 4, b2 = (B >> 2) & 3, b3 = B & 3;
  const double qv = q[25 * b1 + 5 * b2 + b3];
  if (qv != 0.0) {
    const double term = qv * ((g[0][b1] * g[1][b2]) * g[2][b3]);
    acc[SymbolOf<B>::value] += term;
    ident += lane == B ? term : 0.0;
  }
}
template <int... B>
__device__ __forceinline__ void fold_naive(double (&acc)[kSymbols], const double (&g)[3][5], const double* __restrict__ q,
                                           int lane, double& ident, std::integer_sequence<int, B...>) {
  (naive_term<B>(acc, g, q, lane, ident), ...);
}

// v = acc[sym], sym the lane's own symbol: a chain of selects over the register accumulators
template <int... K>
__device__ __forceinline__ double pick_symbol(const double (&acc)[kSymbols], int sym, std::integer_sequence<int, K...>) {
  double v = 0.0;
  ((v = sym == K ? acc[K] : v), ...);
  return v;
}

constexpr int kCellTrips = (kSymbols * kSymbols + 63) / 64;  // 7

// One pass of the fold through LDS: the lanes' accumulator rows into tile[64][21], then cell (X, Y) of the lane's trips
// += the rows of the lanes whose symbol is X (inner edges: the lane is the upper triple, its accumulators the lower
// symbols) or, transposed, the entries X of the lanes whose symbol is Y (naive edge: the lane is the lower triple), in
// ascending lane order.
template <bool kLaneIsLower>
__device__ __forceinline__ void fold_tile(double* tile, int lane, const double (&acc)[kSymbols], double (&cell)[kCellTrips]) {
  __syncthreads();  // (one wave per workgroup: the earlier pass has been read)
#pragma unroll
  for (int k = 0; k < kSymbols; ++k) tile[lane * kSymbols + k] = acc[k];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kCellTrips; ++t) {
    const int id = min(t * 64 + lane, kSymbols * kSymbols - 1);
    const int X = id / kSymbols, Y = id - X * kSymbols;
    double v = cell[t];
    for (int x = 0; x < 64; ++x) {
      const int sx = kSymDev.sym[x];
      if (kLaneIsLower) {
        if (sx == Y) v += tile[x * kSymbols + X];
      } else {
        if (sx == X) v += tile[x * kSymbols + Y];
      }
    }
    cell[t] = v;
  }
}

// K15
__global__ void __launch_bounds__(64) codon_edge_kernel(int C, int frame, int n_prune, int P,
                                                        const int32_t* __restrict__ site_pat,
                                                        const double* __restrict__ table, const double* __restrict__ Q,
                                                        const int32_t* __restrict__ plen, const double* __restrict__ loglik,
                                                        double* __restrict__ codon_counts, double* __restrict__ aa_counts,
                                                        double* __restrict__ seed_change, double* __restrict__ edge_change) {
  __shared__ double tile[64 * kSymbols];
  __shared__ __attribute__((aligned(16))) double hbuf[3 * 80];
  const int lane = threadIdx.x;
  const int c = blockIdx.x, row = blockIdx.y;
  const size_t item = (size_t)row * C + c;
  const int NP = n_prune + 1;
  const int len = plen[row];
  double* __restrict__ cc = codon_counts ? codon_counts + item * 4 : nullptr;
  double* __restrict__ aa = aa_counts ? aa_counts + item * (kSymbols * kSymbols) : nullptr;
  double* __restrict__ sc = seed_change ? seed_change + item * 3 : nullptr;
  double* __restrict__ ec = edge_change ? edge_change + ((size_t)row * (P + 1) * C + c) * 3 : nullptr;  // + e * C * 3
  if (len == 0 || (loglik && !isfinite(loglik[row]))) {
    const double nan = __builtin_nan("");
    if (cc && lane < 4) cc[lane] = nan;
    if (sc && lane < 3) sc[lane] = nan;
    if (aa)
      for (int i = lane; i < kSymbols * kSymbols; i += 64) aa[i] = nan;
    if (ec)
      for (int i = lane; i < (P + 1) * 3; i += 64) ec[(size_t)(i / 3) * C * 3 + i % 3] = nan;
    return;
  }
  const int x1 = lane >> 4, x2 = (lane >> 2) & 3, x3 = lane & 3;
  const int my_sym = kSymDev.sym[lane];
  int pat[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) pat[k] = min(site_pat[frame + 3 * c + k], n_prune);
  const double* __restrict__ q = Q + item * 125;  // wave-uniform
  const double* __restrict__ tab = table + (size_t)row * P * NP * 80;
  constexpr auto all64 = std::make_integer_sequence<int, 64>{};
  constexpr auto all21 = std::make_integer_sequence<int, kSymbols>{};
  double cell[kCellTrips];
#pragma unroll
  for (int t = 0; t < kCellTrips; ++t) cell[t] = 0.0;
  double n_same = 0.0, n_syn = 0.0, n_repl = 0.0;  // the codon's counts over the edges, naive to seed

  // An edge's H of the codon's three patterns, 3 x 80 doubles, goes through LDS: lanes 0 .. 59 fetch four doubles each
  // (coalesced per pattern), the next edge's while this one is contracted, so the lanes' reads in the loops below are LDS
  // reads at no global latency.
  const int fk = min(lane / 20, 2), foff = (lane % 20) * 4;
  const double* __restrict__ fsrc = tab + (size_t)min(site_pat[frame + 3 * c + fk], n_prune) * 80 + foff;
  const size_t slot_stride = (size_t)NP * 80;
  double nx[4];
  if (lane < 60) {
    load4(fsrc + (size_t)(len - 1) * slot_stride, nx);
    double2* h2 = reinterpret_cast<double2*>(hbuf + fk * 80 + foff);
    h2[0] = make_double2(nx[0], nx[1]);
    h2[1] = make_double2(nx[2], nx[3]);
  }
  __syncthreads();
  const double* r1 = hbuf + x1 * 4;
  const double* r2 = hbuf + 80 + x2 * 4;
  const double* r3 = hbuf + 160 + x3 * 4;

  {
    // ---- the naive edge: K14's joint at the MRCA, the lane its triple y; G[k][b] = sum_c H_{len-1}[j_k][b][y_k][c]
    double g[3][5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* rk = k == 0 ? r1 : k == 1 ? r2 : r3;
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        double h[4];
        load4(rk + b * 16, h);
        g[k][b] = (h[0] + h[1]) + (h[2] + h[3]);
      }
    }
    double acc[kSymbols];  // by the symbol of the naive triple
#pragma unroll
    for (int k = 0; k < kSymbols; ++k) acc[k] = 0.0;
    double ident = 0.0, open = 0.0;
#pragma unroll
    for (int b1 = 0; b1 < 5; ++b1)
#pragma unroll
      for (int b2 = 0; b2 < 5; ++b2)
#pragma unroll
        for (int b3 = 0; b3 < 5; ++b3)
          if (b1 == 4 || b2 == 4 || b3 == 4) open += q[25 * b1 + 5 * b2 + b3];  // (uniform: the same sum in every lane)
    fold_naive(acc, g, q, lane, ident, all64);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < kSymbols; ++k) total += acc[k];
    const double diag = pick_symbol(acc, my_sym, all21);
    ident = wave_sum(ident);
    const double syn = wave_sum(diag) - ident, repl = wave_sum(total - diag);
    n_same += ident;
    n_syn += syn;
    n_repl += repl;
    if (ec && lane == 0) {
      double* o = ec + (size_t)P * C * 3;
      o[0] = ident;
      o[1] = syn;
      o[2] = repl;
    }
    if (cc && lane == 0) cc[3] = open;
    if (aa) fold_tile<true>(tile, lane, acc, cell);
  }

  // ---- the inner edges and the seed edge, the lane the upper triple x
  double acc[kSymbols];  // by the symbol of the lower triple, over the slots
#pragma unroll
  for (int k = 0; k < kSymbols; ++k) acc[k] = 0.0;
  for (int s = len - 1; s >= 0; --s) {
    if (s > 0 && lane < 60) load4(fsrc + (size_t)(s - 1) * slot_stride, nx);  // the next edge's, used behind the barrier below
    double e[kSymbols];  // this edge's
#pragma unroll
    for (int k = 0; k < kSymbols; ++k) e[k] = 0.0;
    double same = 0.0;
#pragma unroll 1  // (the 125 bases as loops: a fraction of the code and of the registers of their unrolled form)
    for (int b1 = 0; b1 < 5; ++b1) {
      double h1[4];
      load4(r1 + b1 * 16, h1);
#pragma unroll 1
      for (int b2 = 0; b2 < 5; ++b2) {
        const double* __restrict__ q5 = q + 25 * b1 + 5 * b2;
        if (q5[0] == 0.0 && q5[1] == 0.0 && q5[2] == 0.0 && q5[3] == 0.0 && q5[4] == 0.0) continue;  // (uniform)
        double h2[4], p12[16];
        load4(r2 + b2 * 16, h2);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) p12[i * 4 + j] = h1[i] * h2[j];
        const double d12 = pick4(h1, x1) * pick4(h2, x2);
#pragma unroll 1
        for (int b3 = 0; b3 < 5; ++b3) {
          const double qv = q5[b3];
          if (qv != 0.0) {
            double h3[4];
            load4(r3 + b3 * 16, h3);
            fold_lower(e, p12, h3, qv, all64);
            same += qv * (d12 * pick4(h3, x3));
          }
        }
      }
    }
    __syncthreads();  // every lane has read this edge's H
    if (s > 0 && lane < 60) {
      double2* h2 = reinterpret_cast<double2*>(hbuf + fk * 80 + foff);
      h2[0] = make_double2(nx[0], nx[1]);
      h2[1] = make_double2(nx[2], nx[3]);
    }
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < kSymbols; ++k) {
      total += e[k];
      acc[k] += e[k];
    }
    const double diag = pick_symbol(e, my_sym, all21);
    same = wave_sum(same);
    const double syn = wave_sum(diag) - same, repl = wave_sum(total - diag);
    n_same += same;
    n_syn += syn;
    n_repl += repl;
    if (lane == 0) {
      if (ec) {
        double* o = ec + (size_t)s * C * 3;
        o[0] = same;
        o[1] = syn;
        o[2] = repl;
      }
      if (sc && s == 0) {
        sc[0] = same;
        sc[1] = syn;
        sc[2] = repl;
      }
    }
  }
  if (ec && lane < 3)
    for (int s = len; s < P; ++s) ec[(size_t)s * C * 3 + lane] = 0.0;  // padding slots
  if (cc && lane == 0) {
    cc[0] = n_same;
    cc[1] = n_syn;
    cc[2] = n_repl;
  }
  if (aa) {
    fold_tile<false>(tile, lane, acc, cell);
#pragma unroll
    for (int t = 0; t < kCellTrips; ++t)
      if (t * 64 + lane < kSymbols * kSymbols) aa[t * 64 + lane] = cell[t];
  }
}

// edge_load[n][P+1][2] = sum over the codons, in order, of edge_change[n][P+1][C][1 .. 2]
__global__ void __launch_bounds__(256) codon_edge_load_kernel(long long total, int C, const double* __restrict__ edge_change,
                                                              double* __restrict__ edge_load) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const long long e = gid >> 1;  // row * (P + 1) + edge
  const int k = (int)(gid & 1);
  const double* __restrict__ p = edge_change + (size_t)e * C * 3 + 1 + k;
  double v = 0.0;
  for (int c = 0; c < C; ++c) v += p[(size_t)c * 3];
  edge_load[gid] = v;
}

}  // namespace

void codon_edge_symbols(uint8_t* out) {
  for (int x = 0; x < 64; ++x) out[x] = kSym.sym[x];
}

CondEdgeWsBytes cond_edge_ws_bytes(int R, int n_prune, int P) {
  const size_t t = sizeof(double) * (size_t)P * (n_prune + 1) * 80;
  return {t * R, t};
}

int launch_cond_edges(const DevFamily& fam, int n, int R, int T, const int32_t* ops, const double* brlen, const double* rates,
                      const double* eig, const double* pi, const double* site_lik, const int32_t* site_scal,
                      const double* naive_prob, const int32_t* path, int P, int seed_tip, const AncWs& ws, double* table,
                      double* cond_edge, const int4* hdr, int32_t* err_flag, hipStream_t stream) {
  const int L = fam.n_sites, NP = fam.n_prune + 1;
  if (n < 1 || n > 65535 || L < 1 || P < 1 || P > T - 2 || seed_tip < 1 || seed_tip > T - 1) return 1;
  const size_t lds = anc_lds_bytes(T);
  if (lds > 160 * 1024) return 1;
  launch_ancestral_front(fam, n, R, T, ops, pi, site_lik, site_scal, naive_prob, path, P, ws, nullptr, hdr, err_flag, stream);
  launch_sub_seed(n, T, P, seed_tip, ws.desc, ws.chain, ws.plen, err_flag, stream);
  launch_lds(cond_edge_kernel, dim3(R, n), dim3(256), lds, stream, R, T, fam.n_prune, P, fam.msa,
             static_cast<const AsrOp*>(ws.desc), brlen, rates, eig, pi, site_lik, site_scal, ws.chain, ws.plen,
             reinterpret_cast<double2*>(ws.clv), (int)anc_lp(fam.n_prune), ws.part);
  launch_rate_sum(n, R, P, (size_t)NP * 80, false, ws.plen, ws.part, table, stream);
  if (cond_edge) launch_site_gather(fam, (long long)n * P, 80, table, cond_edge, stream);
  return 0;
}

void launch_codon_edges(const DevFamily& fam, int n, int n_codons, int frame, int P, const double* table, const double* Q,
                        const int32_t* plen, const double* loglik, double* codon_counts, double* aa_counts,
                        double* seed_change, double* edge_change, double* edge_load, hipStream_t stream) {
  if (n < 1 || n_codons < 1 || (!codon_counts && !aa_counts && !seed_change && !edge_change)) return;
  hipLaunchKernelGGL(codon_edge_kernel, dim3(n_codons, n), dim3(64), 0, stream, n_codons, frame, fam.n_prune, P,
                     fam.site_pat, table, Q, plen, loglik, codon_counts, aa_counts, seed_change, edge_change);
  if (edge_load && edge_change) {
    const long long total = (long long)n * (P + 1) * 2;
    hipLaunchKernelGGL(codon_edge_load_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, n_codons,
                       edge_change, edge_load);
  }
}

}  // namespace lh
