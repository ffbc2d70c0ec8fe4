// The tree pass that K3 (lh_asr.hip), K11 (lh_ancestral.hip), K12 (lh_substitutions.hip), K13 (lh_ancestral_probs.hip),
// K14 (K13b's table, lh_node_codon.hip) and K15 (lh_codon_edges.hip) run on, defined once and inlined into each kernel: the
// 4-vector helpers, the per-rate planes' weights, the LDS tables of a (sample, rate), the upward pass over patterns into a
// [op][2][plane] CLV area, one step down a seed's lineage, the seed edge at slot 0 (K12b, K15b) and what the kernels that
// condition on the naive base share (K13b, K15b): a category's weight under each naive base and the five messages into the
// root.
//
// Floating-point contraction is lexical, so everything here is compiled under the compiler's default whoever calls it; the
// down passes of K12b and K15b run with contraction off.  Hence only contraction-neutral arithmetic lives here: selects,
// single multiplications, one division, fma written out, sums of loaded values.  The seed edge stood inside the
// contraction-off region of both its kernels before it came here; being neutral, it compiles to the same arithmetic
// outside.  An expression a kernel's setting could fuse (K11b's and K12b's message into the root) stays in the kernel.
// No private array is reached by a dynamic index: the 4-vectors are indexed by unrolled loops only.
#pragma once

#include "lh_device.h"

namespace lh {

// a plane value whose scaler count lies d above the site's smallest, on that one's scale
__device__ static __forceinline__ double tree_aligned(double v, int d) {
  for (int q = 0; q < d && v != 0.0; ++q) v *= kScaleThreshold;
  return v;
}

// K1's unmixed planes of one (sample, pattern) across the R categories: lik_k(b) at lk[(k * 5 + b) * n_prune], its scaler
// count at sc[k * n_prune].  Values are read on the scale of the smallest count (the arithmetic of K2a's mixture).
struct RatePlanes {
  const int32_t* sc;
  const double* lk;
  int n_prune, smin;
  __device__ __forceinline__ double value(int k, int b) const {
    return tree_aligned(lk[((size_t)k * 5 + b) * n_prune], sc[(size_t)k * n_prune] - smin);
  }
  __device__ __forceinline__ void values(int k, double (&v)[5]) const {
    const int d = sc[(size_t)k * n_prune] - smin;
#pragma unroll
    for (int b = 0; b < 5; ++b) v[b] = tree_aligned(lk[((size_t)k * 5 + b) * n_prune], d);
  }
  // z[b] = sum_k lik_k(b), in rate order
  __device__ __forceinline__ void totals(int R, double (&z)[5]) const {
#pragma unroll
    for (int b = 0; b < 5; ++b) z[b] = 0.0;
    for (int k = 0; k < R; ++k) {
      double v[5];
      values(k, v);
#pragma unroll
      for (int b = 0; b < 5; ++b) z[b] += v[b];
    }
  }
};

// pat < n_prune: K1 has no plane for the all-N pattern
__device__ static __forceinline__ RatePlanes rate_planes(const int32_t* __restrict__ site_scal,
                                                         const double* __restrict__ site_lik, int sample, int R, int n_prune,
                                                         int pat) {
  RatePlanes p;
  p.sc = site_scal + (size_t)sample * R * n_prune + pat;
  p.lk = site_lik + (size_t)sample * R * 5 * n_prune + pat;
  p.n_prune = n_prune;
  p.smin = 0x7fffffff;
  for (int k = 0; k < R; ++k) p.smin = min(p.smin, p.sc[(size_t)k * n_prune]);
  return p;
}

__device__ static __forceinline__ void tree_tip_col(const double* tiptab, int tip, int st, double (&c)[4]) {
  const double* t = tiptab + tip * 16;
  if (st < 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = t[st * 4 + i];
  } else {  // N: row sums of P
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = ((t[i] + t[4 + i]) + t[8 + i]) + t[12 + i];
  }
}

// x = P a, P row-major in LDS at a wave-uniform address
__device__ static __forceinline__ void tree_matvec(const double* p, const double (&a)[4], double (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = fma(p[i * 4 + 3], a[3], fma(p[i * 4 + 2], a[2], fma(p[i * 4 + 1], a[1], p[i * 4] * a[0])));
}

// x = a^T P
__device__ static __forceinline__ void tree_vecmat(const double* p, const double (&a)[4], double (&x)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) x[c] = fma(p[12 + c], a[3], fma(p[8 + c], a[2], fma(p[4 + c], a[1], p[c] * a[0])));
}

// The 2^256 rescaling of an upward CLV after an op, until the largest entry is back at or above 2^-256 (rescale_steps;
// the tree passes normalise per node, so no count is kept).
__device__ static __forceinline__ void tree_rescale(double (&a)[4]) {
  const double top = fmax(fmax(a[0], a[1]), fmax(a[2], a[3]));
  if (__builtin_expect(top < kScaleThreshold, 0)) {
    const int n = rescale_steps((unsigned)__double2hiint(top));
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = ldexp(a[q], n << 8);
  }
}

// The LDS tables of a (sample, rate): tiptab[T][4][4] columns of the tip branches' P (the K1 tip table), pin[T-2][4][4]
// row-major P of the inner branches, by the op that produced the child (entry T-3 unused).  The caller synchronises the
// workgroup behind it.
__device__ static __forceinline__ void tree_fill_tables(int T, const AsrOp* __restrict__ dsc, const double* __restrict__ e,
                                                        const double* __restrict__ bl, double rt, double* tiptab, double* pin) {
  const int n_ops = T - 2;
  double Pm[4][4];
  for (int j = threadIdx.x; j < T + n_ops - 1; j += blockDim.x) {
    if (j < T) {
      compute_pmatrix(e, bl[j] * rt, Pm);
      double* o = tiptab + j * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int st = 0; st < 4; ++st) o[st * 4 + i] = Pm[i][st];
    } else {
      const int k = j - T;  // op k < n_ops - 1 produced inner node T + b.z, whose branch this is
      compute_pmatrix(e, bl[T + dsc[k].b.z] * rt, Pm);
      double* o = pin + (size_t)k * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) o[i * 4 + q] = Pm[i][q];
    }
  }
}

// What a lineage kernel (K11b, K12b, K13b: a workgroup per (rate category blockIdx.x, sample blockIdx.y)) holds once its
// tables stand: the two LDS tables at the head of its dynamic LDS (the kernel's own LDS follows pin + (T - 2) * 16), the
// sample's descriptors and the CLV area of the (sample, rate): [op][2][plane] double2, components (0,1) and (2,3) of a
// pattern in two planes.
struct TreeTables {
  int len;  // the sample's path length; 0 (no valid path): no table is filled and the kernel returns
  double *tiptab, *pin;
  const AsrOp* dsc;
  double2* clv_s;
  size_t plane;
};

// The tables filled and the workgroup synchronised behind them.
__device__ static __forceinline__ TreeTables tree_prologue(double2* smem, int R, int T, const AsrOp* __restrict__ desc,
                                                           const double* __restrict__ brlen, const double* __restrict__ rates,
                                                           const double* __restrict__ eig, const int32_t* __restrict__ plen,
                                                           double2* clv, int Lp) {
  const int n_ops = T - 2;
  const int sample = blockIdx.y, rate = blockIdx.x;
  // (every pointer is formed whatever the length: a pointer that is null on one path no longer reads as based on the
  // kernel's __restrict__ argument, and the descriptor loads of the down pass stop being scalar loads)
  TreeTables t;
  t.len = plen[sample];
  t.tiptab = reinterpret_cast<double*>(smem);
  t.pin = t.tiptab + (size_t)T * 16;
  t.dsc = desc + (size_t)sample * n_ops;
  t.plane = (size_t)Lp;
  t.clv_s = clv + ((size_t)sample * R + rate) * n_ops * 2 * t.plane;
  if (t.len == 0) return t;
  const double* __restrict__ e = eig + (size_t)sample * 36;
  const double rt = rates[(size_t)sample * R + rate];
  const double* __restrict__ bl = brlen + (size_t)sample * (2 * (size_t)T - 2);
  tree_fill_tables(T, t.dsc, e, bl, rt, t.tiptab, t.pin);
  __syncthreads();
  return t;
}

// The CLV of the lane's pattern that op k stored (clv_s: the (sample, rate)'s area), as four doubles.
__device__ static __forceinline__ void tree_load_clv(const double2* clv_s, size_t plane, int k, int pat, double (&y)[4]) {
  const double2* c = clv_s + (size_t)k * 2 * plane + pat;
  const double2 lo = c[0], hi = c[plane];
  y[0] = lo.x;
  y[1] = lo.y;
  y[2] = hi.x;
  y[3] = hi.y;
}

// K3b's upward pass of one pattern (n_prune: the all-N one), the lane's, without K3b's software pipeline: every inner CLV
// stored.  kStoreAll = false (K13b's MRCA form) stores only what a later op pops from the stack, which the lane itself
// reads back.  `a` leaves as the root's CLV.
template <bool kStoreAll = true>
__device__ static __forceinline__ void tree_upward_pattern(int n_ops, int n_prune, int pat, const uint8_t* __restrict__ msa,
                                                           const AsrOp* __restrict__ dsc, const double* tiptab,
                                                           const double* pin, double2* clv_s, size_t plane, double (&a)[4]) {
  const bool all_n = pat >= n_prune;
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = 1.0;
  for (int k = 0; k < n_ops; ++k) {
    const int4 da = dsc[k].a, db = dsc[k].b;
    const int kind = da.x & 15;
    double u[4], v[4];
    if (kind == OP_CHERRY) {
      const int sa = all_n ? 4 : (int)msa[(size_t)da.y * n_prune + pat];
      const int sb = all_n ? 4 : (int)msa[(size_t)da.z * n_prune + pat];
      tree_tip_col(tiptab, db.x, sa, u);
      tree_tip_col(tiptab, db.y, sb, v);
    } else {
      tree_matvec(pin + (size_t)(k - 1) * 16, a, v);
      if (kind == OP_TIP_ACC) {
        const int sa = all_n ? 4 : (int)msa[(size_t)da.y * n_prune + pat];
        tree_tip_col(tiptab, db.x, sa, u);
      } else {
        double y[4];
        tree_load_clv(clv_s, plane, da.w, pat, y);
        tree_matvec(pin + (size_t)da.w * 16, y, u);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = u[q] * v[q];
    tree_rescale(a);
    if (kStoreAll || (da.x >> 8) != 0) {
      double2* ck = clv_s + (size_t)k * 2 * plane + pat;
      ck[0] = make_double2(a[0], a[1]);
      ck[plane] = make_double2(a[2], a[3]);
    }
  }
}

// The pass over all NP = n_prune + 1 patterns (the all-N one last), a lane per pattern (lanes past the last pattern repeat
// it: same values, no predicate).
__device__ static __forceinline__ void tree_upward(int n_ops, int n_prune, const uint8_t* __restrict__ msa,
                                                   const AsrOp* __restrict__ dsc, const double* tiptab, const double* pin,
                                                   double2* clv_s, size_t plane, int wave, int n_waves, int lane) {
  const int NP = n_prune + 1;
  for (int s0 = wave * 64; s0 < NP; s0 += n_waves * 64) {
    double a[4];
    tree_upward_pattern<true>(n_ops, n_prune, min(s0 + lane, NP - 1), msa, dsc, tiptab, pin, clv_s, plane, a);
  }
}

// A chain word (K11c writes it, K12c marks slot 0's): the op that produced the slot's node v_s, and in bit 30 whether
// v_{s-1} is the child that op popped (else its accumulator child).
__device__ static __forceinline__ int chain_op(int word) { return word & 0x3fffffff; }
__device__ static __forceinline__ bool chain_flag(int word) { return (word >> 30) != 0; }

// One step down the lineage, from v_s (s >= 1, chain word `word`) to v_{s-1}, for the pattern `pat` of the lane.
// m = the message of v_s's child off the path: its tip column, or P_kw CLV_kw for the op kw that produced it.  Returns kc,
// the op that produced v_{s-1}.
__device__ static __forceinline__ int tree_sibling_message(const TreeTables& t, int word, const uint8_t* __restrict__ msa,
                                                           int n_prune, int pat, bool all_n, double (&m)[4]) {
  const int k = chain_op(word);
  const int4 da = t.dsc[k].a, db = t.dsc[k].b;
  if ((da.x & 15) == OP_TIP_ACC) {
    const int sa = all_n ? 4 : (int)msa[(size_t)da.y * n_prune + pat];
    tree_tip_col(t.tiptab, db.x, sa, m);
    return k - 1;
  }
  const bool via_pop = chain_flag(word);
  const int kw = via_pop ? k - 1 : da.w;
  double y[4];
  tree_load_clv(t.clv_s, t.plane, kw, pat, y);
  tree_matvec(t.pin + (size_t)kw * 16, y, m);
  return via_pop ? da.w : k - 1;
}

// The seed edge, slot 0 (chain word `word`, marked by K12c): m = the message of the seed tip's sibling -- the cherry's other
// tip, or the accumulator child of a tip-accumulate op --, Lb = the seed tip's indicator vector (all ones for N).  Returns
// the seed tip's index in the tip table.
__device__ static __forceinline__ int tree_seed_edge(const TreeTables& t, int word, const uint8_t* __restrict__ msa,
                                                     int n_prune, int pat, bool all_n, double (&m)[4], double (&Lb)[4]) {
  const int k = chain_op(word);
  const int4 da = t.dsc[k].a, db = t.dsc[k].b;
  const bool flag = chain_flag(word);  // the seed is the cherry's z child
  int useed, srow;
  if ((da.x & 15) == OP_CHERRY) {
    const int sib = flag ? db.x : db.y, sib_row = flag ? da.y : da.z;
    useed = flag ? db.y : db.x;
    srow = flag ? da.z : da.y;
    const int ss = all_n ? 4 : (int)msa[(size_t)sib_row * n_prune + pat];
    tree_tip_col(t.tiptab, sib, ss, m);
  } else {
    useed = db.x;
    srow = da.y;
    double y[4];
    tree_load_clv(t.clv_s, t.plane, k - 1, pat, y);
    tree_matvec(t.pin + (size_t)(k - 1) * 16, y, m);
  }
  const int st = all_n ? 4 : (int)msa[(size_t)srow * n_prune + pat];
#pragma unroll
  for (int c = 0; c < 4; ++c) Lb[c] = (st >= 4 || st == c) ? 1.0 : 0.0;
  return useed;
}

// w[b] = lik_rate(pat, b) / Z_pat(b), the weight of the category under each naive base, from K1's unmixed planes; 0 where
// Z or the category's plane is 0.  The all-N pattern takes K11r's convention (likelihood pi_b whatever the category): 1 / R.
__device__ static __forceinline__ void tree_rate_weights(const int32_t* __restrict__ site_scal,
                                                         const double* __restrict__ site_lik, int sample, int rate, int R,
                                                         int n_prune, int pat, bool all_n, double (&w)[5]) {
  if (all_n) {
#pragma unroll
    for (int b = 0; b < 5; ++b) w[b] = 1.0 / (double)R;
  } else {
    const RatePlanes planes = rate_planes(site_scal, site_lik, sample, R, n_prune, pat);
    double z[5], v[5];
    planes.totals(R, z);
    planes.values(rate, v);
#pragma unroll
    for (int b = 0; b < 5; ++b) w[b] = (z[b] == 0.0 || v[b] == 0.0) ? 0.0 : v[b] / z[b];
  }
}

// The message into the root from above for each basis vector of the naive tip (A, C, G, T, N): A[b][i] = pi_i P_naive[i][b],
// the row sums of P_naive for N.
__device__ static __forceinline__ void tree_root_messages(const double* tiptab, const double* __restrict__ p4,
                                                          double (&A)[5][4]) {
  double n4[4];
  tree_tip_col(tiptab, 0, 4, n4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) A[b][i] = p4[i] * tiptab[b * 4 + i];
    A[4][i] = p4[i] * n4[i];
  }
}

// The descent, in the two halves K12b puts its edge table between.  M = A o m: the message from above into v_s, A, times the
// sibling's.
__device__ static __forceinline__ void tree_join(const double (&A)[4], const double (&m)[4], double (&M)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) M[i] = A[i] * m[i];
}

// A = M^T P_kc, the message into v_{s-1} through its branch, divided by its largest entry (a stored CLV's largest entry
// lies anywhere in [2^-256, 1] -- tree_rescale repeats until it does, as long as the op's own product stayed above the
// subnormals --, so a few unnormalised steps would underflow).
__device__ static __forceinline__ void tree_push_down(const double* pin, int kc, const double (&M)[4], double (&A)[4]) {
  tree_vecmat(pin + (size_t)kc * 16, M, A);
  const double top = fmax(fmax(A[0], A[1]), fmax(A[2], A[3]));
  if (top > 0.0 && top < INFINITY) {
    const double inv = 1.0 / top;
#pragma unroll
    for (int i = 0; i < 4; ++i) A[i] *= inv;
  }
}

// A, the message from above into v_s, becomes the message into v_{s-1}.
__device__ static __forceinline__ void tree_descend(const double* pin, int kc, const double (&m)[4], double (&A)[4]) {
  double M[4];
  tree_join(A, m, M);
  tree_push_down(pin, kc, M, A);
}

}  // namespace lh
