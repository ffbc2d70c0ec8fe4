// One backward-smoothing step over the compact forward layout (device only): the arithmetic K5 (lh_posterior.hip), K9
// (lh_codon.hip) and K10 (lh_events.hip) share, defined once.  K5's header derives the formulas.
//
// The three step forms take (J, [i,] f, next, nx, out, gl): f = the forward row or region vector, next = pi of the position
// above it, read as nx(next, k), out = where the step's result goes.  K5 reads `next` as it is and writes out == f (every
// entry is read and written by its owning lane only, and all of a row's reads precede its writes in that lane's program
// order); K9 reads it through a mask and writes a vector of its own.  Nothing here promises that f and out do not alias: a
// caller that knows so says it with __restrict__ on a forwarding function of its own.
// The shape and the parentheses of every expression fix the FMA contraction and with it the bits: K10 asserts its genes
// bit-equal to K5's, K9 likewise (tests/test_gpu_events.py, tests/test_gpu_codons.py).
#pragma once

#include "lh_device.h"

namespace lh {
namespace smooth {

constexpr int kG = 16;  // lanes per sample
constexpr int kWaves = 4;
constexpr int kPerWave = 64 / kG;

__device__ inline double group_sum(double v) {
#pragma unroll
  for (int m = 1; m < kG; m <<= 1) v += __shfl_xor(v, m, kG);
  return v;
}

// the ratio pi / Z of one successor, 0 where pi is 0 (Z may be 0 there)
__device__ inline double ratio(double p, double z) { return p != 0.0 ? p / z : 0.0; }

// nx of a vector that is read as it is
struct Direct {
  __device__ double operator()(const double* v, size_t k) const { return v[k]; }
};

// ---- the compact forward layout of a sample: V genes | V-D rows | D genes | D-J rows | J genes (light chains: no D part) ----

__device__ inline size_t row_stride(const DevSampleJunction& J) { return (size_t)J.n_left + 5 * (size_t)J.n_right; }

struct ForwardLayout {
  size_t vd_size, dj_size;            // of the junctions' rows
  size_t o_v, o_vd, o_d, o_dj, o_j;  // offsets (light chains: o_d == o_dj == o_j)
};

__device__ inline ForwardLayout forward_layout(const DevSampler& smp) {
  ForwardLayout lay;
  lay.vd_size = (size_t)smp.vd.n_rows * row_stride(smp.vd);
  lay.dj_size = smp.has_d ? (size_t)smp.dj.n_rows * row_stride(smp.dj) : 0;
  lay.o_v = 0;
  lay.o_vd = smp.n_v;
  lay.o_d = lay.o_vd + lay.vd_size;
  lay.o_dj = lay.o_d + (smp.has_d ? smp.n_d : 0);
  lay.o_j = lay.o_dj + lay.dj_size;
  return lay;
}

// ---- the normalisers ----

// A_i = sum_l left_lo[i][l] F[i, l] over the left genes that have a state on row i (f: the forward row; lo: row i of
// left_lo, which the caller's own pass over the left genes reads too)
__device__ inline double left_weight(const DevSampleJunction& J, int i, const double* lo, const double* f, int gl) {
  double a = 0.0;
  for (int l = gl; l < J.n_left; l += kG)
    if (i < J.left_rows[l]) a += lo[l] * f[l];
  return group_sum(a);
}

// Right gene r's tables toward its successors on row i1 = i + 1 of a row i < W - 1, its four NTI states and its germline
// state: gene_prob, nti_transition [a][b] (a -> b), nti_landing_in, nti_landing_out into the row-i1 germline state.
struct RightGene {
  double gp;
  const double *ntt, *nli, *nlo;
};

__device__ inline RightGene right_gene(const DevSampleJunction& J, int i1, int r) {
  return {J.gp[r], J.ntt + (size_t)r * 16, J.nli + (size_t)r * 4, J.nlo + ((size_t)i1 * J.n_right + r) * 4};
}

// Z of those five successors, from a = A_i, the gene's NTI entries f0..f3 and its germline entry fg (0 where it has none)
// of the forward row i; germ_next: the gene has a germline state on row i1 (else li = rt = 0).
// (li and rtrans are looked up after z0..z3: their branch ahead of them cost K5 1 %, profiles/r13_smooth_shared.txt)
struct RowNorm {
  double z0, z1, z2, z3, zg, li, rt;
  bool germ_next;
};

__device__ inline RowNorm row_normalisers(const DevSampleJunction& J, int i1, int r, const RightGene& g, double a, double f0,
                                          double f1, double f2, double f3, double fg) {
  const int nR = J.n_right;
  const double gp = g.gp;
  const double *ntt = g.ntt, *nli = g.nli, *nlo = g.nlo;
  RowNorm n;
  n.germ_next = i1 >= J.right_first[r];
  n.z0 = (gp * nli[0]) * a + (ntt[0] * f0 + ntt[4] * f1 + ntt[8] * f2 + ntt[12] * f3);
  n.z1 = (gp * nli[1]) * a + (ntt[1] * f0 + ntt[5] * f1 + ntt[9] * f2 + ntt[13] * f3);
  n.z2 = (gp * nli[2]) * a + (ntt[2] * f0 + ntt[6] * f1 + ntt[10] * f2 + ntt[14] * f3);
  n.z3 = (gp * nli[3]) * a + (ntt[3] * f0 + ntt[7] * f1 + ntt[11] * f2 + ntt[15] * f3);
  n.li = n.germ_next ? J.li[(size_t)i1 * nR + r] : 0.0;
  n.rt = n.germ_next ? J.rtrans[(size_t)i1 * nR + r] : 0.0;
  n.zg = (gp * n.li) * a + (nlo[0] * f0 + nlo[1] * f1 + nlo[2] * f2 + nlo[3] * f3) + n.rt * fg;
  return n;
}

// The last row's successor of right gene r, gene r of the region right of the junction: its Z, the weight c of "every
// left gene's state" into it less A, and the germline state's transition xt.
struct LastNorm {
  double z, c, xt;
};

__device__ inline LastNorm last_normaliser(const DevSampleJunction& J, int r, double a, double f0, double f1, double f2,
                                           double f3, double fg) {
  const double* xn = J.exit_nlo + (size_t)r * 4;
  LastNorm n;
  n.c = (J.gp[r] * J.exit_li[r]) * J.prod[r];
  n.xt = J.exit_trans[r];
  n.z = n.c * a + (xn[0] * f0 + xn[1] * f1 + xn[2] * f2 + xn[3] * f3) + n.xt * fg;
  return n;
}

// ---- the three step forms ----
// (a row's entries are left | NTI x 4 | right: k = l, nL + 4 r + b, nL + 4 nR + r)

// Junction row i = 0 .. W-2: out = one smoothing step from `next`, a vector of row i + 1, over the forward row f.
template <class Next>
__device__ inline void step_row(const DevSampleJunction& J, int i, const double* f, const double* next, const Next& nx,
                                double* out, int gl) {
  const int nL = J.n_left, nR = J.n_right;
  const size_t kN = nL, kR = (size_t)nL + 4 * (size_t)nR;
  const double *fN = f + kN, *fR = f + kR;
  double *outN = out + kN, *outR = out + kR;
  const int i1 = i + 1;
  const double* lo = J.left_lo + (size_t)i * nL;
  const double a = left_weight(J, i, lo, f, gl);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const RightGene g = right_gene(J, i1, r);
    const double *ntt = g.ntt, *nli = g.nli, *nlo = g.nlo;
    const double f0 = fN[(size_t)r * 4 + 0], f1 = fN[(size_t)r * 4 + 1], f2 = fN[(size_t)r * 4 + 2],
                 f3 = fN[(size_t)r * 4 + 3];
    const double fg = i >= J.right_first[r] ? fR[r] : 0.0;  // the gene has a germline state on row i
    // successors: NTI b of row i + 1 (b = 0..3), germline state of row i + 1
    const RowNorm n = row_normalisers(J, i1, r, g, a, f0, f1, f2, f3, fg);
    const double r0 = ratio(nx(next, kN + (size_t)r * 4 + 0), n.z0), r1 = ratio(nx(next, kN + (size_t)r * 4 + 1), n.z1);
    const double r2 = ratio(nx(next, kN + (size_t)r * 4 + 2), n.z2), r3 = ratio(nx(next, kN + (size_t)r * 4 + 3), n.z3);
    const double rg = n.germ_next ? ratio(nx(next, kR + r), n.zg) : 0.0;
    outN[(size_t)r * 4 + 0] = f0 * (ntt[0] * r0 + ntt[1] * r1 + ntt[2] * r2 + ntt[3] * r3 + nlo[0] * rg);
    outN[(size_t)r * 4 + 1] = f1 * (ntt[4] * r0 + ntt[5] * r1 + ntt[6] * r2 + ntt[7] * r3 + nlo[1] * rg);
    outN[(size_t)r * 4 + 2] = f2 * (ntt[8] * r0 + ntt[9] * r1 + ntt[10] * r2 + ntt[11] * r3 + nlo[2] * rg);
    outN[(size_t)r * 4 + 3] = f3 * (ntt[12] * r0 + ntt[13] * r1 + ntt[14] * r2 + ntt[15] * r3 + nlo[3] * rg);
    outR[r] = fg * (n.rt * rg);
    b += g.gp * (nli[0] * r0 + nli[1] * r1 + nli[2] * r2 + nli[3] * r3 + n.li * rg);
  }
  b = group_sum(b);
  for (int l = gl; l < nL; l += kG) {
    const bool here = i < J.left_rows[l];
    const double own = i1 < J.left_rows[l] ? nx(next, (size_t)l) : 0.0;
    out[l] = own + (here ? f[l] * (lo[l] * b) : 0.0);
  }
}

// Junction row W-1: `next` is a gene vector of the region right of the junction.
template <class Next>
__device__ inline void step_last(const DevSampleJunction& J, const double* f, const double* next, const Next& nx,
                                 double* out, int gl) {
  const int nL = J.n_left, nR = J.n_right, i = J.n_rows - 1;
  const size_t kN = nL, kR = (size_t)nL + 4 * (size_t)nR;
  const double *fN = f + kN, *fR = f + kR;
  double *outN = out + kN, *outR = out + kR;
  const double* lo = J.left_lo + (size_t)i * nL;
  const double a = left_weight(J, i, lo, f, gl);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const double* xn = J.exit_nlo + (size_t)r * 4;
    const double f0 = fN[(size_t)r * 4 + 0], f1 = fN[(size_t)r * 4 + 1], f2 = fN[(size_t)r * 4 + 2],
                 f3 = fN[(size_t)r * 4 + 3];
    const double fg = i >= J.right_first[r] ? fR[r] : 0.0;
    const LastNorm n = last_normaliser(J, r, a, f0, f1, f2, f3, fg);
    const double rho = ratio(nx(next, (size_t)r), n.z);
    outN[(size_t)r * 4 + 0] = f0 * (xn[0] * rho);
    outN[(size_t)r * 4 + 1] = f1 * (xn[1] * rho);
    outN[(size_t)r * 4 + 2] = f2 * (xn[2] * rho);
    outN[(size_t)r * 4 + 3] = f3 * (xn[3] * rho);
    outR[r] = fg * (n.xt * rho);
    b += n.c * rho;
  }
  b = group_sum(b);
  for (int l = gl; l < nL; l += kG) out[l] = i < J.left_rows[l] ? f[l] * (lo[l] * b) : 0.0;
}

// The germline region left of a junction (the expectation of K4's draw_left_region): f[nL] = its forward vector, `next` a
// vector of the junction's row 0, out[nL] = its gene vector.  Row 0's NTI and germline states have the region's genes as
// their only predecessors, with weights enter_lo[g] * (gp nli[b] or gp li[0]) * f[g]: their mass is shared out in
// proportion to enter_lo[g] f[g].
template <class Next>
__device__ inline void step_left(const DevSampleJunction& J, const double* f, const double* next, const Next& nx,
                                 double* out, int gl) {
  const int nL = J.n_left, nR = J.n_right;
  const size_t kN = nL, kR = (size_t)nL + 4 * (size_t)nR;
  double e = 0.0;
  for (int g = gl; g < nL; g += kG) e += J.enter_lo[g] * f[g];
  e = group_sum(e);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const double gp = J.gp[r];
    const double* nli = J.nli + (size_t)r * 4;
    const double li = J.right_first[r] == 0 ? J.li[r] : 0.0;
    const size_t kn = kN + (size_t)r * 4;
    b += ratio(nx(next, kn + 0), (gp * nli[0]) * e) * (gp * nli[0]);
    b += ratio(nx(next, kn + 1), (gp * nli[1]) * e) * (gp * nli[1]);
    b += ratio(nx(next, kn + 2), (gp * nli[2]) * e) * (gp * nli[2]);
    b += ratio(nx(next, kn + 3), (gp * nli[3]) * e) * (gp * nli[3]);
    if (li != 0.0) b += ratio(nx(next, kR + r), (gp * li) * e) * (gp * li);
  }
  b = group_sum(b);
  for (int g = gl; g < nL; g += kG) {
    const double own = J.left_rows[g] > 0 ? nx(next, (size_t)g) : 0.0;
    out[g] = own + f[g] * (J.enter_lo[g] * b);
  }
}

}  // namespace smooth
}  // namespace lh
