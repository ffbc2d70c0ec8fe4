// K9: exact posterior distributions of the naive sequence's codons on the device (gfx950).
//
// With K5's backward kernel  B_t(k | k2) = F_t[k] T(k -> k2) / Z_t(k2)  (lh_posterior.hip) the joint posterior of three
// consecutive chain positions is  P(k, k2, k3) = pi_{t+2}(k3) B_{t+1}(k2 | k3) B_t(k | k2),  and a codon's distribution is
// its push-forward onto the bases the three states write on the codon's sites.  One smoothing step is linear in the
// vector it is given, so the push-forward is a smoothing step per TAG: pi_{t+2} restricted to the entries that write base
// b3 steps down one position, the result restricted to the entries that write b2 steps down once more, and the entries
// of what arrives are summed by the base b1 they write:  1 + 5 + 25 steps and 25 binning passes for a window of three
// positions, of which those whose restricted vector is all zero (N where no state writes N) are skipped.  A window of two
// positions (a germline gene writes two of the codon's sites: 25 local codes) takes one tagged step per code.  The
// untagged recursion pi_q -> pi_{q-1} runs beside it, so the forward arrays are only read (K5 overwrites them; K9 does
// not), and the V / D / J gene posteriors fall out of it.  Only ratios inside one forward row or region vector appear:
// the rows' 2^256 rescalings cancel as in K5.
//
// Lanes as K4 / K5: sixteen lanes per sample, four samples per wave; lane gl owns left genes gl, gl + 16, ... and right
// genes gl, gl + 16, ... (their NTI and germline entries) and the same genes of a region vector.  Every entry of the four
// scratch vectors a sample uses (pi_q, pi_{q-1}, the two tagged vectors) is written and read by its owner only; sums
// over the group are butterflies, which give every lane the same bits in a fixed order, so the skip decisions are
// uniform over the group.  No atomics.  No private array is reached by a dynamic index: the five bins of a binning pass
// are accumulators of a fully unrolled loop, picked by comparing the entry's code with constants, and bins 5 .. 24 of a
// two-site gene take further passes; each bin is then reduced by the butterfly and written once.
// The grid is capped (2048 workgroups; DebugOptions::codon_blocks): a group takes samples slot, slot + slots, ... and keeps
// its scratch vectors.
#include <algorithm>
#include <cmath>

#include "lh_device.h"

namespace lh {

namespace {

constexpr int kG = 16;  // lanes per sample
constexpr int kWaves = 4;
constexpr int kPerWave = 64 / kG;

__device__ inline double group_sum(double v) {
#pragma unroll
  for (int m = 1; m < kG; m <<= 1) v += __shfl_xor(v, m, kG);
  return v;
}

__device__ inline double ratio(double p, double z) { return p != 0.0 ? p / z : 0.0; }

// the entries of a vector that carry local code `want` (want < 0: all of them)
struct Mask {
  const uint8_t* code;
  int want;
};
__device__ inline double mv(const double* __restrict__ v, const Mask& m, size_t k) {
  return (m.want < 0 || m.code[k] == m.want) ? v[k] : 0.0;
}

// A chain position: a germline region (J = the junction to its right, null for the J genes) or a junction row.
struct Pos {
  int kind;  // 0 region, 1 row
  const DevSampleJunction* J;
  int row;
  size_t off;  // of its entries in the compact forward layout
  int n_genes;
};

__device__ inline Pos position(const DevSampler& smp, int q) {
  const DevSampleJunction& VD = smp.vd;
  const DevSampleJunction& DJ = smp.dj;
  const size_t svd = (size_t)VD.n_left + 5 * (size_t)VD.n_right;
  if (q == 0) return Pos{0, &VD, 0, 0, smp.n_v};
  if (q <= VD.n_rows) return Pos{1, &VD, q - 1, (size_t)smp.n_v + (size_t)(q - 1) * svd, 0};
  size_t off = (size_t)smp.n_v + (size_t)VD.n_rows * svd;
  q -= VD.n_rows + 1;
  if (!smp.has_d) return Pos{0, nullptr, 0, off, smp.n_j};
  if (q == 0) return Pos{0, &DJ, 0, off, smp.n_d};
  const size_t sdj = (size_t)DJ.n_left + 5 * (size_t)DJ.n_right;
  off += smp.n_d;
  if (q <= DJ.n_rows) return Pos{1, &DJ, q - 1, off + (size_t)(q - 1) * sdj, 0};
  return Pos{0, nullptr, 0, off + (size_t)DJ.n_rows * sdj, smp.n_j};
}

// f(entry) for every entry of the position's vector this lane owns
template <class F>
__device__ inline void for_owned(const Pos& p, int gl, F&& f) {
  if (p.kind == 0) {
    for (int g = gl; g < p.n_genes; g += kG) f((size_t)g);
    return;
  }
  const int nL = p.J->n_left, nR = p.J->n_right;
  for (int l = gl; l < nL; l += kG) f((size_t)l);
  for (int r = gl; r < nR; r += kG) {
#pragma unroll
    for (int a = 0; a < 4; ++a) f((size_t)nL + 4 * (size_t)r + a);
    f((size_t)nL + 4 * (size_t)nR + r);
  }
}

__device__ inline double mass(const Pos& p, const double* __restrict__ v, const Mask& m, int gl) {
  double a = 0.0;
  for_owned(p, gl, [&](size_t k) { a += mv(v, m, k); });
  return group_sum(a);
}

// The three step forms below are K5's smooth_row, smooth_last_row and smooth_left_region (lh_posterior.hip) written out of
// place and with a mask on the vector they are handed: the transition arithmetic is the same and must change together.
// Junction row i = 0 .. W-2 (smooth_row of K5, out of place): out = one smoothing step from `next` = a (tagged) vector of
// row i + 1, over the forward row f.
__device__ void step_row(const DevSampleJunction& J, int i, const double* __restrict__ f, const double* __restrict__ next,
                         const Mask& m, double* __restrict__ out, int gl) {
  const int nL = J.n_left, nR = J.n_right;
  const size_t oN = nL, oR = (size_t)nL + 4 * (size_t)nR;
  const int i1 = i + 1;
  double a = 0.0;
  for (int l = gl; l < nL; l += kG)
    if (i < J.left_rows[l]) a += J.left_lo[(size_t)i * nL + l] * f[l];
  a = group_sum(a);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const double gp = J.gp[r];
    const double* ntt = J.ntt + (size_t)r * 16;  // [a][b]: a -> b
    const double* nli = J.nli + (size_t)r * 4;
    const double* nlo = J.nlo + ((size_t)i1 * nR + r) * 4;
    const size_t kn = oN + (size_t)r * 4;
    const double f0 = f[kn + 0], f1 = f[kn + 1], f2 = f[kn + 2], f3 = f[kn + 3];
    const bool germ_here = i >= J.right_first[r];
    const bool germ_next = i1 >= J.right_first[r];
    const double fg = germ_here ? f[oR + r] : 0.0;
    const double z0 = (gp * nli[0]) * a + (ntt[0] * f0 + ntt[4] * f1 + ntt[8] * f2 + ntt[12] * f3);
    const double z1 = (gp * nli[1]) * a + (ntt[1] * f0 + ntt[5] * f1 + ntt[9] * f2 + ntt[13] * f3);
    const double z2 = (gp * nli[2]) * a + (ntt[2] * f0 + ntt[6] * f1 + ntt[10] * f2 + ntt[14] * f3);
    const double z3 = (gp * nli[3]) * a + (ntt[3] * f0 + ntt[7] * f1 + ntt[11] * f2 + ntt[15] * f3);
    const double li = germ_next ? J.li[(size_t)i1 * nR + r] : 0.0;
    const double rt = germ_next ? J.rtrans[(size_t)i1 * nR + r] : 0.0;
    const double zg = (gp * li) * a + (nlo[0] * f0 + nlo[1] * f1 + nlo[2] * f2 + nlo[3] * f3) + rt * fg;
    const double r0 = ratio(mv(next, m, kn + 0), z0), r1 = ratio(mv(next, m, kn + 1), z1);
    const double r2 = ratio(mv(next, m, kn + 2), z2), r3 = ratio(mv(next, m, kn + 3), z3);
    const double rg = germ_next ? ratio(mv(next, m, oR + r), zg) : 0.0;
    out[kn + 0] = f0 * (ntt[0] * r0 + ntt[1] * r1 + ntt[2] * r2 + ntt[3] * r3 + nlo[0] * rg);
    out[kn + 1] = f1 * (ntt[4] * r0 + ntt[5] * r1 + ntt[6] * r2 + ntt[7] * r3 + nlo[1] * rg);
    out[kn + 2] = f2 * (ntt[8] * r0 + ntt[9] * r1 + ntt[10] * r2 + ntt[11] * r3 + nlo[2] * rg);
    out[kn + 3] = f3 * (ntt[12] * r0 + ntt[13] * r1 + ntt[14] * r2 + ntt[15] * r3 + nlo[3] * rg);
    out[oR + r] = fg * (rt * rg);
    b += gp * (nli[0] * r0 + nli[1] * r1 + nli[2] * r2 + nli[3] * r3 + li * rg);
  }
  b = group_sum(b);
  for (int l = gl; l < nL; l += kG) {
    const bool here = i < J.left_rows[l];
    const double own = i1 < J.left_rows[l] ? mv(next, m, (size_t)l) : 0.0;
    out[l] = own + (here ? f[l] * (J.left_lo[(size_t)i * nL + l] * b) : 0.0);
  }
}

// Junction row W-1: `next` is a (tagged) gene vector of the region right of the junction.
__device__ void step_last(const DevSampleJunction& J, const double* __restrict__ f, const double* __restrict__ next,
                          const Mask& m, double* __restrict__ out, int gl) {
  const int nL = J.n_left, nR = J.n_right, i = J.n_rows - 1;
  const size_t oN = nL, oR = (size_t)nL + 4 * (size_t)nR;
  double a = 0.0;
  for (int l = gl; l < nL; l += kG)
    if (i < J.left_rows[l]) a += J.left_lo[(size_t)i * nL + l] * f[l];
  a = group_sum(a);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const double* xn = J.exit_nlo + (size_t)r * 4;
    const size_t kn = oN + (size_t)r * 4;
    const double f0 = f[kn + 0], f1 = f[kn + 1], f2 = f[kn + 2], f3 = f[kn + 3];
    const double fg = i >= J.right_first[r] ? f[oR + r] : 0.0;
    const double c = (J.gp[r] * J.exit_li[r]) * J.prod[r];
    const double xt = J.exit_trans[r];
    const double z = c * a + (xn[0] * f0 + xn[1] * f1 + xn[2] * f2 + xn[3] * f3) + xt * fg;
    const double rho = ratio(mv(next, m, (size_t)r), z);
    out[kn + 0] = f0 * (xn[0] * rho);
    out[kn + 1] = f1 * (xn[1] * rho);
    out[kn + 2] = f2 * (xn[2] * rho);
    out[kn + 3] = f3 * (xn[3] * rho);
    out[oR + r] = fg * (xt * rho);
    b += c * rho;
  }
  b = group_sum(b);
  for (int l = gl; l < nL; l += kG)
    out[l] = i < J.left_rows[l] ? f[l] * (J.left_lo[(size_t)i * nL + l] * b) : 0.0;
}

// The germline region left of a junction: `next` is a (tagged) vector of the junction's row 0.
__device__ void step_left(const DevSampleJunction& J, const double* __restrict__ f, const double* __restrict__ next,
                          const Mask& m, double* __restrict__ out, int gl) {
  const int nL = J.n_left, nR = J.n_right;
  const size_t oN = nL, oR = (size_t)nL + 4 * (size_t)nR;
  double e = 0.0;
  for (int g = gl; g < nL; g += kG) e += J.enter_lo[g] * f[g];
  e = group_sum(e);
  double b = 0.0;
  for (int r = gl; r < nR; r += kG) {
    const double gp = J.gp[r];
    const double* nli = J.nli + (size_t)r * 4;
    const double li = J.right_first[r] == 0 ? J.li[r] : 0.0;
    const size_t kn = oN + (size_t)r * 4;
    b += ratio(mv(next, m, kn + 0), (gp * nli[0]) * e) * (gp * nli[0]);
    b += ratio(mv(next, m, kn + 1), (gp * nli[1]) * e) * (gp * nli[1]);
    b += ratio(mv(next, m, kn + 2), (gp * nli[2]) * e) * (gp * nli[2]);
    b += ratio(mv(next, m, kn + 3), (gp * nli[3]) * e) * (gp * nli[3]);
    if (li != 0.0) b += ratio(mv(next, m, oR + r), (gp * li) * e) * (gp * li);
  }
  b = group_sum(b);
  for (int g = gl; g < nL; g += kG) {
    const double own = J.left_rows[g] > 0 ? mv(next, m, (size_t)g) : 0.0;
    out[g] = own + f[g] * (J.enter_lo[g] * b);
  }
}

// out = the smoothing step from position p + 1 down to p (p is never the last position)
__device__ inline void step(const Pos& p, const double* __restrict__ F, const double* __restrict__ next, const Mask& m,
                            double* __restrict__ out, int gl) {
  const double* f = F + p.off;
  if (p.kind == 0)
    step_left(*p.J, f, next, m, out, gl);
  else if (p.row == p.J->n_rows - 1)
    step_last(*p.J, f, next, m, out, gl);
  else
    step_row(*p.J, p.row, f, next, m, out, gl);
}

// dst[base + mult * c] for the position's codes c = 0 .. ncodes-1: the sums of v over the entries that carry code c
__device__ inline void bin_out(const Pos& p, const double* __restrict__ v, const uint8_t* __restrict__ code, int ncodes,
                               int mult, int base, double* __restrict__ dst, int gl) {
  for (int c0 = 0; c0 < ncodes; c0 += 5) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for_owned(p, gl, [&](size_t k) {
      const int c = code[k];
      const double x = v[k];
#pragma unroll
      for (int j = 0; j < 5; ++j) acc[j] += c == c0 + j ? x : 0.0;
    });
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[j] = group_sum(acc[j]);
    if (gl == 0) {
#pragma unroll
      for (int j = 0; j < 5; ++j) dst[base + mult * (c0 + j)] = acc[j];
    }
  }
}

__device__ inline void zero_out(int ncodes, int mult, int base, double* __restrict__ dst, int gl) {
  for (int c = gl; c < ncodes; c += kG) dst[base + mult * c] = 0.0;
}

// One window: top = pi of its highest position; u, v scratch vectors; dst[125].
__device__ void window(const DevSampler& smp, const CodonWindow& w, const uint8_t* __restrict__ codes,
                       const double* __restrict__ F, const double* __restrict__ top, double* __restrict__ u,
                       double* __restrict__ v, double* __restrict__ dst, int gl) {
  const int hi = w.npos - 1;
  const Pos ptop = position(smp, w.top), pmid = position(smp, w.top - 1);
  const uint8_t* ctop = codes + w.code_off[hi];
  if (w.npos == 2) {
    const uint8_t* c0 = codes + w.code_off[0];
    for (int c = 0; c < w.ncodes[1]; ++c) {
      const Mask m{ctop, c};
      const int base = w.mult[1] * c;
      if (mass(ptop, top, m, gl) == 0.0) {
        zero_out(w.ncodes[0], w.mult[0], base, dst, gl);
        continue;
      }
      step(pmid, F, top, m, v, gl);
      bin_out(pmid, v, c0, w.ncodes[0], w.mult[0], base, dst, gl);
    }
    return;
  }
  const Pos plow = position(smp, w.top - 2);
  const uint8_t* c1 = codes + w.code_off[1];
  const uint8_t* c0 = codes + w.code_off[0];
  for (int c = 0; c < w.ncodes[2]; ++c) {
    const Mask m{ctop, c};
    const int base2 = w.mult[2] * c;
    if (mass(ptop, top, m, gl) == 0.0) {
      for (int d = 0; d < w.ncodes[1]; ++d) zero_out(w.ncodes[0], w.mult[0], base2 + w.mult[1] * d, dst, gl);
      continue;
    }
    step(pmid, F, top, m, u, gl);
    for (int d = 0; d < w.ncodes[1]; ++d) {
      const Mask m1{c1, d};
      const int base = base2 + w.mult[1] * d;
      if (mass(pmid, u, m1, gl) == 0.0) {
        zero_out(w.ncodes[0], w.mult[0], base, dst, gl);
        continue;
      }
      step(plow, F, u, m1, v, gl);
      bin_out(plow, v, c0, w.ncodes[0], w.mult[0], base, dst, gl);
    }
  }
}

__global__ void __launch_bounds__(64 * kWaves)
    codon_kernel(const DevSampler* __restrict__ smp_dev, CodonTables t, int n, const double* __restrict__ fwd,
                 size_t forward_size, const double* __restrict__ loglik, double* __restrict__ scratch,
                 double* __restrict__ windows, double* __restrict__ genes) {
  const DevSampler& smp = *smp_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane % kG;
  const int slot = (blockIdx.x * kWaves + wave) * kPerWave + lane / kG;
  const int slots = gridDim.x * kWaves * kPerWave;
  double* buf = scratch + (size_t)slot * 4 * (size_t)t.max_vec;
  const size_t wsize = (size_t)t.n_window * 125;
  for (int s = slot; s < n; s += slots) {  // (a whole group takes a sample: the shuffles stay within groups of 16)
    double* wout = windows + (size_t)s * wsize;
    double* gout = genes + (size_t)s * t.n_genes;
    if (!isfinite(loglik[s])) {  // overflowed row, or a schedule K0c rejected
      for (size_t k = gl; k < wsize; k += kG) wout[k] = __builtin_nan("");
      for (int k = gl; k < t.n_genes; k += kG) gout[k] = __builtin_nan("");
      continue;
    }
    const double* F = fwd + (size_t)s * forward_size;
    double* cur = buf;
    double* oth = buf + t.max_vec;
    double* u = buf + 2 * (size_t)t.max_vec;
    double* v = buf + 3 * (size_t)t.max_vec;
    int q = t.n_pos - 1;
    {
      const Pos pj = position(smp, q);
      const double* fj = F + pj.off;
      double tj = 0.0;
      for (int g = gl; g < pj.n_genes; g += kG) tj += fj[g];
      tj = group_sum(tj);
      for (int g = gl; g < pj.n_genes; g += kG) {
        const double p = fj[g] / tj;
        cur[g] = p;
        gout[t.n_genes - pj.n_genes + g] = p;
      }
    }
    int wi = 0;
    for (; q >= 1; --q) {
      while (wi < t.n_window && t.win[wi].top == q) {
        const CodonWindow w = t.win[wi];
        window(smp, w, t.codes, F, cur, u, v, wout + (size_t)w.out * 125, gl);
        ++wi;
      }
      const Pos pb = position(smp, q - 1);
      step(pb, F, cur, Mask{nullptr, -1}, oth, gl);
      double* x = cur;
      cur = oth;
      oth = x;
      if (pb.kind == 0) {
        const int g0 = q - 1 == 0 ? 0 : smp.n_v;
        for (int g = gl; g < pb.n_genes; g += kG) gout[g0 + g] = cur[g];
      }
    }
  }
}

}  // namespace

int codon_slots(int n) {
  const int per_block = kWaves * kPerWave;
  return std::min((n + per_block - 1) / per_block, debug_options().codon_blocks) * per_block;
}

void launch_codons(const DevSampler* smp_dev, const CodonTables& t, int n, const double* fwd, size_t forward_size,
                   const double* loglik, double* scratch, double* windows, double* genes, hipStream_t stream) {
  if (n <= 0) return;
  const int per_block = kWaves * kPerWave;
  hipLaunchKernelGGL(codon_kernel, dim3(codon_slots(n) / per_block), dim3(64 * kWaves), 0, stream, smp_dev, t, n, fwd,
                     forward_size, loglik, scratch, windows, genes);
}

}  // namespace lh
