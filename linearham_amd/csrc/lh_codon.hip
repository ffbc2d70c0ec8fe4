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
#include "lh_smooth.h"

namespace lh {

namespace {

using namespace smooth;  // the lane groups and the three step forms K5, K9 and K10 share

// the entries of a vector that carry local code `want` (want < 0: all of them); the step forms' reader of `next`
struct Mask {
  const uint8_t* code;
  int want;
  __device__ double operator()(const double* __restrict__ v, size_t k) const {
    return (want < 0 || code[k] == want) ? v[k] : 0.0;
  }
};

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
  const ForwardLayout lay = forward_layout(smp);
  if (q == 0) return Pos{0, &VD, 0, lay.o_v, smp.n_v};
  if (q <= VD.n_rows) return Pos{1, &VD, q - 1, lay.o_vd + (size_t)(q - 1) * row_stride(VD), 0};
  q -= VD.n_rows + 1;
  if (!smp.has_d) return Pos{0, nullptr, 0, lay.o_j, smp.n_j};
  if (q == 0) return Pos{0, &DJ, 0, lay.o_d, smp.n_d};
  if (q <= DJ.n_rows) return Pos{1, &DJ, q - 1, lay.o_dj + (size_t)(q - 1) * row_stride(DJ), 0};
  return Pos{0, nullptr, 0, lay.o_j, smp.n_j};
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
  for_owned(p, gl, [&](size_t k) { a += m(v, k); });
  return group_sum(a);
}

// out = the smoothing step from position p + 1 down to p (p is never the last position), out of place and with a mask on
// the vector it is handed.  The step forms promise nothing about their arrays: the __restrict__ here tells them that K9's
// three are distinct.
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
