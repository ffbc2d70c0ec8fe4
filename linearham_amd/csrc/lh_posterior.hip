// K5: exact posterior state marginals on the device (gfx950): forward filtering / backward smoothing over the
// compact forward arrays K2b writes, in the layout of lh_eval_outputs.forward.
//
// Each step is the expected value of K4's draw at that step (lh_sample.hip): the same weights F[i, k] T(k -> k2), the
// same normaliser Z(k2) = sum_k' F[i, k'] T(k' -> k2), so
//   pi_i(k) = sum_{k2 in succ(k)} pi_{i+1}(k2) F[i, k] T(k -> k2) / Z(k2),
// starting from pi_J(g) = f_J[g] / sum f_J and ending with the germline regions left of each junction (D, then V).
// Only ratios within one forward row or one region vector appear: the rows' 2^256 rescalings (ScaleMatrix counts, or
// the extended-range mode's) cancel and are not read.  A term with pi_{i+1}(k2) = 0 contributes 0, also where Z = 0.
//
// The transition structure FillTransition writes (src/HMM.cpp:964-1089) makes a row O(nL + 16 nR): the successors of
// row i are, per right gene r, its four NTI states and its germline state of row i + 1 (or, on the last row, the gene
// of the region right of the junction), plus each left gene's own state of row i + 1.  For a right-gene successor s
// the weights are  (left_lo[i][l] * c_s) F[i, l]  for every left gene l,  t_s[a] F[i, NTI a of r],  g_s F[i, germ r];
// so with  A_i = sum_l left_lo[i][l] F[i, l]  and  rho_s = pi_{i+1}(s) / Z_s:
//   pi_i(NTI a of r) = F[i, NTI a of r] * sum_s t_s[a] rho_s
//   pi_i(germ r)     = F[i, germ r] * sum_s g_s rho_s
//   pi_i(left l)     = pi_{i+1}(left l) + F[i, l] left_lo[i][l] * B_i,    B_i = sum_r sum_s c_s rho_s
// (a left gene's own next-row state has that state as its only predecessor: its weight cancels).
//
// SIXTEEN LANES per sample, four samples per wave, as K4: lane gl of a group owns left genes gl, gl + 16, ... and
// right genes gl, gl + 16, ...; A_i and B_i are butterfly sums over the group (__shfl_xor: both partners add the same two
// values, so every lane ends with the same bits, and the order is fixed).  Every entry is read and written by its
// owner only, and all of a row's reads precede its writes in that lane's program order: the posteriors overwrite the
// forward arrays in place (pi_{i+1} is read back from where the same lane wrote it).  No private array is reached by
// a dynamic index: the five successors of a right gene are named variables.
#include <cmath>

#include "lh_device.h"
#include "lh_smooth.h"

namespace lh {

namespace {

using namespace smooth;  // the lane groups and the three step forms K5, K9 and K10 share

// Row i = 0 .. W-2 in place: `row` holds the forward row i on entry and pi_i on exit; next = pi_{i+1}, another row.  The
// step forms promise nothing about their arrays; these three forward to them only to carry __restrict__: `row` (read and
// written) against `next` and the tables.
__device__ inline void smooth_row(const DevSampleJunction& J, int i, double* __restrict__ row,
                                  const double* __restrict__ next, int gl) {
  step_row(J, i, row, next, Direct{}, row, gl);
}
// Row W-1: the successor is the gene of the region right of the junction, whose posterior is pg[nR].
__device__ inline void smooth_last_row(const DevSampleJunction& J, double* __restrict__ row, const double* __restrict__ pg,
                                       int gl) {
  step_last(J, row, pg, Direct{}, row, gl);
}
// The germline region left of the junction: f[nL] holds its forward vector on entry and its gene posterior on exit;
// p0 = pi_0 of the junction.
__device__ inline void smooth_left_region(const DevSampleJunction& J, double* __restrict__ f,
                                          const double* __restrict__ p0, int gl) {
  step_left(J, f, p0, Direct{}, f, gl);
}

__device__ void smooth_junction(const DevSampleJunction& J, double* __restrict__ rows, const double* __restrict__ pg, int gl) {
  const size_t stride = row_stride(J);
  const int W = J.n_rows;
  smooth_last_row(J, rows + (size_t)(W - 1) * stride, pg, gl);
  for (int i = W - 2; i >= 0; --i) smooth_row(J, i, rows + (size_t)i * stride, rows + (size_t)(i + 1) * stride, gl);
}

__global__ void __launch_bounds__(64 * kWaves)
    posterior_kernel(const DevSampler* __restrict__ smp_dev, int n, double* __restrict__ post_all, size_t forward_size,
                     const double* __restrict__ loglik) {
  const DevSampler& smp = *smp_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane % kG;
  const int s = (blockIdx.x * kWaves + wave) * kPerWave + lane / kG;
  if (s >= n) return;  // (a whole group leaves: the shuffles stay within groups of 16)
  double* p = post_all + (size_t)s * forward_size;
  if (!isfinite(loglik[s])) {  // overflowed row, or a schedule K0c rejected: no posterior
    for (size_t k = gl; k < forward_size; k += kG) p[k] = __builtin_nan("");
    return;
  }
  const DevSampleJunction& VD = smp.vd;
  const DevSampleJunction& DJ = smp.dj;
  const int nJ = smp.n_j;
  const ForwardLayout lay = forward_layout(smp);
  double* p_v = p + lay.o_v;
  double* p_vd = p + lay.o_vd;
  double* p_d = p + lay.o_d;
  double* p_dj = p + lay.o_dj;
  double* p_j = p + lay.o_j;
  double tj = 0.0;
  for (int g = gl; g < nJ; g += kG) tj += p_j[g];
  tj = group_sum(tj);
  for (int g = gl; g < nJ; g += kG) p_j[g] = p_j[g] / tj;
  if (smp.has_d) {
    smooth_junction(DJ, p_dj, p_j, gl);
    smooth_left_region(DJ, p_d, p_dj, gl);
    smooth_junction(VD, p_vd, p_d, gl);
  } else {
    smooth_junction(VD, p_vd, p_j, gl);
  }
  smooth_left_region(VD, p_v, p_vd, gl);
}

// ---- weighted reduction: sum_i w_i pi_i over a batch, w_i = exp(lw_i - max lw), in a fixed order ----

constexpr int kRedThreads = 256;
constexpr int kSlab = 256;  // samples per partial sum

// One workgroup: max over the finite lw_i, then w_i (0 where lw_i is not finite), sum w and sum w^2 -- each a fixed
// tree over fixed per-thread strides.
__global__ void __launch_bounds__(kRedThreads)
    weight_kernel(int n, const double* __restrict__ loglik, const double* __restrict__ log_offset, double* __restrict__ w,
                  double* __restrict__ stats) {
  __shared__ double red[kRedThreads];
  const int t = threadIdx.x;
  auto lw_of = [&](int i) { return loglik[i] - (log_offset ? log_offset[i] : 0.0); };
  double m = -INFINITY;
  for (int i = t; i < n; i += kRedThreads) {
    const double v = lw_of(i);
    if (isfinite(v)) m = fmax(m, v);
  }
  red[t] = m;
  __syncthreads();
  for (int h = kRedThreads / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
  for (int i = t; i < n; i += kRedThreads) {
    const double v = lw_of(i);
    const double wi = isfinite(v) ? exp(v - m) : 0.0;
    w[i] = wi;
    s1 += wi;
    s2 += wi * wi;
  }
  for (int k = 0; k < 2; ++k) {
    red[t] = k == 0 ? s1 : s2;
    __syncthreads();
    for (int h = kRedThreads / 2; h > 0; h >>= 1) {
      if (t < h) red[t] = red[t] + red[t + h];
      __syncthreads();
    }
    if (t == 0) stats[1 + k] = red[0];
    __syncthreads();
  }
  if (t == 0) stats[0] = m;
}

// partial[slab][j] = sum over the slab's samples i, in order, of w_i post[i][j] (samples with w_i == 0 skipped: their
// posteriors may be NaN).  Thread j of the grid's x dimension: consecutive entries, coalesced.
__global__ void __launch_bounds__(kRedThreads)
    slab_kernel(int n, size_t forward_size, const double* __restrict__ post, const double* __restrict__ w,
                double* __restrict__ partial) {
  const size_t j = (size_t)blockIdx.x * kRedThreads + threadIdx.x;
  const int slab = blockIdx.y;
  if (j >= forward_size) return;
  const int i0 = slab * kSlab, i1 = min(n, i0 + kSlab);
  double acc = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double wi = w[i];
    if (wi != 0.0) acc += wi * post[(size_t)i * forward_size + j];
  }
  partial[(size_t)slab * forward_size + j] = acc;
}

__global__ void __launch_bounds__(kRedThreads)
    slab_sum_kernel(int n_slabs, size_t forward_size, const double* __restrict__ partial, double* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (j >= forward_size) return;
  double acc = 0.0;
  for (int k = 0; k < n_slabs; ++k) acc += partial[(size_t)k * forward_size + j];
  out[j] = acc;
}

}  // namespace

void launch_posterior(const DevSampler* smp_dev, int n, double* post, size_t forward_size, const double* loglik,
                      hipStream_t stream) {
  const int per_block = kWaves * kPerWave;
  hipLaunchKernelGGL(posterior_kernel, dim3((n + per_block - 1) / per_block), dim3(64 * kWaves), 0, stream, smp_dev, n, post,
                     forward_size, loglik);
}

int posterior_slabs(int n) { return (n + kSlab - 1) / kSlab; }

void launch_slab_sum(int n_slabs, size_t size, const double* partial, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((size + kRedThreads - 1) / kRedThreads)), dim3(kRedThreads), 0, stream,
                     n_slabs, size, partial, out);
}

void launch_weighted_slabs(int n, size_t size, const double* rows, const double* w, double* partial, double* weighted_sum,
                           hipStream_t stream) {
  if (size == 0) return;
  const int slabs = posterior_slabs(n);
  const unsigned bx = (unsigned)((size + kRedThreads - 1) / kRedThreads);
  hipLaunchKernelGGL(slab_kernel, dim3(bx, slabs), dim3(kRedThreads), 0, stream, n, size, rows, w, partial);
  hipLaunchKernelGGL(slab_sum_kernel, dim3(bx), dim3(kRedThreads), 0, stream, slabs, size, partial, weighted_sum);
}

void launch_posterior_reduce(int n, size_t forward_size, const double* post, const double* loglik, const double* log_offset,
                             double* w, double* partial, double* weighted_sum, double* stats, hipStream_t stream) {
  hipLaunchKernelGGL(weight_kernel, dim3(1), dim3(kRedThreads), 0, stream, n, loglik, log_offset, w, stats);
  if (weighted_sum) launch_weighted_slabs(n, forward_size, post, w, partial, weighted_sum, stream);
}

}  // namespace lh
