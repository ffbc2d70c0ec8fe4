// K10: exact posteriors of the recombination events on the device (gfx950): per junction, where the left gene stops,
// where the right gene starts, and the joint of the two (whose diagonals are the insertion-length distribution).
//
// A state path with non-zero probability reads  left-germline* NTI* right-germline*  on a junction's W rows
// (FillTransition, src/HMM.cpp:964-1089).  With  a = rows the left gene l occupies  and  b = first row of the right
// gene r's germline states (W: none)  the kernel writes, per sample and junction,
//   exit [nL][W+1] = P(l, a),   enter[nR][W+1] = P(r, b),   span[W+1][W+1] = P(a, b)   (zero below the diagonal).
// exit and enter are differences of K5's posteriors pi (lh_posterior.hip), the regions' gene posteriors standing in as
// rows -1 and W:
//   exit[l][a] = pi_{a-1}(left l) - pi_a(left l),       enter[r][b] = pi_b(germ r) - pi_{b-1}(germ r).
// span is a run-length statistic, which no per-row marginal holds: for every (r, b) the mass pi_b(germ r) steps back
// through K5's conditional  C_i[k, k2] = F[i, k] T(k -> k2) / Z_i(k2);  what lands on left-germline states of row i is
// span[i+1][b], what lands on r's four NTI states goes on, what lands on r's germline state is dropped (b would not be
// its first row).  An NTI state carries its right gene, so the chain is a 4-vector per (r, b) under the gene's 4 x 4
// nti_transition.  Only ratios inside one forward row appear, as in K5: the rows' rescalings cancel.
//
// Two phases per junction, lanes as K4 / K5 / K9 (sixteen lanes per sample, four samples per wave; lane gl owns left
// genes and right genes gl, gl + 16, ...):
//   tabulate  per (row i, right gene r): the reciprocals of K5's normalisers Z_i(NTI b of r on row i + 1) and
//             Z_i(germ r on row i + 1) -- on the last row, of the right region's gene r -- and  A_i gp_r  (on the last
//             row  A_i gp_r exit_li_r prod_r), with K5's A_i = sum_l left_lo[i][l] F[i, l]: six doubles, in the sample
//             slot's scratch area (W nR 4 doubles do not fit the LDS for a 70-D family).  1 / Z is 0 where Z is 0: the
//             mass that would be divided by it is 0 too (K5's rule).
//   chains    for every round of sixteen right genes, every b and every row below it the lanes walk their genes' chains
//             in step; a cell's sixteen contributions are added by the butterfly (every lane the same bits, fixed order)
//             and lane 0 adds the rounds up in ascending order in the output.  No atomics.
// Every scratch and output entry is written and read back by one lane only.  No private array is reached by a dynamic
// index: a chain's vector is four named variables.  The grid is capped (DebugOptions::events_blocks): a lane group takes
// samples slot, slot + slots, ... and keeps its scratch area.
#include <algorithm>
#include <cmath>

#include "lh_device.h"
#include "lh_smooth.h"

namespace lh {

namespace {

using namespace smooth;  // the lane groups and K5's normalisers

constexpr int kTab = 6;  // doubles per (row, right gene) of the scratch table

__device__ inline double recip(double z) { return z != 0.0 ? 1.0 / z : 0.0; }

// tab[i][r][0..3] = 1 / Z_i(NTI b of r, row i + 1), [4] = 1 / Z_i(germ r, row i + 1 | the right region's gene r),
// [5] = the weight of "every left gene's row-i state" into those successors, less the successor's own factor
__device__ void tabulate(const DevSampleJunction& J, const double* __restrict__ F, double* __restrict__ tab, int gl) {
  const int nL = J.n_left, nR = J.n_right, W = J.n_rows;
  const size_t stride = row_stride(J);
  for (int i = 0; i < W; ++i) {
    const double* f = F + (size_t)i * stride;
    const double* fN = f + nL;
    const double* fR = f + nL + 4 * (size_t)nR;
    const double a = left_weight(J, i, J.left_lo + (size_t)i * nL, f, gl);
    for (int r = gl; r < nR; r += kG) {
      double* t = tab + ((size_t)i * nR + r) * kTab;
      const double f0 = fN[(size_t)r * 4 + 0], f1 = fN[(size_t)r * 4 + 1], f2 = fN[(size_t)r * 4 + 2],
                   f3 = fN[(size_t)r * 4 + 3];
      const double fg = i >= J.right_first[r] ? fR[r] : 0.0;
      if (i + 1 < W) {
        const RightGene g = right_gene(J, i + 1, r);
        const RowNorm n = row_normalisers(J, i + 1, r, g, a, f0, f1, f2, f3, fg);
        t[0] = recip(n.z0);
        t[1] = recip(n.z1);
        t[2] = recip(n.z2);
        t[3] = recip(n.z3);
        t[4] = n.germ_next ? recip(n.zg) : 0.0;
        t[5] = g.gp * a;
      } else {
        const LastNorm n = last_normaliser(J, r, a, f0, f1, f2, f3, fg);
        t[0] = t[1] = t[2] = t[3] = 0.0;
        t[4] = recip(n.z);
        t[5] = n.c * a;
      }
    }
  }
}

// lane 0 keeps the cell: the first round sets it, the later ones add to it in order
__device__ inline void cell(double* __restrict__ span, int W1, int a, int b, double v, bool first, int gl) {
  v = group_sum(v);
  if (gl == 0) {
    double* p = span + (size_t)a * W1 + b;
    *p = first ? v : *p + v;
  }
}

struct Step {  // named members, not an array: nothing here is reached by a dynamic index
  double z0, z1, z2, z3, ag, f0, f1, f2, f3;
};

// F: the junction's forward rows; P: its posteriors (K5); pg: the posterior of the right region's genes
__device__ void span_chains(const DevSampleJunction& J, const double* __restrict__ F, const double* __restrict__ P,
                            const double* __restrict__ pg, const double* __restrict__ tab, double* __restrict__ span,
                            int gl) {
  const int nL = J.n_left, nR = J.n_right, W = J.n_rows, W1 = W + 1;
  const size_t stride = row_stride(J);
  const size_t oN = nL, oR = (size_t)nL + 4 * (size_t)nR;
  for (int k = gl; k < W1 * W1; k += kG)
    if (k / W1 > k % W1) span[k] = 0.0;  // below the diagonal (no chain comes there)
  for (int r0 = 0; r0 < nR; r0 += kG) {
    const int r = r0 + gl;
    const bool have = r < nR;
    const bool first = r0 == 0;
    const int rr = have ? r : 0;  // (a lane without a gene walks gene 0's tables)
    const double* ntt = J.ntt + (size_t)rr * 16;
    const double* nli = J.nli + (size_t)rr * 4;
    const double t00 = ntt[0], t01 = ntt[1], t02 = ntt[2], t03 = ntt[3], t10 = ntt[4], t11 = ntt[5], t12 = ntt[6],
                 t13 = ntt[7], t20 = ntt[8], t21 = ntt[9], t22 = ntt[10], t23 = ntt[11], t30 = ntt[12], t31 = ntt[13],
                 t32 = ntt[14], t33 = ntt[15];
    const double n0 = nli[0], n1 = nli[1], n2 = nli[2], n3 = nli[3];
    const int rf = J.right_first[rr];
    // (that lane's table entries belong to another lane: whatever it reads of them is discarded here)
    auto put = [&](int a, int b, double v) { cell(span, W1, a, b, have ? v : 0.0, first, gl); };
    // what the step from row i + 1 down to row i reads of row i
    auto fetch = [&](int i) {
      const double* t = tab + ((size_t)i * nR + rr) * kTab;
      const double* f = F + (size_t)i * stride + oN + (size_t)rr * 4;
      return Step{t[0], t[1], t[2], t[3], t[5], f[0], f[1], f[2], f[3]};
    };
    for (int b = 0; b <= W; ++b) {
      // the mass that has a germline state of r on row b (b = W: the right region's gene r)
      double m = 0.0;
      if (have) m = b == W ? pg[r] : (b >= rf ? P[(size_t)b * stride + oR + r] : 0.0);
      if (b == 0) {  // no row before it: the left gene has no junction row either
        put(0, 0, m);
        continue;
      }
      // the step from row b down to row b - 1: left genes close the chain, NTI states carry it on
      const int ib = b - 1;
      const double* tb = tab + ((size_t)ib * nR + rr) * kTab;
      const double* fb = F + (size_t)ib * stride + oN + (size_t)rr * 4;
      const double rho = m * tb[4];
      double v0, v1, v2, v3;
      if (b == W) {
        const double* xn = J.exit_nlo + (size_t)rr * 4;
        put(b, b, tb[5] * rho);
        v0 = fb[0] * (xn[0] * rho), v1 = fb[1] * (xn[1] * rho), v2 = fb[2] * (xn[2] * rho), v3 = fb[3] * (xn[3] * rho);
      } else {
        const double* nlo = J.nlo + ((size_t)b * nR + rr) * 4;
        const double li = b >= rf ? J.li[(size_t)b * nR + rr] : 0.0;
        put(b, b, (tb[5] * li) * rho);
        v0 = fb[0] * (nlo[0] * rho), v1 = fb[1] * (nlo[1] * rho), v2 = fb[2] * (nlo[2] * rho), v3 = fb[3] * (nlo[3] * rho);
      }
      // (v0 .. v3) sits on row i + 1.  What a step loads does not depend on the chain: the next row's table entry and
      // forward values are fetched a step ahead, so that the chain waits for arithmetic only.
      Step cur = b >= 2 ? fetch(b - 2) : Step{};
      for (int i = b - 2; i >= 0; --i) {
        const Step nxt = i > 0 ? fetch(i - 1) : cur;
        const double q0 = v0 * cur.z0, q1 = v1 * cur.z1, q2 = v2 * cur.z2, q3 = v3 * cur.z3;
        put(i + 1, b, cur.ag * (n0 * q0 + n1 * q1 + n2 * q2 + n3 * q3));
        v0 = cur.f0 * (t00 * q0 + t01 * q1 + t02 * q2 + t03 * q3);
        v1 = cur.f1 * (t10 * q0 + t11 * q1 + t12 * q2 + t13 * q3);
        v2 = cur.f2 * (t20 * q0 + t21 * q1 + t22 * q2 + t23 * q3);
        v3 = cur.f3 * (t30 * q0 + t31 * q1 + t32 * q2 + t33 * q3);
        cur = nxt;
      }
      // row 0's NTI states have the left region's genes as their only predecessors
      put(0, b, (v0 + v1) + (v2 + v3));
    }
  }
}

// P: the junction's posteriors; pl, pg: the posteriors of the left and right regions' genes
__device__ void differences(const DevSampleJunction& J, const double* __restrict__ P, const double* __restrict__ pl,
                            const double* __restrict__ pg, double* __restrict__ exit_t, double* __restrict__ enter_t,
                            int gl) {
  const int nL = J.n_left, nR = J.n_right, W = J.n_rows, W1 = W + 1;
  const size_t stride = row_stride(J);
  const size_t oR = (size_t)nL + 4 * (size_t)nR;
  for (int l = gl; l < nL; l += kG) {
    const int rows = J.left_rows[l];
    double prev = pl[l];
    for (int a = 0; a <= W; ++a) {
      const double cur = a < rows ? P[(size_t)a * stride + l] : 0.0;
      exit_t[(size_t)l * W1 + a] = prev - cur;
      prev = cur;
    }
  }
  for (int r = gl; r < nR; r += kG) {
    const int rf = J.right_first[r];
    double prev = 0.0;
    for (int b = 0; b <= W; ++b) {
      const double cur = b == W ? pg[r] : (b >= rf ? P[(size_t)b * stride + oR + r] : 0.0);
      enter_t[(size_t)r * W1 + b] = cur - prev;
      prev = cur;
    }
  }
}

__device__ void junction_events(const DevSampleJunction& J, const double* __restrict__ F, const double* __restrict__ P,
                                const double* __restrict__ pl, const double* __restrict__ pg, double* __restrict__ tab,
                                double* __restrict__ out, int gl) {
  const int W1 = J.n_rows + 1;
  double* exit_t = out;
  double* enter_t = exit_t + (size_t)J.n_left * W1;
  double* span = enter_t + (size_t)J.n_right * W1;
  differences(J, P, pl, pg, exit_t, enter_t, gl);
  tabulate(J, F, tab, gl);
  span_chains(J, F, P, pg, tab, span, gl);
}

__global__ void __launch_bounds__(64 * kWaves)
    events_kernel(const DevSampler* __restrict__ smp_dev, int n, const double* __restrict__ fwd,
                  const double* __restrict__ post, size_t forward_size, const double* __restrict__ loglik,
                  double* __restrict__ scratch, size_t scratch_size, double* __restrict__ events, size_t events_size,
                  double* __restrict__ genes) {
  const DevSampler& smp = *smp_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane % kG;
  const int slot = (blockIdx.x * kWaves + wave) * kPerWave + lane / kG;
  const int slots = gridDim.x * kWaves * kPerWave;
  double* tab = scratch + (size_t)slot * scratch_size;
  const DevSampleJunction& VD = smp.vd;
  const DevSampleJunction& DJ = smp.dj;
  const int nV = smp.n_v, nD = smp.has_d ? smp.n_d : 0, nJ = smp.n_j;
  const ForwardLayout lay = forward_layout(smp);
  const size_t o_vd = lay.o_vd, o_d = lay.o_d, o_dj = lay.o_dj, o_j = lay.o_j;
  const size_t vd_out = ((size_t)VD.n_left + VD.n_right + VD.n_rows + 1) * (VD.n_rows + 1);
  const size_t vd_tab = (size_t)VD.n_rows * VD.n_right * kTab;  // each junction has its own table
  const int n_genes = nV + nD + nJ;
  for (int s = slot; s < n; s += slots) {  // (a whole group takes a sample: the shuffles stay within groups of 16)
    double* ev = events + (size_t)s * events_size;
    double* gout = genes ? genes + (size_t)s * n_genes : nullptr;
    if (!isfinite(loglik[s])) {  // overflowed row, or a schedule K0c rejected
      for (size_t k = gl; k < events_size; k += kG) ev[k] = __builtin_nan("");
      if (gout)
        for (int k = gl; k < n_genes; k += kG) gout[k] = __builtin_nan("");
      continue;
    }
    const double* F = fwd + (size_t)s * forward_size;
    const double* P = post + (size_t)s * forward_size;
    if (gout) {
      for (int g = gl; g < nV; g += kG) gout[g] = P[g];
      for (int g = gl; g < nD; g += kG) gout[nV + g] = P[o_d + g];
      for (int g = gl; g < nJ; g += kG) gout[nV + nD + g] = P[o_j + g];
    }
    if (smp.has_d) {
      junction_events(VD, F + o_vd, P + o_vd, P, P + o_d, tab, ev, gl);
      junction_events(DJ, F + o_dj, P + o_dj, P + o_d, P + o_j, tab + vd_tab, ev + vd_out, gl);
    } else {
      junction_events(VD, F + o_vd, P + o_vd, P, P + o_j, tab, ev, gl);
    }
  }
}

}  // namespace

int events_slots(int n) {
  const int per_block = kWaves * kPerWave;
  return std::min((n + per_block - 1) / per_block, debug_options().events_blocks) * per_block;
}

size_t events_scratch_doubles(const DevSampler& smp) {
  const size_t vd = (size_t)smp.vd.n_rows * smp.vd.n_right, dj = smp.has_d ? (size_t)smp.dj.n_rows * smp.dj.n_right : 0;
  return std::max<size_t>((vd + dj) * kTab, 1);
}

void launch_events(const DevSampler& smp, const DevSampler* smp_dev, int n, const double* fwd, const double* post,
                   size_t forward_size, const double* loglik, double* scratch, double* events, size_t events_size,
                   double* genes, hipStream_t stream) {
  if (n <= 0) return;
  const int per_block = kWaves * kPerWave;
  hipLaunchKernelGGL(events_kernel, dim3(events_slots(n) / per_block), dim3(64 * kWaves), 0, stream, smp_dev, n, fwd, post,
                     forward_size, loglik, scratch, events_scratch_doubles(smp), events, events_size, genes);
}

}  // namespace lh
