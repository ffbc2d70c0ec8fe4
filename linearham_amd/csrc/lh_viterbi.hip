// K8: the most probable V(D)J state path of every sample (max-product sweep + trace-back), and the HMM prior of given
// paths (gfx950).
//
// Inside a germline region a path is deterministic; paths branch only in the junctions, over the left genes, the four NTI
// states of a right gene and the gene's own previous position.  So the max-product sweep is K2b's structured sweep
// (junction_kernel, lh_forward.hip) with every sum replaced by a maximum: the cross-gene rank-one term
// A = sum_l f_l landing_out_l becomes A* = max_l f_l landing_out_l, one value and one arg-max per row.  K2a's outputs
// (gem, gcnt, jem, and jrs in the extended-range mode) are read exactly as K2b reads them: a gene's germline product is
// already a single path.
//
// One form, viterbi_kernel<GA, GB, kExt>, with junction_kernel's launch shape: one wave per sample, gene g in lane g % 64,
// slot g / 64, the NTI blocks and the sample's jem slice in LDS, the padded junction tables.  Every value is >= 0, so a
// padded table entry (zero) never wins against a positive value.
//
// RESCALING.  After every row the vector is multiplied by the exact power of two that brings its LARGEST entry into
// [1, 2), and the exponents are summed in an integer (K2a's 2^-256 counts enter as multiples of 256).  The value of the
// best path is then m 2^E with m in [1, 2): a canonical form that depends on the true values only, so log_path has the
// same bits in the default and the extended-range mode and at any batch position.
//
// BACK-POINTERS, not max-forward arrays (global memory, viterbi_bp_bytes() per sample):
//   int32 argl[W_vd + 1 | W_dj + 1]         the arg-max left gene of cross term c: c = 0 out of the left germline
//                                           region, c = i + 1 out of junction row i
//   uint8 code[W][5][nR] | exit[nR]         per junction: the predecessor of (row, right gene r, state k = NTI A,C,G,T |
//                                           germline) and of r's germline region: 0 = cross term, 1..4 = own NTI base,
//                                           5 = own germline position of the row before
// The same wave traces the path back after the sweep (a release / acquire fence pair and a wave barrier in between, as
// junction_kernel's for its jem slice) and writes it in K4's layout and encoding (lh_sample.hip): J gene | D-J rows |
// D gene | V-D rows | V gene, dense state indices.
//
// TIES are broken by the values alone: the lowest left gene in a cross term; among the kinds cross < NTI A, C, G, T < own
// germline (a later kind wins only when strictly larger); the lowest gene of the final J vector.
#include <algorithm>

#include "lh_device.h"

namespace lh {

namespace {

constexpr int kVitWaves = 4;  // samples per workgroup
constexpr double kLn2 = 0.693147180559945309417;

// the largest of the wave's values (all >= 0), wave-uniform
__device__ inline double wave_max(double v) {
  v = fmax(v, dpp_move<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmax(v, dpp_move<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmax(v, dpp_move<0x141>(v));  // lane i <-> 7 - i within each 8
  v = fmax(v, dpp_move<0x140>(v));  // lane i <-> 15 - i within each 16
  return fmax(fmax(read_lane(v, 0), read_lane(v, 16)), fmax(read_lane(v, 32), read_lane(v, 48)));
}

// the lowest gene (lane + 64 slot) whose value equals the wave's maximum m
template <int G>
__device__ inline int wave_argmax(const double (&v)[G], double m) {
  int arg = 0;
  bool found = false;
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const unsigned long long hit = __builtin_amdgcn_ballot_w64(v[q] == m);
    if (!found && hit != 0) {
      arg = 64 * q + (int)__builtin_ctzll(hit);
      found = true;
    }
  }
  return arg;
}

// the exponent e that brings m into [1, 2) as m 2^-e (a subnormal or zero m: 1074, which cannot overflow)
__device__ inline int norm_exp(double m) {
  const int ef = ((unsigned)__double2hiint(m) >> 20) & 0x7ff;
  return ef ? ef - 1023 : -1074;
}

__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One junction: the max-product rows, the hand-off into the right germline region (g_out, largest entry in [1, 2)) and
// the back-pointers.  Returns the exponent of g_out (exp_in: that of f_in).
template <int GL, int GR, bool kExt>
__device__ int viterbi_junction(const DevJunction& J, const double* jem, const double* ntt_lds, int lane,
                                const double (&f_in)[GL], int exp_in, const double* __restrict__ germ_em,
                                const double* __restrict__ pad_trans, const double* __restrict__ pad_em,
                                double (&g_out)[GR], const int32_t* __restrict__ jrs, int32_t* __restrict__ argl,
                                uint8_t* __restrict__ code) {
  const int W = J.n_rows, nL = J.n_left, nR = J.n_right;
  int E = exp_in;
  double fL[GL], fN[GR][4], fR[GR], nli[GR][4];
#pragma unroll
  for (int q = 0; q < GL; ++q) fL[q] = f_in[q];
#pragma unroll
  for (int q = 0; q < GR; ++q) {
    fR[q] = 0.0;
    fN[q][0] = fN[q][1] = fN[q][2] = fN[q][3] = 0.0;
    const double2* p = reinterpret_cast<const double2*>(J.right_gp_nli) + 2u * (lane + 64u * q);
    const double2 a = p[0], b = p[1];
    nli[q][0] = a.x;
    nli[q][1] = a.y;
    nli[q][2] = b.x;
    nli[q][3] = b.y;
  }
  // cross term c: A = max_l f[l] * landing_out[l], its arg-max to argl[c]
  double A;
  auto cross = [&](int c, const double* __restrict__ lo) __attribute__((always_inline)) {
    double part[GL], m = 0.0;
#pragma unroll
    for (int q = 0; q < GL; ++q) {
      part[q] = fL[q] * lo[lane + 64u * q];
      m = fmax(m, part[q]);
    }
    A = wave_max(m);
    const int arg = wave_argmax<GL>(part, A);
    if (lane == 0) argl[c] = min(arg, nL - 1);
  };
  cross(0, J.enter_lo);

  for (int i = 0; i < W; ++i) {
    const size_t ol = (size_t)i * J.left_pad, orr = (size_t)i * J.right_pad;
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < GL; ++q) {
      const unsigned l = lane + 64u * q;
      const double v = (fL[q] * J.left_trans[ol + l]) * jem[J.left_xmsa[ol + l]];
      fL[q] = v;
      m = fmax(m, v);
    }
    uint8_t* crow = code + (size_t)i * 5 * nR;
#pragma unroll
    for (int q = 0; q < GR; ++q) {
      const unsigned r = lane + 64u * q;
      const bool live = (int)r < nR;
      const double n[4] = {fN[q][0], fN[q][1], fN[q][2], fN[q][3]};
      // NTI->NTI block of gene r, transposed in LDS: [b * 4 + a] = transition a -> b
      const double* tt = ntt_lds + 16u * r;
      const int4 nx = reinterpret_cast<const int4*>(J.nti_xmsa)[orr + r];
      const int nxs[4] = {nx.x, nx.y, nx.z, nx.w};
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double best = A * nli[q][b];
        int c = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double t = n[a] * tt[4 * b + a];
          if (t > best) {
            best = t;
            c = 1 + a;
          }
        }
        const double v = best * jem[nxs[b]];
        fN[q][b] = v;
        m = fmax(m, v);
        if (live) crow[(size_t)b * nR + r] = (uint8_t)c;
      }
      const double* nlo = J.right_nlo + 4 * (orr + r);
      double best = A * J.right_gp_li[orr + r];
      int c = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double t = n[a] * nlo[a];
        if (t > best) {
          best = t;
          c = 1 + a;
        }
      }
      {
        const double t = fR[q] * J.right_trans[orr + r];
        if (t > best) {
          best = t;
          c = 5;
        }
      }
      const double v = best * jem[J.right_xmsa[orr + r]];
      fR[q] = v;
      m = fmax(m, v);
      if (live) crow[(size_t)4 * nR + r] = (uint8_t)c;
    }
    const int e = norm_exp(wave_max(m));
#pragma unroll
    for (int q = 0; q < GL; ++q) fL[q] = ldexp(fL[q], -e);
#pragma unroll
    for (int q = 0; q < GR; ++q) {
      fR[q] = ldexp(fR[q], -e);
#pragma unroll
      for (int b = 0; b < 4; ++b) fN[q][b] = ldexp(fN[q][b], -e);
    }
    E += e;
    if constexpr (kExt) E -= 256 * jrs[i];
    cross(i + 1, J.left_lo + ol);
  }

  // hand-off into the right germline region
  double m = 0.0;
  uint8_t* cexit = code + (size_t)W * 5 * nR;
#pragma unroll
  for (int q = 0; q < GR; ++q) {
    const unsigned r = lane + 64u * q;
    const double* xn = J.exit_nlo + 4u * r;
    double best = A * J.exit_gp_li[r];
    int c = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double t = fN[q][a] * xn[a];
      if (t > best) {
        best = t;
        c = 1 + a;
      }
    }
    {
      const double t = fR[q] * J.exit_trans[r];
      if (t > best) {
        best = t;
        c = 5;
      }
    }
    double v = 0.0;
    if ((int)r < nR) {
      v = best * germ_em[r];
      if (pad_trans) v *= pad_trans[r];
      if (pad_em) v *= pad_em[r];
      cexit[r] = (uint8_t)c;
    }
    m = fmax(m, v);
    g_out[q] = v;
  }
  const int e = norm_exp(wave_max(m));
#pragma unroll
  for (int q = 0; q < GR; ++q) g_out[q] = ldexp(g_out[q], -e);
  return E + e;
}

// Follows the back-pointers of one junction from gene `right_gene` of the region right of it: out[0 .. W) receives the
// rows' dense states; returns the gene of the region left of it.  Wave-uniform; lane 0 writes.
__device__ int trace_junction(const DevSampleJunction& S, int right_gene, const int32_t* argl, const uint8_t* code,
                              int32_t* __restrict__ out, bool writer) {
  const int W = S.n_rows, nR = S.n_right, r = right_gene;
  int kind = code[(size_t)W * 5 * nR + r];
  int i = W - 1;
  while (i >= 0 && kind != 0) {
    const int k = kind == 5 ? 4 : kind - 1;
    const int dense = S.right_dense[r] + (kind == 5 ? 4 + (i - S.right_first[r]) : k);
    if (writer) out[i] = dense;
    kind = code[((size_t)i * 5 + k) * nR + r];
    --i;
  }
  // the cross term out of row i (i = -1: out of the left region): the left gene's own states from there down
  const int l = min(max(argl[i + 1], 0), S.n_left - 1);
  const int base = S.left_dense[l];
  for (; i >= 0; --i)
    if (writer) out[i] = base + i;
  return l;
}

// GA: register slots for the V genes (ceil(nV / 64)); GB: slots for the D and J genes.
template <int GA, int GB, bool kExt>
__global__ void __launch_bounds__(64 * kVitWaves)
    viterbi_kernel(const DevFamily fam, const DevSampler* __restrict__ smp_dev, int n, const double* __restrict__ gem_all,
                   const int32_t* __restrict__ gcnt_all, const double* __restrict__ jem_all,
                   const int32_t* __restrict__ jrs_all, const double* __restrict__ loglik, uint8_t* __restrict__ bp_all,
                   size_t bp_bytes, int32_t* __restrict__ states_all, double* __restrict__ log_path) {
  // [NTI->NTI blocks of the vd right genes | same for dj | kVitWaves slices of n_jcols + 1 doubles]
  extern __shared__ double vlds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * kVitWaves + wave;
  const int NJ = fam.n_jcols;
  double* ntt_vd = vlds;
  double* ntt_dj = ntt_vd + 16 * (size_t)fam.vd.right_pad;
  double* jem = ntt_dj + (fam.has_d ? 16 * (size_t)fam.dj.right_pad : 0) + (size_t)wave * (NJ + 1);
  for (int t = threadIdx.x; t < 16 * fam.vd.right_pad; t += 64 * kVitWaves) ntt_vd[t] = fam.vd.right_ntt[t];
  if (fam.has_d)
    for (int t = threadIdx.x; t < 16 * fam.dj.right_pad; t += 64 * kVitWaves) ntt_dj[t] = fam.dj.right_ntt[t];
  __syncthreads();
  if (s >= n) return;  // whole waves leave; nothing below synchronises across waves
  const DevSampler& smp = *smp_dev;
  const int S = smp.states_per_sample;
  int32_t* out = states_all + (size_t)s * S;
  const double ll = loglik[s];
  if (!isfinite(ll)) {  // (a schedule K0c rejected leaves NaN here)
    for (int j = lane; j < S; j += 64) out[j] = -1;
    if (lane == 0) log_path[s] = ll < 0.0 ? ll : __builtin_nan("");  // -inf: no path has positive probability
    return;
  }
  {
    const double* src = jem_all + (size_t)s * NJ;
    for (int j = lane; j < NJ; j += 64) jem[j] = src[j];
    if (lane == 0) jem[NJ] = 0.0;  // what a state that cannot emit at a site looks up
  }
  wave_sync();

  const int nV = fam.vgerm.n_genes, nD = fam.dgerm.n_genes, nJ = fam.jgerm.n_genes;
  const int Wvd = fam.vd.n_rows, Wdj = fam.has_d ? fam.dj.n_rows : 0;
  const double* gem = gem_all + (size_t)s * fam.gem_size;
  const int cv = gcnt_all[(size_t)s * 3 + 0], cd = gcnt_all[(size_t)s * 3 + 1], cj = gcnt_all[(size_t)s * 3 + 2];
  const int32_t* jrs = kExt ? jrs_all + (size_t)s * (Wvd + Wdj) : nullptr;
  uint8_t* bp = bp_all + (size_t)s * bp_bytes;
  int32_t* argl_vd = reinterpret_cast<int32_t*>(bp);
  int32_t* argl_dj = argl_vd + Wvd + 1;
  uint8_t* code_vd = reinterpret_cast<uint8_t*>(argl_dj + (fam.has_d ? Wdj + 1 : 0));
  uint8_t* code_dj = code_vd + ((size_t)Wvd * 5 + 1) * fam.vd.n_right;

  // the V germline region (as junction_kernel)
  double gV[GA], m = 0.0;
#pragma unroll
  for (int q = 0; q < GA; ++q) {
    const int t = lane + 64 * q;
    double v = 0.0;
    if (t < nV) {
      v = fam.vgerm_gene_prob[t];
      v *= fam.vpadding_transition[t];
      v *= gem[t];
      v *= fam.vgerm_trans_prod[t];
      v *= gem[nV + t];
    }
    m = fmax(m, v);
    gV[q] = v;
  }
  int E = norm_exp(wave_max(m));
#pragma unroll
  for (int q = 0; q < GA; ++q) gV[q] = ldexp(gV[q], -E);
  E -= 256 * cv;

  double gJ[GB];
  if (fam.has_d) {
    double gD[GB];
    const double* dgerm_em = gem + 2 * (size_t)nV;
    const double* jgerm_em = dgerm_em + nD;
    const double* jpad_em = jgerm_em + nJ;
    E = viterbi_junction<GA, GB, kExt>(fam.vd, jem, ntt_vd, lane, gV, E, dgerm_em, nullptr, nullptr, gD, jrs, argl_vd,
                                       code_vd) -
        256 * cd;
    E = viterbi_junction<GB, GB, kExt>(fam.dj, jem, ntt_dj, lane, gD, E, jgerm_em, fam.jpadding_transition, jpad_em, gJ,
                                       kExt ? jrs + Wvd : nullptr, argl_dj, code_dj) -
        256 * cj;
  } else {
    const double* jgerm_em = gem + 2 * (size_t)nV;
    const double* jpad_em = jgerm_em + nJ;
    E = viterbi_junction<GA, GB, kExt>(fam.vd, jem, ntt_vd, lane, gV, E, jgerm_em, fam.jpadding_transition, jpad_em, gJ,
                                       jrs, argl_vd, code_vd) -
        256 * cj;
  }
  double mj = 0.0;
#pragma unroll
  for (int q = 0; q < GB; ++q) mj = fmax(mj, gJ[q]);  // zero beyond the last J gene
  mj = wave_max(mj);
  if (!(mj > 0.0)) {
    for (int j = lane; j < S; j += 64) out[j] = -1;
    if (lane == 0) log_path[s] = -__builtin_inf();
    return;
  }
  const int jg = min(wave_argmax<GB>(gJ, mj), nJ - 1);
  if (lane == 0) log_path[s] = log(mj) + (double)E * kLn2;

  // trace-back: the back-pointers were written by all lanes of this wave
  wave_sync();
  const bool writer = lane == 0;
  int o = 0;
  if (writer) out[o] = jg;
  ++o;
  int left;
  if (fam.has_d) {
    const int dg = trace_junction(smp.dj, jg, argl_dj, code_dj, out + o, writer);
    o += Wdj;
    if (writer) out[o] = dg;
    ++o;
    left = trace_junction(smp.vd, dg, argl_vd, code_vd, out + o, writer);
  } else {
    left = trace_junction(smp.vd, jg, argl_vd, code_vd, out + o, writer);
  }
  o += Wvd;
  if (writer) out[o] = left;
}

size_t viterbi_lds(const DevFamily& fam) {
  return ((size_t)kVitWaves * (fam.n_jcols + 1) + 16 * ((size_t)fam.vd.right_pad + (fam.has_d ? fam.dj.right_pad : 0))) *
         sizeof(double);
}

template <int GA, int GB, bool kExt>
void launch_viterbi_e(const DevFamily& fam, const DevSampler* smp_dev, int n, const double* gem, const int32_t* gcnt,
                      const double* jem, const int32_t* jrs, const double* loglik, uint8_t* bp, int32_t* states,
                      double* log_path, hipStream_t stream) {
  launch_lds(viterbi_kernel<GA, GB, kExt>, dim3((n + kVitWaves - 1) / kVitWaves), dim3(64 * kVitWaves), viterbi_lds(fam),
             stream, fam, smp_dev, n, gem, gcnt, jem, jrs, loglik, bp, viterbi_bp_bytes(fam), states, log_path);
}

template <int GA>
void launch_viterbi_a(int gb, bool ext, const DevFamily& fam, const DevSampler* smp_dev, int n, const double* gem,
                      const int32_t* gcnt, const double* jem, const int32_t* jrs, const double* loglik, uint8_t* bp,
                      int32_t* states, double* log_path, hipStream_t stream) {
#define LH_ARGS fam, smp_dev, n, gem, gcnt, jem, jrs, loglik, bp, states, log_path, stream
#define LH_GB(G)                             \
  {                                          \
    if (ext)                                 \
      launch_viterbi_e<GA, G, true>(LH_ARGS); \
    else                                     \
      launch_viterbi_e<GA, G, false>(LH_ARGS); \
  }
  if (gb <= 1)
    LH_GB(1)
  else if (gb <= 2)
    LH_GB(2)
  else
    LH_GB(4)
#undef LH_GB
#undef LH_ARGS
}

// ---- path priors ----

struct PathState {
  int kind;  // -1: the gene of the region left of the junction; 0 left-gene state, 1 NTI, 2 right germline; 3: the region right of it
  int gene, base;
};

// log of the junction's share of the path's weight with every emission 1: the transitions from gene `left` of the region
// left of it through the rows' states st[0 .. W) into gene `right` of the region right of it, in the unfused factors of
// DevSampleJunction.  ok = false: a state index out of range or not of its row, or a transition of probability 0.
__device__ double junction_log_prior(const DevSampleJunction& J, int left, const int32_t* __restrict__ st, int right,
                                     bool& ok) {
  const int W = J.n_rows, nL = J.n_left, nR = J.n_right;
  double lp = 0.0;
  PathState prev{-1, left, 0};
  for (int i = 0; i <= W && ok; ++i) {
    PathState sc{3, right, 0};
    if (i < W) {
      const int dense = st[i];
      if (dense < 0 || dense >= J.n_states) {
        ok = false;
        break;
      }
      const int c = J.state_class[dense];
      sc = PathState{c & 3, c >> 4, (c >> 2) & 3};
      if (sc.kind == 0) {
        const int row = dense - J.left_dense[sc.gene];
        if (row != i || row >= J.left_rows[sc.gene]) ok = false;
      } else if (sc.kind == 2) {
        const int off = dense - J.right_dense[sc.gene] - 4;
        if (off < 0 || J.right_first[sc.gene] + off != i) ok = false;
      } else if (sc.kind == 1) {
        if (dense != J.right_dense[sc.gene] + sc.base) ok = false;
      } else {
        ok = false;
      }
      if (!ok) break;
    }
    const int r = sc.gene;  // right gene for kinds 1, 2, 3
    double t = 0.0;
    if (prev.kind <= 0) {  // the left gene's region or its state on row i - 1
      const int l = prev.gene;
      if (sc.kind == 0) {
        if (r == l) t = J.left_trans[(size_t)i * nL + l];
      } else {
        const double lo = i == 0 ? J.enter_lo[l] : J.left_lo[(size_t)(i - 1) * nL + l];
        const double g = lo * J.gp[r];
        if (sc.kind == 1)
          t = g * J.nli[(size_t)r * 4 + sc.base];
        else if (sc.kind == 2)
          t = g * J.li[(size_t)i * nR + r];
        else
          t = (g * J.exit_li[r]) * J.prod[r];
      }
    } else if (prev.gene == r && sc.kind != 0) {  // a right gene's states lead to its own only
      if (prev.kind == 1) {
        const int a = prev.base;
        if (sc.kind == 1)
          t = J.ntt[(size_t)r * 16 + a * 4 + sc.base];
        else if (sc.kind == 2)
          t = J.nlo[((size_t)i * nR + r) * 4 + a];
        else
          t = J.exit_nlo[(size_t)r * 4 + a];
      } else {
        if (sc.kind == 2)
          t = J.rtrans[(size_t)i * nR + r];
        else if (sc.kind == 3)
          t = J.exit_trans[r];
      }
    }
    if (!(t > 0.0)) ok = false;
    lp += log(t);
    prev = sc;
  }
  return lp;
}

__global__ void __launch_bounds__(64)
    path_prior_kernel(const DevFamily fam, const DevSampler* __restrict__ smp_dev, int K, const int32_t* __restrict__ states,
                      double* __restrict__ log_prior, int32_t* __restrict__ first_bad) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const DevSampler& smp = *smp_dev;
  const int32_t* st = states + (size_t)k * smp.states_per_sample;
  const int Wvd = smp.vd.n_rows, Wdj = smp.has_d ? smp.dj.n_rows : 0;
  const int jg = st[0];
  const int vg = st[smp.states_per_sample - 1];
  bool ok = jg >= 0 && jg < smp.n_j && vg >= 0 && vg < smp.n_v;
  double lp = 0.0;
  if (ok) {
    lp = log(fam.vgerm_gene_prob[vg]) + log(fam.vpadding_transition[vg]) + log(fam.vgerm_trans_prod[vg]) +
         log(fam.jpadding_transition[jg]);
    if (smp.has_d) {
      const int dg = st[1 + Wdj];
      ok = dg >= 0 && dg < smp.n_d;
      if (ok) lp += junction_log_prior(smp.dj, dg, st + 1, jg, ok);
      if (ok) lp += junction_log_prior(smp.vd, vg, st + 2 + Wdj, dg, ok);
    } else {
      lp += junction_log_prior(smp.vd, vg, st + 1, jg, ok);
    }
    if (!(lp > -__builtin_inf())) ok = false;
  }
  log_prior[k] = ok ? lp : __builtin_nan("");
  if (!ok) atomicMin(first_bad, k);
}

}  // namespace

size_t viterbi_bp_bytes(const DevFamily& fam) {
  const size_t Wvd = fam.vd.n_rows, Wdj = fam.has_d ? fam.dj.n_rows : 0;
  size_t b = sizeof(int32_t) * (Wvd + 1 + (fam.has_d ? Wdj + 1 : 0)) + (Wvd * 5 + 1) * fam.vd.n_right +
             (fam.has_d ? (Wdj * 5 + 1) * fam.dj.n_right : 0);
  return (b + 3) & ~(size_t)3;
}

size_t viterbi_lds_bytes(const DevFamily& fam) { return viterbi_lds(fam); }

void launch_viterbi(const DevFamily& fam, const DevSampler* smp_dev, int n, const double* gem, const int32_t* gcnt,
                    const double* jem, const int32_t* jrs, const double* loglik, uint8_t* bp, int32_t* states,
                    double* log_path, bool ext, hipStream_t stream) {
  const int ga = (fam.vgerm.n_genes + 63) / 64;
  const int gb = (std::max(fam.dgerm.n_genes, fam.jgerm.n_genes) + 63) / 64;
#define LH_ARGS gb, ext, fam, smp_dev, n, gem, gcnt, jem, jrs, loglik, bp, states, log_path, stream
  if (ga <= 1)
    launch_viterbi_a<1>(LH_ARGS);
  else if (ga <= 2)
    launch_viterbi_a<2>(LH_ARGS);
  else if (ga <= 4)
    launch_viterbi_a<4>(LH_ARGS);
  else if (ga <= 8)
    launch_viterbi_a<8>(LH_ARGS);
  else
    launch_viterbi_a<16>(LH_ARGS);
#undef LH_ARGS
}

void launch_path_prior(const DevFamily& fam, const DevSampler* smp_dev, int K, const int32_t* states, double* log_prior,
                       int32_t* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(path_prior_kernel, dim3((K + 63) / 64), dim3(64), 0, stream, fam, smp_dev, K, states, log_prior,
                     first_bad);
}

}  // namespace lh
