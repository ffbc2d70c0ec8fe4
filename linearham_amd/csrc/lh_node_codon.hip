// K14: exact codon marginals of a node of a seed's lineage, and how the node's codon differs from the naive one (gfx950).
//
// Given the naive base of a site, the node's base at that site is independent of everything else (K13, lh_ancestral_probs.hip):
// G_t[j][b][x] = P(x_{v,j} = x | column j, naive_j = b) is K13b's table.  The three sites of a codon are coupled only
// through the naive codon, whose 125-entry posterior Q_t[c] K9 gives (lh_codon.hip), so for codon c over sites j1, j2, j3
//   T_t[c][x1 x2 x3] = sum over b in {A,C,G,T,N}^3 of Q_t[c][b1 b2 b3] G_t[j1][b1][x1] G_t[j2][b2][x2] G_t[j3][b3][x3].
// change[c][0..3] folds the joint P(b, x) = Q[b] prod G by the relation of x to b: identical, another codon with the same
// translation, a different translation, and (entry 3) the naive triple holds an N -- the mass Q puts there, whatever x.
//
// Kernels:
//  * naive_codon_kernel, a wave per (row, codon): Q[n][C][125].  A window codon is K9's; a codon inside a germline region
//    is the region's gene posterior pushed onto the triples its genes write there (NodeCodonTables: the triple of every gene
//    of the region at that codon).  The wave loads 64 genes at a time, a lane each, and hands them round in ascending gene
//    order (readlane at a uniform index); lane e owns the entries e and e + 64 and adds a gene's posterior where the gene's
//    triple is its entry, 0.0 otherwise.  Adding 0.0 changes no bits, so every entry is the sum of its genes in ascending
//    gene order, the order of the host's expansion (posterior.codon_table, PhyloHMM::ExpandCodons): no atomics, one fixed
//    summation order, any number of genes in a region.
//  * node_codon_kernel, a wave per (row, codon), lane = node triple x = 16 x1 + 4 x2 + x3.  A lane holds its 15 entries of G
//    (three 5-vectors); Q is read at wave-uniform addresses and a zero entry is skipped by a uniform branch (a germline
//    codon has a handful of non-zero triples).  T accumulates in the factored order b1, b2, b3; the three classes are the
//    lanes' partial sums of the 64 N-free terms, reduced over the wave by a fixed butterfly.  The class of (b, x) comes from
//    a compile-time relation (kSameAa), the standard code with the stop codons as a symbol of their own.
// No private array is reached by a dynamic index: the 5-vectors are indexed by unrolled loops only.  A row without a path
// (plen 0) or with a non-finite log-likelihood gets NaN.
#include "lh_device.h"

namespace lh {

namespace {

// same[x] bit b: the N-free triples b = 16 b1 + 4 b2 + b3 and x have the same translation (b = x included)
struct SameAa {
  uint64_t same[64];
};
constexpr SameAa make_same_aa() {
  // the standard code over T, C, A, G (first base slowest)
  const char code[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
  const int tcag[4] = {2, 1, 3, 0};  // A, C, G, T -> position in TCAG
  char aa[64] = {};
  for (int x = 0; x < 64; ++x) aa[x] = code[tcag[x >> 4] * 16 + tcag[(x >> 2) & 3] * 4 + tcag[x & 3]];
  SameAa t{};
  for (int x = 0; x < 64; ++x)
    for (int b = 0; b < 64; ++b)
      if (aa[b] == aa[x]) t.same[x] |= (uint64_t)1 << b;
  return t;
}
constexpr SameAa kSameAaHost = make_same_aa();
__device__ const SameAa kSameAa = make_same_aa();

__global__ void __launch_bounds__(256) naive_codon_kernel(NodeCodonTables t, int n, const double* __restrict__ windows,
                                                          const double* __restrict__ genes, double* __restrict__ Q) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)n * t.n_codons) return;
  const int row = (int)(item / t.n_codons), c = (int)(item - (long long)row * t.n_codons);
  double* __restrict__ q = Q + (size_t)item * 125;
  const int src = t.codon_src[c];
  if (src >= 0) {
    const double* __restrict__ w = windows + ((size_t)row * t.n_window + src) * 125;
    q[lane] = w[lane];
    if (lane + 64 < 125) q[lane + 64] = w[lane + 64];
    return;
  }
  const int4 info = t.germ[-1 - src];  // the codes' offset, the region's first gene and its gene count
  const uint8_t* __restrict__ code = t.codes + info.x;
  const double* __restrict__ g = genes + (size_t)row * t.n_genes + info.y;
  double lo = 0.0, hi = 0.0;  // entries lane and lane + 64
  for (int g0 = 0; g0 < info.z; g0 += 64) {
    const int m = min(64, info.z - g0);
    const double gv = lane < m ? g[g0 + lane] : 0.0;
    const int gc = lane < m ? code[g0 + lane] : 255;
    for (int j = 0; j < m; ++j) {
      const double v = read_lane(gv, j);
      const int e = __builtin_amdgcn_readlane(gc, j);
      lo += e == lane ? v : 0.0;
      hi += e == lane + 64 ? v : 0.0;
    }
  }
  q[lane] = lo;
  if (lane + 64 < 125) q[lane + 64] = hi;
}

__global__ void __launch_bounds__(256) node_codon_kernel(int n, int C, int frame, int n_prune,
                                                         const int32_t* __restrict__ site_pat,
                                                         const double* __restrict__ table, const double* __restrict__ Q,
                                                         const int32_t* __restrict__ plen, const double* __restrict__ loglik,
                                                         double* __restrict__ codons, double* __restrict__ change) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)n * C) return;
  const int row = (int)(item / C), c = (int)(item - (long long)row * C);
  double* __restrict__ out = codons ? codons + (size_t)item * 64 : nullptr;
  double* __restrict__ cls = change ? change + (size_t)item * 4 : nullptr;
  if (plen[row] == 0 || (loglik && !isfinite(loglik[row]))) {
    if (out) out[lane] = __builtin_nan("");
    if (cls && lane < 4) cls[lane] = __builtin_nan("");
    return;
  }
  // the lane's entries of G: g[k][b] = G[site k of the codon][b][x_k]
  double g[3][5];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int pat = min(site_pat[frame + 3 * c + k], n_prune);
    const int xk = (lane >> (4 - 2 * k)) & 3;
    const double* __restrict__ t5 = table + ((size_t)row * (n_prune + 1) + pat) * 20 + xk;
#pragma unroll
    for (int b = 0; b < 5; ++b) g[k][b] = t5[4 * b];
  }
  const double* __restrict__ q = Q + (size_t)item * 125;  // wave-uniform
  if (out) {
    double t = 0.0;
#pragma unroll
    for (int b1 = 0; b1 < 5; ++b1) {
      double s1 = 0.0;
#pragma unroll
      for (int b2 = 0; b2 < 5; ++b2) {
        double s2 = 0.0;
#pragma unroll
        for (int b3 = 0; b3 < 5; ++b3) {
          const double qv = q[25 * b1 + 5 * b2 + b3];
          if (qv != 0.0) s2 += qv * g[2][b3];
        }
        s1 += g[1][b2] * s2;
      }
      t += g[0][b1] * s1;
    }
    out[lane] = t;
  }
  if (cls) {
    const uint64_t same = kSameAa.same[lane];
    double ident = 0.0, syn = 0.0, repl = 0.0, open = 0.0;
#pragma unroll
    for (int b1 = 0; b1 < 5; ++b1)
#pragma unroll
      for (int b2 = 0; b2 < 5; ++b2)
#pragma unroll
        for (int b3 = 0; b3 < 5; ++b3) {
          const double qv = q[25 * b1 + 5 * b2 + b3];
          if (b1 == 4 || b2 == 4 || b3 == 4) {
            open += qv;  // (uniform: every lane forms the same sum in the same order)
          } else if (qv != 0.0) {
            const int b = 16 * b1 + 4 * b2 + b3;
            const double term = qv * ((g[0][b1] * g[1][b2]) * g[2][b3]);
            const bool is_same = (same >> b) & 1;
            ident += lane == b ? term : 0.0;
            syn += (is_same && lane != b) ? term : 0.0;
            repl += is_same ? 0.0 : term;
          }
        }
    ident = wave_sum(ident);
    syn = wave_sum(syn);
    repl = wave_sum(repl);
    if (lane == 0) {
      double2* o = reinterpret_cast<double2*>(cls);
      o[0] = make_double2(ident, syn);
      o[1] = make_double2(repl, open);
    }
  }
}

}  // namespace

void node_codon_classes(uint8_t* out) {
  for (int i = 0; i < 125; ++i) {
    const int b1 = i / 25, b2 = (i / 5) % 5, b3 = i % 5;
    for (int x = 0; x < 64; ++x) {
      uint8_t k = 3;
      if (b1 < 4 && b2 < 4 && b3 < 4) {
        const int b = 16 * b1 + 4 * b2 + b3;
        k = b == x ? 0 : ((kSameAaHost.same[x] >> b) & 1) ? 1 : 2;
      }
      out[i * 64 + x] = k;
    }
  }
}

void launch_naive_codons(const NodeCodonTables& t, int n, const double* windows, const double* genes, double* Q,
                         hipStream_t stream) {
  const long long items = (long long)n * t.n_codons;
  if (items <= 0) return;
  hipLaunchKernelGGL(naive_codon_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, t, n, windows, genes, Q);
}

void launch_node_codons(const DevFamily& fam, int n, int n_codons, int frame, const double* table, const double* Q,
                        const int32_t* plen, const double* loglik, double* codons, double* change, hipStream_t stream) {
  const long long items = (long long)n * n_codons;
  if (items <= 0 || (!codons && !change)) return;
  hipLaunchKernelGGL(node_codon_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, n, n_codons, frame,
                     fam.n_prune, fam.site_pat, table, Q, plen, loglik, codons, change);
}

}  // namespace lh
