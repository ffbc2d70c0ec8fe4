// K6c: the naive sequences of K4's sampled states, on the device (gfx950).
//
// A row of K4's states (J gene | D-J rows | D gene | V-D rows | V gene; light chains J | V-J rows | V) fixes one naive
// base on every site its states cover, and N elsewhere: exactly what HMM::ApplySampledStates writes into
// RowSampler::naive_seq.  The (site, base) pairs come from tables the family already has on the device: the germline
// genes' caller-column lists of the K6 twin's segments, its junction column matrices (rows x genes, NTI x 4) and the
// caller column -> (site, naive base) map K6a keeps; K4's state classes turn a junction state into (kind, gene).
//
// assemble_kernel: one wave per row.  The row is built in LDS region by region, in ApplySampledStates' order, with a
// barrier between regions, then hashed and written out as bytes seqs[n][L] (A,C,G,T,N = 0..4).  The hash is an XOR over
// the row's 8-byte words of a 64-bit mix of (word, position): XOR is exact and order-free, so the bits do not depend
// on the lane split, the batch or the run.
// verify_kernel, append_kernel, gather_kernel: the sequence store's three (lh_device.h), written once over a row source
// and instantiated for K6c's rows (slot x = row x of seqs) and K7's (slot x = a row of anc or naive, found through the
// path).  verify: one wave per slot compares its bytes with the stored sequence the host assigned to it; append copies
// the first slot of each new id into the store; gather: the slots a host reads back.
// No atomics anywhere; every output element has one writer.
#include <algorithm>

#include "lh_device.h"

namespace lh {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / 64;

__device__ inline void put(const CollectTables& t, uint8_t* s, int col) {
  if (col < 0 || col >= t.n_cols) return;
  const int site = t.col_site[col];
  if (site >= 0 && site < t.L) s[site] = t.col_base[col];
}

// The caller columns of gene g of a germline set: eight 16-bit entries per chunk (indices or byte offsets, `scale`),
// padded with the sentinel.  Unpacked with constant indices only.
__device__ inline void put_gene(const CollectTables& t, const CollectSegments& g, int gene, int lane, uint8_t* s) {
  if (gene < 0 || gene >= g.n_genes) return;
  for (int c = lane; c < g.n_chunks; c += 64) {
    const uint4 q = g.inds[(size_t)c * g.n_genes + gene];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const uint32_t w = h < 2 ? q.x : h < 4 ? q.y : h < 6 ? q.z : q.w;
      const int v = (int)((w >> (16 * (h & 1))) & 0xffffu);
      if (v != t.seg_sentinel) put(t, s, v / t.seg_scale);
    }
  }
}

// Junction rows: row i's state k is a left-gene germline state, an NTI state or a right-gene germline state (K4's class
// word: kind | NTI base << 2 | gene << 4); the column it emits at row i is in the junction's column matrices.
__device__ inline void put_junction(const CollectTables& t, const CollectJunction& J, const int32_t* st, int lane,
                                    uint8_t* s) {
  for (int i = lane; i < J.n_rows; i += 64) {
    const int k = st[i];
    if (k < 0 || k >= J.n_states) continue;
    const int cls = J.state_class[k], kind = cls & 3, b = (cls >> 2) & 3, gene = cls >> 4;
    int j = -1;
    if (kind == 0 && gene < J.n_left) j = J.left_xmsa[(size_t)i * J.left_pad + gene];
    else if (kind == 1 && gene < J.n_right) j = J.nti_xmsa[((size_t)i * J.right_pad + gene) * 4 + b];
    else if (kind == 2 && gene < J.n_right) j = J.right_xmsa[(size_t)i * J.right_pad + gene];
    if (j >= 0 && j < t.n_jcols) put(t, s, t.jcols[j]);
  }
}

__global__ void __launch_bounds__(kThreads)
    assemble_kernel(CollectTables t, int n, const int32_t* __restrict__ states, uint8_t* __restrict__ seqs,
                    uint64_t* __restrict__ hash) {
  extern __shared__ uint8_t rows[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = blockIdx.x * kRowsPerBlock + w;
  const bool live = r < n;  // (every wave takes every barrier)
  const int Lp = (t.L + 7) & ~7;
  uint8_t* s = rows + (size_t)w * Lp;
  const int32_t* st = states + (size_t)(live ? r : 0) * t.states_per_sample;
  for (int j = lane; j < Lp; j += 64) s[j] = 4;
  __syncthreads();
  int o = 0;
  if (live) put_gene(t, t.jg, st[o], lane, s);
  ++o;
  __syncthreads();
  if (t.has_d) {
    if (live) put_junction(t, t.dj, st + o, lane, s);
    o += t.dj.n_rows;
    __syncthreads();
    if (live) put_gene(t, t.dg, st[o], lane, s);
    ++o;
    __syncthreads();
  }
  if (live) put_junction(t, t.vd, st + o, lane, s);
  o += t.vd.n_rows;
  __syncthreads();
  if (live) put_gene(t, t.vg, st[o], lane, s);
  __syncthreads();
  if (!live) return;
  uint64_t h = 0;
  for (int q = lane; q < Lp / 8; q += 64) {
    uint64_t word = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) word |= (uint64_t)s[q * 8 + b] << (8 * b);
    h ^= hash_word(word, q);
  }
  uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    lo ^= (uint32_t)__shfl_xor((int)lo, m, 64);
    hi ^= (uint32_t)__shfl_xor((int)hi, m, 64);
  }
  uint8_t* out = seqs + (size_t)r * t.L;
  for (int j = lane; j < t.L; j += 64) out[j] = s[j];
  if (lane == 0) hash[r] = hash_finish(((uint64_t)hi << 32) | lo, t.L) & t.hash_mask;
}

// The sequence store's three kernels (lh_device.h), generic over the row source.
// flag[x] = 1 where slot x's bytes differ from those of store[ids[x]], or it has no row, or the store does not hold that
// id (0 for slots with ids[x] < 0).  One wave per slot.
template <class Rows>
__global__ void __launch_bounds__(kThreads)
    verify_kernel(Rows src, int K, const int32_t* __restrict__ ids, const uint8_t* __restrict__ store,
                  uint8_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const size_t x = (size_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (x >= n_slots(src)) return;
  const int k = ids[x], L = src.L;
  const uint8_t* row = k >= 0 ? slot_row(src, (int)x) : nullptr;
  bool diff = false;
  if (row && k < K) {
    const uint8_t* st = store + (size_t)k * L;
    for (int j = lane; j < L; j += 64) diff |= row[j] != st[j];
  }
  const bool any = __any(diff);
  if (lane == 0) flag[x] = k >= 0 && (k >= K || !row || any) ? 1 : 0;
}

// store[pairs[2p]][..] = slot pairs[2p + 1]
template <class Rows>
__global__ void __launch_bounds__(kThreads)
    append_kernel(Rows src, int K, int n_pairs, const int32_t* __restrict__ pairs, uint8_t* __restrict__ store) {
  const int L = src.L;
  const size_t total = (size_t)n_pairs * L, slots = n_slots(src);
  for (size_t x = (size_t)blockIdx.x * kThreads + threadIdx.x; x < total; x += (size_t)gridDim.x * kThreads) {
    const size_t p = x / L, j = x % L;
    const int k = pairs[2 * p], y = pairs[2 * p + 1];
    if (k < 0 || k >= K || y < 0 || (size_t)y >= slots) continue;
    const uint8_t* row = slot_row(src, y);
    if (row) store[(size_t)k * L + j] = row[j];
  }
}

// out[q][..] = slot slots_in[q] (the rows a host reads back: collisions to resolve)
template <class Rows>
__global__ void __launch_bounds__(kThreads)
    gather_kernel(Rows src, int n_out, const int32_t* __restrict__ slots_in, uint8_t* __restrict__ out) {
  const int L = src.L;
  const size_t total = (size_t)n_out * L, slots = n_slots(src);
  for (size_t x = (size_t)blockIdx.x * kThreads + threadIdx.x; x < total; x += (size_t)gridDim.x * kThreads) {
    const size_t q = x / L, j = x % L;
    const int y = slots_in[q];
    const uint8_t* row = (y >= 0 && (size_t)y < slots) ? slot_row(src, y) : nullptr;
    out[x] = row ? row[j] : (uint8_t)4;
  }
}

unsigned byte_blocks(size_t total) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((total + kThreads - 1) / kThreads, 4096));
}

}  // namespace

size_t collect_lds_bytes(int L) { return (size_t)kRowsPerBlock * ((L + 7) & ~7); }

void launch_collect(const CollectTables& t, int n, const int32_t* states, uint8_t* seqs, uint64_t* hash,
                    hipStream_t stream) {
  if (n <= 0) return;
  const unsigned blocks = (unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock);
  const size_t lds = collect_lds_bytes(t.L);
  launch_lds(assemble_kernel, dim3(blocks), dim3(kThreads), lds, stream, t, n, states, seqs, hash);
}

template <class Rows>
void launch_store_verify(const Rows& src, int K, const int32_t* ids, const uint8_t* store, uint8_t* flag,
                         hipStream_t stream) {
  const size_t slots = n_slots(src);
  if (slots == 0) return;
  hipLaunchKernelGGL(verify_kernel<Rows>, dim3((unsigned)((slots + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(kThreads), 0,
                     stream, src, K, ids, store, flag);
}

template <class Rows>
void launch_store_append(const Rows& src, int K, int n_pairs, const int32_t* pairs, uint8_t* store, hipStream_t stream) {
  if (n_pairs <= 0 || n_slots(src) == 0) return;
  hipLaunchKernelGGL(append_kernel<Rows>, dim3(byte_blocks((size_t)n_pairs * src.L)), dim3(kThreads), 0, stream, src, K,
                     n_pairs, pairs, store);
}

template <class Rows>
void launch_store_gather(const Rows& src, int n_out, const int32_t* slots, uint8_t* out, hipStream_t stream) {
  if (n_out <= 0 || n_slots(src) == 0) return;
  hipLaunchKernelGGL(gather_kernel<Rows>, dim3(byte_blocks((size_t)n_out * src.L)), dim3(kThreads), 0, stream, src, n_out,
                     slots, out);
}

#define LH_STORE_KERNELS(Rows)                                                                                          \
  template void launch_store_verify<Rows>(const Rows&, int, const int32_t*, const uint8_t*, uint8_t*, hipStream_t);     \
  template void launch_store_append<Rows>(const Rows&, int, int, const int32_t*, uint8_t*, hipStream_t);                \
  template void launch_store_gather<Rows>(const Rows&, int, const int32_t*, uint8_t*, hipStream_t);
LH_STORE_KERNELS(FlatRows)
LH_STORE_KERNELS(LineageBatch)
#undef LH_STORE_KERNELS

}  // namespace lh
