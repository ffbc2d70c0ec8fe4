// K7: the lineage of a seed sequence, collected on the device (gfx950).
//
// A tree sample's lineage is the chain of inner nodes from the seed tip's parent up to the tree's root (naive's
// neighbour), then naive itself.  K3 leaves the sampled states of every inner node in anc[n][T-2][L]; the lineage needs
// only the P or fewer rows on that chain, and the host needs of each row only whether it has seen the sequence before.
// So the rows stay where they are and two 64-bit hashes per row come back: one of the bases, one of their translation.
//
// lineage_kernel: one wave per (sample, slot).  A lane takes 24 consecutive bases: three 8-byte words of the base hash
// and, translated codon by codon (standard code, frame 0, a codon with N = the one symbol all its resolutions give,
// else X: TranslateDna), one 8-byte word of the amino-acid hash.  The hash is K6c's (lh_device.h: XOR over the words
// of a mix of (word, position), a final mix with the length), so its bits depend on the sequence alone and a naive
// sequence hashes here as it does there.  Padding slots get kLineagePadHash; a sample whose schedule K3 refused (0xff in
// its anc rows) gets all-ones in every slot.
// With D ancestral draws per tree sample (LineageBatch::draws) the batch has n * D virtual samples: anc and the hashes lie
// at the virtual sample, path and naive at its tree sample.
// No atomics anywhere; every output element has one writer.  Path entries are checked before they index anything.
#include <algorithm>

#include "lh_device.h"

namespace lh {

namespace {

constexpr int kThreads = 256;
constexpr int kSlotsPerBlock = kThreads / 64;
constexpr int kChunk = 24;  // bases per lane and step: 3 base words, 8 codons

// amino acid of the codon (a, b, c), bases A,C,G,T,N = 0..4, at [a*25 + b*5 + c]
struct CodonTable {
  uint8_t aa[125];
};
constexpr CodonTable make_codon_table() {
  // the standard code over T, C, A, G (first base slowest)
  const char code[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
  const int tcag[4] = {2, 1, 3, 0};  // A, C, G, T -> position in TCAG
  CodonTable t{};
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 5; ++b)
      for (int c = 0; c < 5; ++c) {
        char aa = 0;
        for (int x = 0; x < 4; ++x)
          for (int y = 0; y < 4; ++y)
            for (int z = 0; z < 4; ++z) {
              if ((a < 4 && x != a) || (b < 4 && y != b) || (c < 4 && z != c)) continue;
              const char r = code[tcag[x] * 16 + tcag[y] * 4 + tcag[z]];
              aa = (aa == 0 || aa == r) ? r : 'X';
            }
        t.aa[a * 25 + b * 5 + c] = (uint8_t)aa;
      }
  return t;
}
__device__ const CodonTable kCodons = make_codon_table();

__device__ inline uint8_t translate(uint8_t a, uint8_t b, uint8_t c) {
  return (a > 4 || b > 4 || c > 4) ? (uint8_t)'X' : kCodons.aa[a * 25 + b * 5 + c];
}

__device__ inline uint64_t wave_xor(uint64_t h) {
  uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    lo ^= (uint32_t)__shfl_xor((int)lo, m, 64);
    hi ^= (uint32_t)__shfl_xor((int)hi, m, 64);
  }
  return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(kThreads)
    lineage_kernel(LineageBatch b, uint64_t* __restrict__ nt_hash, uint64_t* __restrict__ aa_hash) {
  const int lane = threadIdx.x & 63;
  const size_t x = (size_t)blockIdx.x * kSlotsPerBlock + (threadIdx.x >> 6);
  if (x >= n_slots(b)) return;
  const int i = (int)(x / (b.P + 1)), s = (int)(x % (b.P + 1));  // i: the virtual sample (tree sample, draw)
  const int L = b.L;
  const uint8_t* row = slot_row(b, i, s);
  // (K3 writes 0xff into every anc byte of a sample whose schedule it refuses; sampled states are 0..3)
  const bool refused = L > 0 && b.anc[(size_t)i * (b.T - 2) * L] == 0xff;
  if (refused || !row) {
    if (lane == 0) nt_hash[x] = aa_hash[x] = refused ? ~0ull : kLineagePadHash;
    return;
  }
  const int n_words = (L + 7) / 8, n_aa = L / 3, n_aa_words = (n_aa + 7) / 8;
  const int n_chunks = (L + kChunk - 1) / kChunk;  // covers both: 3 * n_chunks >= n_words, n_chunks >= n_aa_words
  uint64_t h_nt = 0, h_aa = 0;
  for (int c = lane; c < n_chunks; c += 64) {
    uint8_t base[kChunk];
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int j = c * kChunk + k;
      base[k] = j < L ? row[j] : (uint8_t)4;  // (K6c pads its last word with N)
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = 3 * c + k;
      uint64_t word = 0;
#pragma unroll
      for (int m = 0; m < 8; ++m) word |= (uint64_t)base[8 * k + m] << (8 * m);
      if (q < n_words) h_nt ^= hash_word(word, q);
    }
    if (c < n_aa_words) {
      uint64_t word = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint8_t aa = 8 * c + k < n_aa ? translate(base[3 * k], base[3 * k + 1], base[3 * k + 2]) : (uint8_t)0;
        word |= (uint64_t)aa << (8 * k);
      }
      h_aa ^= hash_word(word, c);
    }
  }
  h_nt = wave_xor(h_nt);
  h_aa = wave_xor(h_aa);
  if (lane == 0) {
    nt_hash[x] = hash_finish(h_nt, L) & b.hash_mask;
    aa_hash[x] = hash_finish(h_aa, n_aa) & b.hash_mask;
  }
}

unsigned slot_blocks(const LineageBatch& b) {
  return (unsigned)((n_slots(b) + kSlotsPerBlock - 1) / kSlotsPerBlock);
}

}  // namespace

void launch_lineage(const LineageBatch& b, uint64_t* nt_hash, uint64_t* aa_hash, hipStream_t stream) {
  if (b.n <= 0) return;
  hipLaunchKernelGGL(lineage_kernel, dim3(slot_blocks(b)), dim3(kThreads), 0, stream, b, nt_hash, aa_hash);
}

}  // namespace lh
