// The kernels of libgfalign.so (include/gf_alignable.h): the seeds of the candidate reads, the entry table of the sorted
// seeds, and the scan of one piece of reference text.  The arithmetic is gf_al_core.h, the text the host tests run.
//
// gf_al_k_seeds: a workgroup per read writes the read's two strand strings next to each other, then a seed per valid
// 16-mer into the slot of its first base (a slot without a seed keeps GF_AL_NO_SEED) and the key's bit into the filter.
// gf_al_k_index: a thread per slot of the sorted seeds; the first seed of a bucket writes the bucket's start.
//
// gf_al_k_scan, the hot path: a thread takes GF_AL_SCAN_SPAN consecutive text positions, 16 bytes of text a lane and
// the lanes of a wavefront back to back (two 16-byte loads a lane, the second the next lane's first).  It rolls the
// 2-bit key over its 31 bytes in registers, asks the filter for all its valid windows at once (up to 16 independent
// loads in flight a lane), and only for the bits that come back set leaves the streaming loop: the key is formed again
// from the text, its bucket of the sorted seeds is entered, the key's equal range is found by bisection and walked, and
// per seed the diagonal is tested — unless the read is flagged already, or the seed does not open an exact run on that
// diagonal.  The only write is an atomic OR of the read's bit.
//
// Every loop is bounded by the piece's length, a bucket's length (bisection: its logarithm), an equal range's length or
// a read's length.  No spin wait, no queue, no scratch, no communication between workgroups; every offset is checked
// against its array before anything is read through it.
#pragma once

#include <hip/hip_runtime.h>

#include "gf_al_core.h"

#define GF_AL_THREADS 256
#define GF_AL_MAX_BLOCKS 2048
#define GF_AL_SCAN_SPAN 16                                     // text positions a thread: one 16-byte load
#define GF_AL_SCAN_TILE ((int64_t)GF_AL_THREADS * GF_AL_SCAN_SPAN)   // text positions a workgroup and round

// the read r inside bases[0, bases_bytes): false when its offsets point outside or it is too long
__device__ __forceinline__ bool gf_al_read_of(const int64_t* __restrict__ offsets, int64_t r, int64_t bases_bytes, int64_t& start,
                                              int64_t& len) {
  start = offsets[r];
  const int64_t end = offsets[r + 1];
  len = end - start;
  return start >= 0 && end >= start && end <= bases_bytes && len <= GF_AL_MAX_LEN;
}

__global__ __launch_bounds__(GF_AL_THREADS) void gf_al_k_fill(int64_t* __restrict__ seeds, int64_t n_slots) {
  for (int64_t i = (int64_t)blockIdx.x * GF_AL_THREADS + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * GF_AL_THREADS)
    seeds[i] = GF_AL_NO_SEED;
}

// strands: uint8[2 * bases_bytes]; seeds: int64[2 * bases_bytes], GF_AL_NO_SEED everywhere; filter: zeroed
__global__ __launch_bounds__(GF_AL_THREADS) void gf_al_k_seeds(const uint8_t* __restrict__ bases, int64_t bases_bytes,
                                                                const int64_t* __restrict__ offsets, int64_t n_reads,
                                                                uint8_t* __restrict__ strands, int64_t* __restrict__ seeds,
                                                                uint32_t* __restrict__ filter, int32_t log2_bits) {
  for (int64_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
    int64_t start, len;
    const bool ok = gf_al_read_of(offsets, r, bases_bytes, start, len);   // (the same in every thread of the workgroup)
    if (ok) {
      uint8_t* fwd = strands + gf_al_string_start(start, len, 0);
      uint8_t* rev = strands + gf_al_string_start(start, len, 1);
      for (int64_t i = threadIdx.x; i < len; i += GF_AL_THREADS) {
        fwd[i] = bases[start + i];
        rev[i] = gf_al_complement(bases[start + len - 1 - i]);
      }
    }
    __syncthreads();   // (the strings are written: the windows below read them)
    if (ok && len >= GF_AL_K) {
      const int64_t windows = len - GF_AL_K + 1;
      for (int64_t w = threadIdx.x; w < 2 * windows; w += GF_AL_THREADS) {
        const int64_t t = w >= windows, j = w - t * windows;
        const int64_t at = gf_al_string_start(start, len, t);
        uint32_t key;
        if (gf_al_window_key(strands + at, j, key)) {
          seeds[at + j] = gf_al_seed(key, (uint32_t)(2 * r + t), (uint32_t)j);
          const uint32_t bit = gf_al_filter_bit(key, log2_bits);
          atomicOr(filter + (bit >> 5), 1u << (bit & 31u));
        }
      }
    }
  }
}

// bucket_start: int32[2^GF_AL_BUCKET_BITS + 1]; the seeds sorted, the slots without a seed behind them
__global__ __launch_bounds__(GF_AL_THREADS) void gf_al_k_index(const int64_t* __restrict__ seeds, int64_t n_slots,
                                                                int32_t* __restrict__ bucket_start) {
  const int32_t n_buckets = 1 << GF_AL_BUCKET_BITS;
  for (int64_t i = (int64_t)blockIdx.x * GF_AL_THREADS + threadIdx.x; i <= n_slots; i += (int64_t)gridDim.x * GF_AL_THREADS) {
    const bool seed = i < n_slots && seeds[i] != GF_AL_NO_SEED;
    const bool prev_seed = i > 0 && seeds[i - 1] != GF_AL_NO_SEED;
    if (!seed && i > 0 && !prev_seed) continue;   // behind the first slot without a seed: nothing starts here
    // the buckets that start at i: those behind the previous seed's up to this seed's, or up to the end
    const int32_t from = prev_seed ? (int32_t)gf_al_bucket(gf_al_seed_key(seeds[i - 1])) + 1 : 0;
    const int32_t to = seed ? (int32_t)gf_al_bucket(gf_al_seed_key(seeds[i])) : n_buckets;
    for (int32_t b = from; b <= to; b++) bucket_start[b] = (int32_t)i;
  }
}

// A set filter bit at text position g: the key's equal range of the sorted seeds, a diagonal per seed.
__device__ __noinline__ void gf_al_probe(const uint8_t* __restrict__ text, int64_t text_bytes, int64_t g,
                                         const uint8_t* __restrict__ strands, int64_t bases_bytes,
                                         const int64_t* __restrict__ offsets, int64_t n_reads,
                                         const int64_t* __restrict__ seeds, int64_t n_slots,
                                         const int32_t* __restrict__ bucket_start, uint32_t* __restrict__ flags) {
  uint32_t key = 0;
  for (int32_t i = 0; i < GF_AL_K; i++) key = (key << 2) | (gf_al_code(gf_al_upper(text[g + i])) & 3u);
  const uint32_t b = gf_al_bucket(key);
  int64_t lo = bucket_start[b], hi = bucket_start[b + 1];
  lo = lo < 0 ? 0 : lo > n_slots ? n_slots : lo;
  hi = hi < lo ? lo : hi > n_slots ? n_slots : hi;
  const int64_t first = gf_al_seed(key, 0, 0);
  int64_t end = hi;
  while (lo < end) {   // the first seed of the bucket that is not below the key
    const int64_t mid = lo + ((end - lo) >> 1);
    if (seeds[mid] < first) lo = mid + 1;
    else end = mid;
  }
  for (int64_t i = lo; i < hi; i++) {
    const int64_t seed = seeds[i];
    if (seed == GF_AL_NO_SEED || gf_al_seed_key(seed) != key) break;
    const int64_t s = gf_al_seed_string(seed), j = gf_al_seed_offset(seed), r = s >> 1;
    if (r >= n_reads) continue;
    const uint32_t bit = 1u << (r & 31);
    if (flags[r >> 5] & bit) continue;   // (flagged already: nothing can change for this read)
    int64_t start, len;
    if (!gf_al_read_of(offsets, r, bases_bytes, start, len) || j > len - GF_AL_K) continue;
    const uint8_t* str = strands + gf_al_string_start(start, len, s);
    if (!gf_al_opens_run(str, j, text, g)) continue;   // (the seed before this one on the diagonal tests it)
    if (gf_al_diagonal(str, len, text, text_bytes, g - j)) atomicOr(flags + (r >> 5), bit);
  }
}

// text: 16-byte aligned; flags: uint32[ceil(n_reads / 32)]
__global__ __launch_bounds__(GF_AL_THREADS) void gf_al_k_scan(const uint8_t* __restrict__ text, int64_t text_bytes,
                                                               const uint8_t* __restrict__ strands, int64_t bases_bytes,
                                                               const int64_t* __restrict__ offsets, int64_t n_reads,
                                                               const int64_t* __restrict__ seeds, int64_t n_slots,
                                                               const int32_t* __restrict__ bucket_start,
                                                               const uint32_t* __restrict__ filter, int32_t log2_bits,
                                                               uint32_t* __restrict__ flags) {
  for (int64_t tile = (int64_t)blockIdx.x * GF_AL_SCAN_TILE; tile < text_bytes; tile += (int64_t)gridDim.x * GF_AL_SCAN_TILE) {
    const int64_t g0 = tile + (int64_t)threadIdx.x * GF_AL_SCAN_SPAN;
    if (g0 + GF_AL_K > text_bytes) continue;   // (no whole window starts here)
    // the 31 bytes of this thread's 16 windows; past the end of the text: separators
    uint32_t w[8];
    if (g0 + 32 <= text_bytes) {
      const uint4 a = *reinterpret_cast<const uint4*>(text + g0), c = *reinterpret_cast<const uint4*>(text + g0 + 16);
      w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = c.x, w[5] = c.y, w[6] = c.z, w[7] = c.w;
    } else {
#pragma unroll
      for (int32_t q = 0; q < 8; q++) {
        uint32_t v = 0;
#pragma unroll
        for (int32_t k = 0; k < 4; k++) {
          const int64_t at = g0 + 4 * q + k;
          if (at < text_bytes) v |= (uint32_t)text[at] << (8 * k);
        }
        w[q] = v;
      }
    }
    uint32_t key = 0, bits[GF_AL_SCAN_SPAN];
    int32_t valid = 0;      // the bases of ACGT that end at this byte
    uint32_t ask = 0;       // the windows that have a key
#pragma unroll
    for (int32_t k = 0; k < GF_AL_SCAN_SPAN + GF_AL_K - 1; k++) {
      const uint32_t c = gf_al_code(gf_al_upper((uint8_t)(w[k >> 2] >> (8 * (k & 3)))));
      key = (key << 2) | (c & 3u);
      valid = c < 4u ? valid + 1 : 0;
      if (k >= GF_AL_K - 1) {
        bits[k - (GF_AL_K - 1)] = gf_al_filter_bit(key, log2_bits);
        if (valid >= GF_AL_K) ask |= 1u << (k - (GF_AL_K - 1));
      }
    }
    uint32_t hits = 0;
#pragma unroll
    for (int32_t q = 0; q < GF_AL_SCAN_SPAN; q++)
      if ((ask >> q) & 1u) hits |= ((filter[bits[q] >> 5] >> (bits[q] & 31u)) & 1u) << q;
    while (hits) {
      const int32_t q = __ffs(hits) - 1;
      hits &= hits - 1;
      gf_al_probe(text, text_bytes, g0 + q, strands, bases_bytes, offsets, n_reads, seeds, n_slots, bucket_start, flags);
    }
  }
}
