// The duplicate removal of libgfdedup.so (include/gf_dedup.h) over records in HBM:
//
//   keys       K of every record                                        gf_dd_k_keys (a block per tile of 256 records,
//                                                                         G lanes per record)
//   insert     every key found or placed in the table, the lowest       gf_dd_k_insert (a thread per record)
//              index and the count of its slot
//   remove     decide: which records are duplicates, the survivors'     gf_dd_k_decide (a block per tile, a thread per
//              lengths scanned inside the tile                            record)
//              offsets and gather                                         gf_pp_k_scan, gf_pp_k_gather (gf_pp_kernels.h,
//                                                                         as they are)
//   rehash     the old table's entries placed in the new one             gf_dd_k_fill, gf_dd_k_rehash (a thread per slot)
//   histogram  the keys by how often they were offered                   gf_dd_k_histogram (a thread per slot)
//
// Keys: a group of G = 16 lanes takes a record, as in gf_pp_k_decide and for its reason: a read of 150 bases is 10
// pieces of 16 bytes (gf_dd_core.h says what a chunk, a piece and a round are), so four records fill a wavefront to two
// thirds.  A lane loads its piece's chunk and the one behind it — its neighbour's, from the cache — in aligned 16-byte
// loads, funnel-shifts its two record-relative words out of them, masks the bytes at or past L, mixes, and the group
// adds up with __shfl_xor: the sum does not depend on the order.
//
// Insert: linear probing from the key's home slot.  A slot is read first; only an empty one is claimed, with a 64-bit
// atomicCAS, and a slot that another key won is passed.  Then one atomicMin on first[] and, with count[], one
// atomicAdd: three scattered 64- and 32-bit atomics a record at the most.  A probe gives up after `slots` entries.
// Deterministic: which slot a key ends in depends on the order of arrival, the set of (key, first, count) does not —
// every min and every sum is an integer.
#pragma once

#include "gf_dd_core.h"
#include "gf_pp_kernels.h"

// chunk c (>= 0) behind the 16-byte aligned address p
__device__ __forceinline__ gf_dd_chunk gf_dd_load(const uint8_t* p, int64_t c) {
  const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * c);
  return gf_dd_chunk{{(uint64_t)v.x | (uint64_t)v.y << 32, (uint64_t)v.z | (uint64_t)v.w << 32}};
}

// H of record i of one side by the G lanes of a group, in every lane of the group; L: its length
template <int G>
__device__ __forceinline__ uint64_t gf_dd_hash_group(const uint8_t* __restrict__ bases,
                                                     const int64_t* __restrict__ off, int64_t i, int64_t& L) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t start = off[i];
  L = gf_dd_length(start, off[i + 1]);
  uint64_t sum = 0;
  if (L > 0) {
    const uintptr_t p = (uintptr_t)(bases + start);
    const int a = (int)(p & 15);
    const uint8_t* base = (const uint8_t*)(p - a);
    for (int64_t k = gl; 16 * k < L; k += G) {
      const gf_dd_chunk c0 = gf_dd_load(base, k);
      const gf_dd_chunk c1 = gf_dd_needs_next(a, L, k) ? gf_dd_load(base, k + 1) : gf_dd_chunk{{0, 0}};
      sum += gf_dd_piece_sum(c0, c1, a, L, k);
    }
  }
#pragma unroll
  for (int o = 1; o < G; o <<= 1) sum += __shfl_xor((unsigned long long)sum, o);
  return gf_dd_finish(L, sum);
}

// ---- keys: block b takes the records GF_PP_TILE b .., a group of G lanes a record at a time, both mates
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_keys(const uint8_t* __restrict__ l_bases,
                                                                const int64_t* __restrict__ l_off,
                                                                const uint8_t* __restrict__ r_bases,
                                                                const int64_t* __restrict__ r_off, int64_t n,
                                                                unsigned long long* __restrict__ rec_keys) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    int64_t L1 = 0, L2 = 0;
    const uint64_t h1 = gf_dd_hash_group<G>(l_bases, l_off, i, L1);
    uint64_t key;
    if (r_off) {
      const uint64_t h2 = gf_dd_hash_group<G>(r_bases, r_off, i, L2);
      key = gf_dd_key_pair(L1, h1, L2, h2);
    } else {
      key = gf_dd_key_single(L1, h1);
    }
    if (gl == 0) rec_keys[i] = key;
  }
}

// a wavefront's count of `flag` added to *total by its first lane
__device__ __forceinline__ void gf_dd_wave_add(bool flag, unsigned long long* total) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(total, (unsigned long long)__popcll(m));
}

// a key found or placed in the table: its slot, -1 when `slots` entries were visited without success
__device__ __forceinline__ int64_t gf_dd_place(unsigned long long* __restrict__ keys, int64_t slots,
                                               unsigned long long key, bool& is_new) {
  is_new = false;
  int64_t s = gf_dd_home(key, slots);
  for (int64_t t = 0; t < slots; ++t, s = gf_dd_next(s, slots)) {
    unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      cur = atomicCAS(&keys[s], 0ull, key);
      if (cur == 0) {
        is_new = true;
        return s;
      }
    }
    if (cur == key) return s;
  }
  return -1;
}

// ---- insert: a thread a record
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_insert(const unsigned long long* __restrict__ rec_keys,
                                                                  int64_t n, int64_t first_index,
                                                                  unsigned long long* __restrict__ keys,
                                                                  long long* __restrict__ first,
                                                                  unsigned int* __restrict__ count, int64_t slots,
                                                                  int64_t* __restrict__ rec_slot,
                                                                  unsigned long long* __restrict__ totals) {
  const int64_t i = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x;
  const unsigned long long key = i < n ? rec_keys[i] : 0ull;
  bool is_new = false;
  int64_t s = -1;
  if (key) {
    s = gf_dd_place(keys, slots, key, is_new);
    if (s >= 0) {
      atomicMin(&first[s], (long long)(first_index + i));
      if (count) atomicAdd(&count[s], 1u);
    }
  }
  if (i < n) rec_slot[i] = s;
  gf_dd_wave_add(i < n, &totals[0]);
  gf_dd_wave_add(key != 0, &totals[1]);
  gf_dd_wave_add(is_new, &totals[2]);
  gf_dd_wave_add(key != 0 && s < 0, &totals[5]);
}

// ---- decide: block b takes the records GF_PP_TILE b .., a thread a record.  Leaves what gf_pp_k_decide leaves: the
// survivors' lengths as offsets inside the tile (out.off[i], made absolute by gf_pp_k_gather) and the tile's kept bytes
// per side, so that the other two stages are the read filter's.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_decide(GfPpSide L, GfPpSide R, int sides, int64_t n,
                                                                  int64_t first_index,
                                                                  const int64_t* __restrict__ rec_slot,
                                                                  const long long* __restrict__ first, GfPpOut out_l,
                                                                  GfPpOut out_r, int64_t* __restrict__ tile_sum_l,
                                                                  int64_t* __restrict__ tile_sum_r,
                                                                  uint8_t* __restrict__ dup,
                                                                  unsigned long long* __restrict__ totals) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  __shared__ unsigned long long s_removed;
  const int64_t i = (int64_t)blockIdx.x * GF_PP_TILE + threadIdx.x;
  if (threadIdx.x == 0) s_removed = 0;
  bool is_dup = false;
  long long len_l = 0, len_r = 0;
  if (i < n) {
    const int64_t s = rec_slot[i];
    is_dup = s >= 0 && first[s] != (long long)(first_index + i);
    len_l = gf_dd_length(L.off[i], L.off[i + 1]);
    if (sides == 2) len_r = gf_dd_length(R.off[i], R.off[i + 1]);
    dup[i] = is_dup ? 1 : 0;
  }
  __syncthreads();  // (s_removed)
  if (is_dup && len_l + len_r) atomicAdd(&s_removed, (unsigned long long)(len_l + len_r));
  int ea, ta;
  long long el, tl, er, tr;
  gf_scan_block_scan2(0, is_dup ? 0 : len_l, s_a, s_b, ea, el, ta, tl);
  gf_scan_block_scan2(0, is_dup ? 0 : len_r, s_a, s_b, ea, er, ta, tr);
  if (i < n) {
    out_l.off[i] = el;
    if (sides == 2) out_r.off[i] = er;
  }
  gf_dd_wave_add(is_dup, &totals[3]);
  if (threadIdx.x == 0) {
    tile_sum_l[blockIdx.x] = tl;
    if (sides == 2) tile_sum_r[blockIdx.x] = tr;
    if (s_removed) atomicAdd(&totals[4], s_removed);  // (behind the scans' barriers: every lane has added)
  }
}

// ---- rehash: the new table emptied, then a thread an old slot
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_fill(unsigned long long* __restrict__ keys,
                                                                long long* __restrict__ first,
                                                                unsigned int* __restrict__ count, int64_t slots) {
  const int64_t s = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x;
  if (s >= slots) return;
  keys[s] = 0;
  first[s] = GF_DD_NO_INDEX;
  if (count) count[s] = 0;
}

__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_rehash(const unsigned long long* __restrict__ old_keys,
                                                                  const long long* __restrict__ old_first,
                                                                  const unsigned int* __restrict__ old_count,
                                                                  int64_t old_slots,
                                                                  unsigned long long* __restrict__ keys,
                                                                  long long* __restrict__ first,
                                                                  unsigned int* __restrict__ count, int64_t slots) {
  const int64_t o = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x;
  if (o >= old_slots) return;
  const unsigned long long key = old_keys[o];
  if (!key) return;
  bool is_new;
  const int64_t s = gf_dd_place(keys, slots, key, is_new);  // (a larger table has room for every key of the old one)
  if (s < 0) return;
  atomicMin(&first[s], old_first[o]);
  if (count && old_count) atomicAdd(&count[s], old_count[o]);
}

// ---- histogram: a thread a slot, the block's levels summed in LDS
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_dd_k_histogram(const unsigned long long* __restrict__ keys,
                                                                     const unsigned int* __restrict__ count,
                                                                     int64_t slots,
                                                                     unsigned long long* __restrict__ hist) {
  __shared__ unsigned int s_hist[GF_DD_LEVELS];
  if (threadIdx.x < GF_DD_LEVELS) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x;
  if (s < slots && keys[s]) {
    const int level = gf_dd_level(count[s]);
    if (level > 0) atomicAdd(&s_hist[level], 1u);
  }
  __syncthreads();
  if (threadIdx.x < GF_DD_LEVELS && s_hist[threadIdx.x])
    atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}
