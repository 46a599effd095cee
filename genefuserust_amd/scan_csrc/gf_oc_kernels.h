// The overlap correction of libgfcorrect.so (include/gf_overlap_correct.h) over records in HBM, one kernel:
//
//   correct   I* of every pair and the correction at it, in place; I*, the      gf_oc_k_correct (a block per tile of 256
//             corrected bases per read; the totals, one atomic per counter        pairs, G lanes per pair)
//             and block
//
// The shape is gf_at_k_decide's (gf_at_kernels.h, whose group helpers are used as they are): a group of G = 16 lanes
// takes a pair, loads both mates' bases once in aligned 16-byte chunks, a chunk a lane, packs them into the group's
// planes in LDS — a forwards, b as its reverse complement — and searches I* in rounds of G inserts from the largest
// downwards.  Behind the group's max every lane knows I*.  Then a lane takes a word of [lo, hi), 32 positions: it
// computes the differences from the planes in LDS again (gf_oc_diff_word, the expression the search counted), never
// from global memory, and for each set bit — there are at most max_diff in the pair — reads the four bytes with byte
// loads, decides (gf_oc_decide) and writes two bytes with byte stores.
//
// Two things the stores depend on:
//   bytes, not words    a record's neighbours in the buffer are other pairs' records, corrected by other groups at the
//                       same time; a wider read-modify-write around a byte would write a neighbour's bytes back as they
//                       were.  The chunk loads of the packing do read up to 15 bytes of a neighbour, while it may be
//                       written, but those bytes are masked out of the planes (gf_at_pack_chunk) and so never looked at.
//   behind the sync     the planes are packed from the very bytes that are rewritten.  Every lane of the group has
//                       finished its chunk loads behind the group sync that ends the packing, and that sync lies in
//                       front of the search, so in front of every store of the group.
//
// A read of 512 bases is 16 words: one word a lane at the most, and the per-lane counts (at most 512 in all) are summed
// over the group as three 10-bit fields of one register.
//
// Deterministic: the LDS atomics are ORs of disjoint bits, every byte belongs to one (i, j), the totals are integer sums.
#pragma once

#include "gf_at_kernels.h"
#include "gf_oc_core.h"

struct GfOcSide {
  uint8_t* bases;
  uint8_t* quals;
  const int64_t* off;
};

template <int G>
__device__ __forceinline__ uint32_t gf_oc_group_sum(uint32_t v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// One pair by the G lanes of a group, in place.  Returns I* (-1 without one) and the pair's counts, in every lane of the
// group.  s_a / s_r: the group's planes.
template <int G>
__device__ __forceinline__ int32_t gf_oc_correct_group(const GfOcSide& Ls, const GfOcSide& Rs, int64_t i,
                                                       const gf_oc_settings& s, const gf_at_settings& t, uint32_t* s_a,
                                                       uint32_t* s_r, gf_oc_counts& c) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t start_l = Ls.off[i], len_l = Ls.off[i + 1] - start_l;
  const int64_t start_r = Rs.off[i], len_r = Rs.off[i + 1] - start_r;
  c.fixed[0] = c.fixed[1] = c.left = 0;
  if (gf_at_passes(len_l) || gf_at_passes(len_r)) return -1;
  const int32_t L1 = (int32_t)len_l, L2 = (int32_t)len_r;
  gf_at_group_sync();  // (the pair before this one has been read to its end)
  gf_at_zero_group<G>(s_a);
  gf_at_zero_group<G>(s_r);
  gf_at_group_sync();
  gf_at_pack_group<G>(Ls.bases + start_l, L1, false, s_a);
  gf_at_pack_group<G>(Rs.bases + start_r, L2, true, s_r);
  gf_at_group_sync();  // (every chunk of the pair is loaded and packed: from here on its bytes may be written)
  const int32_t first = gf_at_first_insert(t);
  int32_t insert = -1;
  for (int32_t top = gf_at_last_insert(L1, L2, t); top >= first; top -= G) {
    const int32_t I = top - gl;
    const bool ok = I >= first && gf_at_try_insert(s_a, s_r, L1, L2, I, t);
    insert = gf_at_group_max<G>(ok ? I : -1);
    if (insert >= 0) break;
  }
  if (insert < 0) return -1;
  const int32_t lo = insert > L2 ? insert - L2 : 0, hi = insert < L1 ? insert : L1;
  gf_oc_counts mine = {{0, 0}, 0};
  for (int32_t w = (lo >> 5) + gl; w <= (hi - 1) >> 5; w += G)
    gf_oc_correct_word(gf_oc_diff_word(s_a, s_r, L1, L2, insert, w), w, insert, Ls.bases + start_l,
                       Ls.quals + start_l, Rs.bases + start_r, Rs.quals + start_r, s, mine);
  const uint32_t sum =
      gf_oc_group_sum<G>((uint32_t)mine.fixed[0] | (uint32_t)mine.fixed[1] << 10 | (uint32_t)mine.left << 20);
  c.fixed[0] = (int32_t)(sum & 1023u);
  c.fixed[1] = (int32_t)((sum >> 10) & 1023u);
  c.left = (int32_t)(sum >> 20);
  return insert;
}

// ---- correct: block b takes the pairs GF_PP_TILE b .., a group of G lanes a pair at a time.  Writes the corrected
// bytes, insert[i] and fixed[side n + i] (either may be null), and the block's share of the totals.
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_oc_k_correct(gf_oc_settings s, gf_at_settings t, GfOcSide L,
                                                                   GfOcSide R, int64_t n, int32_t* __restrict__ insert_out,
                                                                   int32_t* __restrict__ fixed_out,
                                                                   unsigned long long* __restrict__ totals) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ uint32_t s_planes[GROUPS][2][GF_AT_READ_WORDS];
  __shared__ unsigned long long s_tot[GF_OC_TOTALS];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  if (threadIdx.x < GF_OC_TOTALS) s_tot[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long t_found = 0, t_differ = 0, t_reads = 0, t_bases = 0, t_left = 0;
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    gf_oc_counts c;
    const int32_t insert = gf_oc_correct_group<G>(L, R, i, s, t, s_planes[g][0], s_planes[g][1], c);
    if (gl == 0) {
      if (insert_out) insert_out[i] = insert;
      if (fixed_out) {
        fixed_out[i] = c.fixed[0];
        fixed_out[n + i] = c.fixed[1];
      }
      if (insert >= 0) ++t_found;
      if (c.fixed[0] + c.fixed[1] + c.left > 0) ++t_differ;
      t_reads += (c.fixed[0] > 0) + (c.fixed[1] > 0);
      t_bases += (unsigned long long)(c.fixed[0] + c.fixed[1]);
      t_left += (unsigned long long)c.left;
    }
  }
  if (gl == 0) {
    if (t_found) atomicAdd(&s_tot[1], t_found);
    if (t_differ) atomicAdd(&s_tot[2], t_differ);
    if (t_reads) atomicAdd(&s_tot[3], t_reads);
    if (t_bases) atomicAdd(&s_tot[4], t_bases);
    if (t_left) atomicAdd(&s_tot[5], t_left);
  }
  if (threadIdx.x == 0) {
    const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
    atomicAdd(&s_tot[0], (unsigned long long)in_tile);
  }
  __syncthreads();
  if (threadIdx.x < GF_OC_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}
