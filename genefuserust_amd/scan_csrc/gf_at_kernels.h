// The adapter trimming of libgfadapt.so (include/gf_adapter_trim.h) over records in HBM, three kernels:
//
//   decide   what every record keeps and how: the pair overlap, the     gf_at_k_decide (a block per tile of 256 records,
//            adapter sequence, the limits; the kept lengths scanned       G lanes per pair)
//            inside the tile; the totals, one atomic per counter and block
//   offsets  where each tile's records go                                gf_pp_k_scan   (gf_pp_kernels.h, as it is)
//   gather   the kept prefixes of bases and qualities, back to back      gf_pp_k_gather (gf_pp_kernels.h, as it is)
//
// Decide leaves exactly what gf_pp_k_decide leaves: tile-relative offsets in out.off and the tiles' kept bytes, so the
// other two stages are the read filter's.
//
// A group of G lanes takes a pair (gf_at_core.h says what planes, chunks, inserts and rounds are; gf_at_decide_pair
// there is this kernel's walk by one thread).  The bases are loaded once, in aligned 16-byte chunks, a chunk a lane,
// and packed into the group's planes in LDS: a forwards, b as its reverse complement.  Then a lane takes an insert:
// per 32 positions six funnel shifts, two XOR, three OR, a mask and a popcount, no loop over bases.  The inserts go in
// rounds of G from the largest downwards, and a max over the group ends the search in the first round that accepts
// one.  A lane leaves an insert as soon as its differences pass max_diff: a wrong diagonal differs in three positions
// of four, so it costs one word step, not ov / 32.  The sequence step is the same compare against the adapter's planes,
// which are kernel arguments (registers), at a position a lane, in rounds of G from 0 upwards with a min over the group.
// R2's sequence step needs b forwards: only then, in a pair without an I*, is b packed a second time.
//
// G = 16.  A pair of 150-base reads is 2 x 10 or 11 chunks and 240 inserts.  Packing keeps 10 or 11 of 16 lanes busy,
// where a wavefront per pair (G = 64) would keep one lane in six busy; the search is G-independent work per insert, and
// what G changes is how much of it runs past the answer: a round is all or nothing, so on average G / 2 inserts below I*
// are tested for nothing, 8 with G = 16 and 32 with G = 64, while a read-through pair's I* lies 100 to 170 inserts
// below the largest.  Groups of a wavefront run different numbers of rounds and wait for each other; with four pairs a
// wavefront the wait is for the slowest of four, and 16 pairs a group per tile even that out.  Shorter reads gain
// nothing from a smaller G (G = 8 packs 150 bases in two rounds), longer ones up to 512 bases pack in three rounds.
// Measured on 1 M pairs of 150 bases: 1.61 ms a call with G = 16, 2.25 ms with G = 64.
//
// Deterministic: the LDS atomics are ORs of disjoint bits, the totals integer sums.
#pragma once

#include "gf_at_core.h"
#include "gf_pp_kernels.h"

// what the lanes of a group wrote to LDS before is seen by all of them behind this (as in gf_pp_decide_group)
__device__ __forceinline__ void gf_at_group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int G>
__device__ __forceinline__ int gf_at_group_max(int v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    const int y = __shfl_xor(v, o);
    v = y > v ? y : v;
  }
  return v;
}

// the planes of the read at `first` (rc: of its reverse complement), by the G lanes of a group, into zeroed planes
template <int G>
__device__ __forceinline__ void gf_at_pack_group(const uint8_t* first, int32_t L, bool rc, uint32_t* planes) {
  const int gl = threadIdx.x & (G - 1);
  const uintptr_t p = (uintptr_t)first;
  const int a = (int)(p & 15);
  const uint8_t* base = (const uint8_t*)(p - a);
  for (int c = gl; c <= (a + L - 1) >> 4; c += G)
    gf_at_pack_chunk(gf_pp_load(base, c), 16 * c - a, L, rc, [&](int plane, int word, uint32_t bits) {
      atomicOr(&planes[plane * GF_AT_PLANE + word], bits);
    });
}

template <int G>
__device__ __forceinline__ void gf_at_zero_group(uint32_t* planes) {
  for (int k = threadIdx.x & (G - 1); k < GF_AT_READ_WORDS; k += G) planes[k] = 0;
}

// One record, both mates, by the G lanes of a group: what each keeps and how, in every lane of the group.
// s_a / s_r: the group's planes.
template <int G>
__device__ __forceinline__ void gf_at_decide_group(const GfPpSide& Ls, const GfPpSide& Rs, int sides, int64_t i,
                                                   const gf_at_settings& s, const gf_at_adapter& ad_l,
                                                   const gf_at_adapter& ad_r, uint32_t* s_a, uint32_t* s_r,
                                                   int64_t (&kept)[2], int (&how)[2]) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t start_l = Ls.off[i], len_l = Ls.off[i + 1] - start_l;
  const int64_t start_r = sides == 2 ? Rs.off[i] : 0, len_r = sides == 2 ? Rs.off[i + 1] - start_r : 0;
  kept[0] = len_l;
  kept[1] = len_r;
  how[0] = how[1] = GF_AT_UNTOUCHED;
  if (gf_at_passes(len_l) || (sides == 2 && gf_at_passes(len_r))) return;
  const int32_t L1 = (int32_t)len_l, L2 = (int32_t)len_r;
  const bool overlap = sides == 2 && s.overlap;
  gf_at_group_sync();  // (the record before this one has been read to its end)
  gf_at_zero_group<G>(s_a);
  if (overlap) gf_at_zero_group<G>(s_r);
  gf_at_group_sync();
  gf_at_pack_group<G>(Ls.bases + start_l, L1, false, s_a);
  if (overlap) gf_at_pack_group<G>(Rs.bases + start_r, L2, true, s_r);
  gf_at_group_sync();
  if (overlap) {
    const int32_t first = gf_at_first_insert(s);
    int32_t insert = -1;
    for (int32_t top = gf_at_last_insert(L1, L2, s); top >= first; top -= G) {
      const int32_t I = top - gl;
      const bool ok = I >= first && gf_at_try_insert(s_a, s_r, L1, L2, I, s);
      insert = gf_at_group_max<G>(ok ? I : -1);
      if (insert >= 0) break;
    }
    if (insert >= 0) {
      int32_t k;
      how[0] = gf_at_by_overlap(L1, insert, &k);
      kept[0] = k;
      how[1] = gf_at_by_overlap(L2, insert, &k);
      kept[1] = k;
      return;
    }
  }
  for (int side = 0; side < sides; ++side) {
    const gf_at_adapter& ad = side ? ad_r : ad_l;
    if (ad.len <= 0) continue;
    if (side == 1) {  // b forwards, over its reverse complement
      gf_at_group_sync();
      gf_at_zero_group<G>(s_r);
      gf_at_group_sync();
      gf_at_pack_group<G>(Rs.bases + start_r, L2, false, s_r);
      gf_at_group_sync();
    }
    const uint32_t* X = side ? s_r : s_a;
    const int32_t L = side ? L2 : L1, last = L - s.min_adapter;
    for (int32_t p0 = 0; p0 <= last; p0 += G) {
      const int32_t p = p0 + gl;
      const bool ok = p <= last && gf_at_adapter_at(X, L, p, ad);
      const int32_t found = -gf_at_group_max<G>(ok ? -p : -(1 << 20));  // the smallest
      if (found < (1 << 20)) {
        kept[side] = found;
        how[side] = GF_AT_BY_SEQUENCE;
        break;
      }
    }
  }
}

// ---- decide: block b takes the records GF_PP_TILE b .., a group of G lanes a record at a time, both mates.  Writes
// how, the kept lengths as offsets inside the tile (out.off[i], made absolute by gf_pp_k_gather), the tile's kept bytes
// per side (tile_sum[side][b]) and the block's share of the totals.
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_at_k_decide(
    gf_at_settings s, gf_at_adapter ad_l, gf_at_adapter ad_r, GfPpSide L, GfPpSide R, int sides, int64_t n,
    GfPpOut out_l, GfPpOut out_r, int64_t* __restrict__ tile_sum_l, int64_t* __restrict__ tile_sum_r,
    uint8_t* __restrict__ how_out, unsigned long long* __restrict__ totals) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ uint32_t s_planes[GROUPS][2][GF_AT_READ_WORDS];
  __shared__ long long s_len[2][GF_PP_TILE];
  __shared__ unsigned long long s_tot[GF_AT_TOTALS];
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  if (threadIdx.x < GF_AT_TOTALS) s_tot[threadIdx.x] = 0;
  s_len[0][threadIdx.x] = 0;
  s_len[1][threadIdx.x] = 0;
  __syncthreads();
  unsigned long long t_removed = 0, t_how[4] = {0, 0, 0, 0}, t_pairs = 0;
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    int64_t kept[2];
    int how[2];
    gf_at_decide_group<G>(L, R, sides, i, s, ad_l, ad_r, s_planes[g][0], s_planes[g][1], kept, how);
    if (gl == 0) {
      if (how[0] == GF_AT_BY_OVERLAP || how[0] == GF_AT_OVERLAP_CLEAN) ++t_pairs;
      for (int side = 0; side < sides; ++side) {
        const GfPpSide& in = side ? R : L;
        const int64_t had = in.off[i + 1] - in.off[i];
        if (kept[side] < 0) kept[side] = 0;  // (offsets that run backwards: a record of length 0)
        ++t_how[how[side]];
        if (kept[side] < had) t_removed += (unsigned long long)(had - kept[side]);
        s_len[side][r] = kept[side];
        how_out[side * n + i] = (uint8_t)how[side];
      }
    }
  }
  if (gl == 0) {
    if (t_how[GF_AT_BY_OVERLAP] + t_how[GF_AT_BY_SEQUENCE])
      atomicAdd(&s_tot[1], t_how[GF_AT_BY_OVERLAP] + t_how[GF_AT_BY_SEQUENCE]);
    if (t_removed) atomicAdd(&s_tot[2], t_removed);
    if (t_how[GF_AT_BY_OVERLAP]) atomicAdd(&s_tot[3], t_how[GF_AT_BY_OVERLAP]);
    if (t_how[GF_AT_BY_SEQUENCE]) atomicAdd(&s_tot[4], t_how[GF_AT_BY_SEQUENCE]);
    if (t_pairs) atomicAdd(&s_tot[5], t_pairs);
  }
  __syncthreads();
  const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
  if (threadIdx.x == 0) s_tot[0] = (unsigned long long)(in_tile * sides);
  // where each record's kept bytes go inside the tile, per side
  int ea, ta;
  long long el, tl, er, tr;
  gf_scan_block_scan2(0, s_len[0][threadIdx.x], s_a, s_b, ea, el, ta, tl);
  gf_scan_block_scan2(0, s_len[1][threadIdx.x], s_a, s_b, ea, er, ta, tr);
  const int64_t i = tile0 + threadIdx.x;
  if (i < n) {
    out_l.off[i] = el;
    if (sides == 2) out_r.off[i] = er;
  }
  if (threadIdx.x == 0) {
    tile_sum_l[blockIdx.x] = tl;
    if (sides == 2) tile_sum_r[blockIdx.x] = tr;
  }
  __syncthreads();  // (s_tot[0])
  if (threadIdx.x < GF_AT_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}
