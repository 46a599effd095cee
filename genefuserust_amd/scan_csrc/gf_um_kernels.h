// The UMI calls of libgfumi.so (include/gf_umi.h) over records in HBM:
//
//   cut     decide: which records are long enough, U of those, the      gf_um_k_decide (a block per tile of 256 records,
//           lengths they keep scanned inside the tile; the totals, one    G lanes per record)
//           atomic per counter and block
//           offsets and gather                                            gf_pp_k_scan, gf_pp_k_gather (gf_pp_kernels.h,
//                                                                         as they are)
//   names   U of every record's name line; the totals                    gf_um_k_names (a block per tile, G lanes per
//                                                                         record)
//   mix     K' of every record, in place                                  gf_um_k_mix (a thread per record)
//
// The gather is the read filter's, driven through its arguments: it copies the bytes a record keeps from in.bases +
// in.off[i], so a side that loses c bytes at its head is handed bases + c and quals + c.  It loads single bytes, and no
// byte of a record that keeps nothing, so nothing outside the records is read through the shifted pointers.
//
// Decide: a group of G = 16 lanes takes a record, as in gf_dd_k_keys.  A UMI is at most 32 bytes, two pieces of
// gf_dd_core.h, so two lanes of the group hash and the others wait; the offsets, the compare and the scan are what the
// kernel spends its time on, and they are the duplicate removal's.
//
// Names: a name line is 40 - 70 bytes, three to five chunks, a lane each; a round of G chunks covers 256 bytes, longer
// lines take further rounds.  The token's end is the lowest set bit of the group's ballot over "my chunk holds a space
// or tab inside the line", the last colon the highest of the ballot over "my chunk holds a colon in front of that end".
// Then the field, at most 64 bytes, is hashed as a UMI is.  Deterministic: the atomics are integer sums.
#pragma once

#include "gf_pp_kernels.h"
#include "gf_um_core.h"

// chunk c (>= 0) behind the 16-byte aligned address p
__device__ __forceinline__ gf_dd_chunk gf_um_load(const uint8_t* p, int64_t c) {
  const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * c);
  return gf_dd_chunk{{(uint64_t)v.x | (uint64_t)v.y << 32, (uint64_t)v.z | (uint64_t)v.w << 32}};
}

// The lowest lane of this lane's group of G whose `flag` is set: its `value` in every lane of the group, -1 when no
// lane has it (gf_pp_group_last is its mirror).
template <int G>
__device__ __forceinline__ int gf_um_group_first(bool flag, int value) {
  const int lane = threadIdx.x & 63, first = lane & ~(G - 1);
  const unsigned long long all = __ballot(flag);
  const unsigned long long mine = G == 64 ? all : (all >> first) & ((1ull << (G & 63)) - 1ull);
  const int src = mine ? first + __ffsll((long long)mine) - 1 : lane;
  const int got = __shfl(value, src);
  return mine ? got : -1;
}

// H of the L (<= 64) bytes at `first` by the G lanes of a group, in every lane of the group, with whether an N is
// among the bytes and whether a name's field may not hold one of them.  The round loop and the reduction are those of
// gf_dd_hash_group (gf_dd_kernels.h), kept in step by hand: that one returns the sum alone, and the two flags come out
// of the same pieces and shuffles.
template <int G>
__device__ __forceinline__ uint64_t gf_um_hash_group(const uint8_t* first, int64_t L, bool& has_n, bool& invalid) {
  const int gl = threadIdx.x & (G - 1);
  uint64_t sum = 0;
  bool n = false, bad = false;
  if (L > 0) {
    const uintptr_t p = (uintptr_t)first;
    const int a = (int)(p & 15);
    const uint8_t* base = (const uint8_t*)(p - a);
    for (int64_t k = gl; 16 * k < L; k += G) {
      const gf_dd_chunk c0 = gf_um_load(base, k);
      const gf_dd_chunk c1 = gf_dd_needs_next(a, L, k) ? gf_um_load(base, k + 1) : gf_dd_chunk{{0, 0}};
      gf_um_piece(c0, c1, a, L, k, sum, n, bad);
    }
  }
  int flags = (n ? 1 : 0) | (bad ? 2 : 0);
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    sum += __shfl_xor((unsigned long long)sum, o);
    flags |= __shfl_xor(flags, o);
  }
  has_n = flags & 1;
  invalid = flags & 2;
  return gf_dd_finish(L > 0 ? L : 0, sum);
}

// ---- decide: block b takes the records GF_PP_TILE b .., a group of G lanes a record at a time, both mates.  Leaves what
// gf_pp_k_decide leaves: the lengths the records keep as offsets inside the tile (out.off[i], made absolute by
// gf_pp_k_gather) and the tile's kept bytes per side, so that the other two stages are the read filter's.
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_um_k_decide(gf_um_settings s, GfPpSide L, GfPpSide R, int sides,
                                                                  int64_t n, GfPpOut out_l, GfPpOut out_r,
                                                                  int64_t* __restrict__ tile_sum_l,
                                                                  int64_t* __restrict__ tile_sum_r,
                                                                  unsigned long long* __restrict__ codes,
                                                                  unsigned long long* __restrict__ totals) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ long long s_len[2][GF_PP_TILE];
  __shared__ unsigned long long s_tot[GF_UM_TOTALS];
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  if (threadIdx.x < GF_UM_TOTALS) s_tot[threadIdx.x] = 0;
  s_len[0][threadIdx.x] = 0;
  s_len[1][threadIdx.x] = 0;
  __syncthreads();
  const int32_t c = s.length + s.skip;
  const bool takes_l = gf_um_takes(s.source, 0), takes_r = sides == 2 && gf_um_takes(s.source, 1);
  unsigned long long t_tagged = 0, t_n = 0, t_cut = 0, t_short = 0, t_removed = 0;
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    const int64_t start_l = L.off[i], len_l = gf_dd_length(start_l, L.off[i + 1]);
    int64_t start_r = 0, len_r = 0;
    if (sides == 2) {
      start_r = R.off[i];
      len_r = gf_dd_length(start_r, R.off[i + 1]);
    }
    const bool stays = !(takes_l && !gf_um_long_enough(len_l, c)) && !(takes_r && !gf_um_long_enough(len_r, c));
    uint64_t h_l = 0, h_r = 0, code = 0;
    bool n_l = false, n_r = false, bad;
    if (stays) {  // (the same in every lane of the group)
      if (takes_l) h_l = gf_um_hash_group<G>(L.bases + start_l, s.length, n_l, bad);
      if (takes_r) h_r = gf_um_hash_group<G>(R.bases + start_r, s.length, n_r, bad);
      code = takes_l && takes_r ? gf_um_code_pair(h_l, h_r) : gf_um_code(takes_l ? h_l : h_r);
    }
    if (gl == 0) {
      codes[i] = code;
      if (stays) {
        ++t_tagged;
        if (n_l || n_r) ++t_n;
        t_cut += (unsigned long long)((takes_l ? c : 0) + (takes_r ? c : 0));
        s_len[0][r] = len_l - (takes_l ? c : 0);
        s_len[1][r] = len_r - (takes_r ? c : 0);
      } else {
        ++t_short;
        t_removed += (unsigned long long)(len_l + len_r);
      }
    }
  }
  if (gl == 0) {
    if (t_tagged) atomicAdd(&s_tot[1], t_tagged);
    if (t_n) atomicAdd(&s_tot[3], t_n);
    if (t_cut) atomicAdd(&s_tot[4], t_cut);
    if (t_short) atomicAdd(&s_tot[5], t_short);
    if (t_removed) atomicAdd(&s_tot[6], t_removed);
  }
  __syncthreads();
  const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
  if (threadIdx.x == 0) s_tot[0] = (unsigned long long)in_tile;
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
  if (threadIdx.x < GF_UM_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

// ---- names: block b takes the records GF_PP_TILE b .., a group of G lanes a name line at a time
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_um_k_names(const uint8_t* __restrict__ text, int64_t text_bytes,
                                                                 const int64_t* __restrict__ nl_pos, int64_t newlines,
                                                                 int64_t n, unsigned long long* __restrict__ codes,
                                                                 unsigned long long* __restrict__ totals) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ unsigned long long s_tot[GF_UM_TOTALS];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  if (threadIdx.x < GF_UM_TOTALS) s_tot[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long t_tagged = 0, t_missing = 0, t_n = 0;
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    uint64_t code = 0;
    bool has_n = false;
    int64_t s, e;
    if (gf_um_name_line(nl_pos, newlines, text_bytes, i, s, e)) {  // (the same in every lane of the group)
      if (e > s && text[e - 1] == '\r') --e;
      const int64_t len = e - s;
      const uintptr_t p = (uintptr_t)(text + s);
      const int a = (int)(p & 15);
      const uint8_t* base = (const uint8_t*)(p - a);
      int64_t end = len, colon = -1;
      for (int64_t c0 = 0; 16 * c0 - a < len; c0 += G) {
        const int64_t p0 = 16 * (c0 + gl) - a, round0 = 16 * c0 - a;
        const uint32_t in_line = gf_um_range(p0, 0, len);
        // (a chunk with no byte of the line is not loaded)
        const gf_dd_chunk v = in_line ? gf_um_load(base, c0 + gl) : gf_dd_chunk{{0, 0}};
        const uint32_t sp = gf_um_space_mask(v) & in_line;
        const int found = gf_um_group_first<G>(sp != 0, sp ? 16 * gl + gf_um_low_bit(sp) : 0);
        if (found >= 0) end = round0 + found;
        const uint32_t co = gf_um_colon_mask(v) & gf_um_range(p0, 0, end);
        const int last = gf_pp_group_last<G>(co != 0, co ? 16 * gl + gf_um_high_bit(co) : 0);
        if (last >= 0) colon = round0 + last;
        if (found >= 0) break;
      }
      int64_t f_start, f_len;
      if (gf_um_field(colon, end, f_start, f_len)) {
        bool n_in, invalid;
        const uint64_t h = gf_um_hash_group<G>(text + s + f_start, f_len, n_in, invalid);
        if (!invalid) {
          code = gf_um_code(h);
          has_n = n_in;
        }
      }
    }
    if (gl == 0) {
      codes[i] = code;
      if (code) ++t_tagged;
      else ++t_missing;
      if (has_n) ++t_n;
    }
  }
  if (gl == 0) {
    if (t_tagged) atomicAdd(&s_tot[1], t_tagged);
    if (t_missing) atomicAdd(&s_tot[2], t_missing);
    if (t_n) atomicAdd(&s_tot[3], t_n);
  }
  const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
  if (threadIdx.x == 0) atomicAdd(&s_tot[0], (unsigned long long)in_tile);
  __syncthreads();
  if (threadIdx.x < GF_UM_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

// ---- mix: a thread a record
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_um_k_mix(unsigned long long* __restrict__ rec_keys,
                                                               const unsigned long long* __restrict__ codes,
                                                               int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * GF_SCAN_THREADS + threadIdx.x;
  if (i < n) rec_keys[i] = gf_um_mix_key(rec_keys[i], codes[i]);
}
