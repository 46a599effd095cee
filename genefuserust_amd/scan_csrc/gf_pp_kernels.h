// The read filter of libgfprep.so (include/gf_read_filter.h) over records in HBM, three kernels:
//
//   decide   kept length and reason of every record, both mates      gf_pp_k_decide (a block per tile of 256 records,
//            and the pair rule; the kept lengths scanned inside the    G lanes per record)
//            tile; the totals, one atomic per counter and block
//   offsets  where each tile's records go: an exclusive scan of the   gf_pp_k_scan (one block, in place on the tiles'
//            tiles' kept bytes, per side                               sums: gf_scan_totals_block)
//   gather   the kept prefixes of bases and qualities, back to back   gf_pp_k_gather (a block per tile, a wavefront per
//                                                                      record, a byte per lane: coalesced both ways)
//
// Decide reads every base and quality byte in aligned 16-byte loads, a chunk per lane (gf_pp_core.h says what a chunk,
// a tile and the window step are; gf_pp_decide_read there is this kernel's walk by one thread).  G lanes share a record:
// a read of 150 bases is 10 or 11 chunks, so with G = 16 four records fill a wavefront's 64 lanes to two thirds, where a
// wavefront per record (G = 64) would leave five lanes in six idle on every instruction.  The last tile of a record —
// all of it, up to 241 bases — is loaded once and stays in registers for all three steps; longer records walk further
// tiles towards their start, and a group loops alone while the other groups of its wavefront wait.  "The last position
// where a predicate holds" is a ballot over the lanes' own answers and the highest set bit of the group's 16 bits.
// Deterministic: the atomics are integer sums.
#pragma once

#include "gf_pp_core.h"
#include "gf_scan_common.h"

#define GF_PP_TILE GF_SCAN_THREADS  // records per block of decide and gather: what the offsets scan counts as one

struct GfPpSide {
  const uint8_t* bases;
  const uint8_t* quals;
  const int64_t* off;
};

struct GfPpOut {
  uint8_t* bases;
  uint8_t* quals;
  int64_t* off;
};

// chunk c (>= 0) behind the 16-byte aligned address p
__device__ __forceinline__ gf_pp_chunk gf_pp_load(const uint8_t* p, int c) {
  const uint4 v = *reinterpret_cast<const uint4*>(p + 16 * (int64_t)c);
  return gf_pp_chunk{{v.x, v.y, v.z, v.w}};
}

// the chunk, or zeros in front of the record's chunk 0
__device__ __forceinline__ gf_pp_chunk gf_pp_load_or_zero(const uint8_t* p, int c) {
  return c >= 0 ? gf_pp_load(p, c) : gf_pp_chunk{{0, 0, 0, 0}};
}

// The highest lane of this lane's group of G whose `flag` is set: its `value` in every lane of the group, -1 when no
// lane has it.  The lanes of a group run together, whatever the other groups of the wavefront do.
template <int G>
__device__ __forceinline__ int gf_pp_group_last(bool flag, int value) {
  const int lane = threadIdx.x & 63, first = lane & ~(G - 1);
  const unsigned long long all = __ballot(flag);
  const unsigned long long mine = G == 64 ? all : (all >> first) & ((1ull << (G & 63)) - 1ull);
  const int src = mine ? first + 63 - __clzll((long long)mine) : lane;
  const int got = __shfl(value, src);
  return mine ? got : -1;
}

// One record of one side by the G lanes of a group: its kept length and its own reason, in every lane of the group.
// s_S: the group's 16 x (G + 1) prefix sums of the window step, S[j] at row j & 15, column j >> 4, so that the lanes
// of a group store and load neighbouring columns of one row.
template <int G>
__device__ __forceinline__ int gf_pp_decide_group(const GfPpSide& side, int64_t i, const gf_pp_settings& s,
                                                  uint16_t* s_S, int64_t& kept) {
  const int gl = threadIdx.x & (G - 1);
  const int64_t start = side.off[i], len64 = side.off[i + 1] - start;
  if (len64 > GF_MAX_READ_LEN) {
    kept = len64;
    return GF_PP_KEPT;
  }
  const int32_t L = len64 < 0 ? 0 : (int32_t)len64;
  int32_t e2 = 0, n_bases = 0, low = 0;
  if (L > 0) {
    const uintptr_t pb = (uintptr_t)(side.bases + start), pq = (uintptr_t)(side.quals + start);
    const int ab = (int)(pb & 15), aq = (int)(pq & 15);
    const uint8_t* bases = (const uint8_t*)(pb - ab);
    const uint8_t* quals = (const uint8_t*)(pq - aq);
    const int top_b = (ab + L - 1) >> 4, top_q = (aq + L - 1) >> 4;
    // the last tile, this lane's chunk of it: loaded once for all three steps
    const gf_pp_chunk last_b = gf_pp_load_or_zero(bases, top_b - (G - 1) + gl);
    const gf_pp_chunk last_q = gf_pp_load_or_zero(quals, top_q - (G - 1) + gl);

    int32_t e1 = L;
    if (s.poly_g_min > 0) {
      int32_t last = -1;
      for (int top = top_b;; top -= G) {
        const int c = top - (G - 1) + gl;
        uint32_t m = 0;
        if (c >= 0) m = gf_pp_not_g_mask(top == top_b ? last_b : gf_pp_load(bases, c)) & gf_pp_range(16 * c - ab, 0, L);
        last = gf_pp_group_last<G>(m != 0, m ? 16 * c - ab + gf_pp_top_bit(m) : 0);
        if (last >= 0 || top - (G - 1) <= 0) break;
      }
      if (L - 1 - last >= s.poly_g_min) e1 = last + 1;
    }

    e2 = e1;
    const int32_t W = s.cut_tail_window;
    if (W > 0) {
      e2 = 0;
      if (e1 >= W) {
        const uint32_t need = (uint32_t)(W * s.cut_tail_mean);
        for (int top = top_q;; top -= G - GF_PP_HALO) {
          const int c0 = top - (G - 1);
          const int32_t p0 = 16 * c0 - aq;
          uint32_t p[16];
          gf_pp_phred_prefix(top == top_q ? last_q : gf_pp_load_or_zero(quals, c0 + gl), p);
          // S[16 gl]: the sums of the chunks in front of this lane's
          uint32_t incl = p[15];
#pragma unroll
          for (int o = 1; o < G; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (gl >= o) incl += y;
          }
          const uint32_t base = incl - p[15];
          if (gl == 0) s_S[0] = 0;
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int j = 16 * gl + k + 1;
            s_S[(j & 15) * (G + 1) + (j >> 4)] = (uint16_t)(base + p[k]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          const uint32_t ends = gf_pp_range(p0 + 16 * gl + 1, W, e1 + 1);
          const uint32_t hit = gf_pp_window_ends(gl, base, p, ends, W, need, [&](int j) {
            return (uint32_t)s_S[(j & 15) * (G + 1) + (j >> 4)];
          });
          const int found = gf_pp_group_last<G>(hit != 0, hit ? p0 + 16 * gl + gf_pp_top_bit(hit) + 1 : 0);
          // (the next round stores into s_S: every lane of the group has loaded what it needs before any goes on)
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          if (found >= 0) {
            e2 = found;
            break;
          }
          if (p0 <= 0) break;
        }
      }
    }

    if (e2 > 0) {
      uint32_t both = 0;  // low << 16 | n: neither passes 4096
      for (int r = 0;; ++r) {
        const int cb = top_b - (G - 1) - r * G + gl, cq = top_q - (G - 1) - r * G + gl;
        if (cb >= 0)
          both += gf_pp_popcount(gf_pp_n_mask(r == 0 ? last_b : gf_pp_load(bases, cb)) & gf_pp_range(16 * cb - ab, 0, e2));
        if (cq >= 0)
          both += gf_pp_popcount(gf_pp_low_mask(r == 0 ? last_q : gf_pp_load(quals, cq), s.qualified_phred) &
                                 gf_pp_range(16 * cq - aq, 0, e2)) << 16;
        if (top_b - (G - 1) - r * G <= 0 && top_q - (G - 1) - r * G <= 0) break;
      }
#pragma unroll
      for (int o = 1; o < G; o <<= 1) both += __shfl_xor(both, o);
      n_bases = (int32_t)(both & 0xFFFFu);
      low = (int32_t)(both >> 16);
    }
  }
  kept = e2;
  return gf_pp_reason(e2, n_bases, low, s);
}

// ---- decide: block b takes the records GF_PP_TILE b .., a group of G lanes a record at a time, both mates.  Writes the
// reasons, the kept lengths as offsets inside the tile (out.off[i], made absolute by gf_pp_k_gather), the tile's kept
// bytes per side (tile_sum[side][b]) and the block's share of the totals.
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_pp_k_decide(
    gf_pp_settings s, GfPpSide L, GfPpSide R, int sides, int64_t n, GfPpOut out_l, GfPpOut out_r,
    int64_t* __restrict__ tile_sum_l, int64_t* __restrict__ tile_sum_r, uint8_t* __restrict__ reasons,
    unsigned long long* __restrict__ totals) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ uint16_t s_S[GROUPS][16 * (G + 1)];
  __shared__ long long s_len[2][GF_PP_TILE];
  __shared__ unsigned long long s_tot[GF_PP_TOTALS];
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE;
  if (threadIdx.x < GF_PP_TOTALS) s_tot[threadIdx.x] = 0;
  s_len[0][threadIdx.x] = 0;
  s_len[1][threadIdx.x] = 0;
  __syncthreads();
  unsigned long long t_kept = 0, t_short = 0, t_removed = 0, t_reason[5] = {0, 0, 0, 0, 0};
  for (int r = g; r < GF_PP_TILE; r += GROUPS) {
    const int64_t i = tile0 + r;
    if (i >= n) break;
    int64_t kept[2] = {0, 0}, had[2] = {0, 0};
    int reason[2] = {GF_PP_KEPT, GF_PP_KEPT};
    had[0] = L.off[i + 1] - L.off[i];
    reason[0] = gf_pp_decide_group<G>(L, i, s, s_S[g], kept[0]);
    if (sides == 2) {
      had[1] = R.off[i + 1] - R.off[i];
      reason[1] = gf_pp_decide_group<G>(R, i, s, s_S[g], kept[1]);
      gf_pp_pair_rule(reason[0], reason[1]);
    }
    if (gl == 0) {
      for (int side = 0; side < sides; ++side) {
        if (reason[side] != GF_PP_KEPT) kept[side] = 0;
        else {
          ++t_kept;
          if (kept[side] < had[side]) {
            ++t_short;
            t_removed += (unsigned long long)(had[side] - kept[side]);
          }
        }
        ++t_reason[reason[side]];
        s_len[side][r] = kept[side];
        reasons[side * n + i] = (uint8_t)reason[side];
      }
    }
  }
  if (gl == 0) {
    if (t_kept) atomicAdd(&s_tot[1], t_kept);
    if (t_short) atomicAdd(&s_tot[2], t_short);
    if (t_removed) atomicAdd(&s_tot[3], t_removed);
    for (int k = 1; k < 5; ++k)
      if (t_reason[k]) atomicAdd(&s_tot[3 + k], t_reason[k]);
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
  if (threadIdx.x < GF_PP_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

// ---- offsets: the tiles' kept bytes, per side, to where each tile starts; entry `tiles` and out.off[n] the sum.  One
// block, in place (gf_scan_totals_block).
template <int S>
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_pp_k_scan(int64_t* tile_sum_l, int64_t* tile_sum_r,
                                                                       int64_t tiles, int64_t n, int64_t* off_l,
                                                                       int64_t* off_r) {
  long long total[S];
  if constexpr (S == 2) {
    int64_t* const both[2] = {tile_sum_l, tile_sum_r};
    gf_scan_totals_block(both, both, tiles, total);
  } else {
    total[0] = gf_scan_totals_block(tile_sum_l, tile_sum_l, tiles);
  }
  if (threadIdx.x == 0) {
    tile_sum_l[tiles] = total[0];
    off_l[n] = total[0];
    if (S == 2) {
      tile_sum_r[tiles] = total[S - 1];
      off_r[n] = total[S - 1];
    }
  }
}

// ---- gather: block b makes the offsets of its tile absolute and copies the kept prefixes, a wavefront a record
// (lane j: bytes j, j + 64, ..).
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_pp_k_gather(GfPpSide L, GfPpSide R, int sides, int64_t n,
                                                                  GfPpOut out_l, GfPpOut out_r,
                                                                  const int64_t* __restrict__ tile_start_l,
                                                                  const int64_t* __restrict__ tile_start_r) {
  __shared__ long long s_at[2][GF_PP_TILE + 1];
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE, i = tile0 + threadIdx.x;
  const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
  for (int side = 0; side < sides; ++side) {
    const GfPpOut& out = side ? out_r : out_l;
    const int64_t* tile_start = side ? tile_start_r : tile_start_l;
    const long long first = tile_start[blockIdx.x], bytes = tile_start[blockIdx.x + 1] - first;
    s_at[side][threadIdx.x] = first + (i < n ? out.off[i] : bytes);
    if (threadIdx.x == 0) s_at[side][GF_PP_TILE] = first + bytes;
  }
  __syncthreads();
  for (int side = 0; side < sides; ++side) {
    const GfPpOut& out = side ? out_r : out_l;
    if (i < n) out.off[i] = s_at[side][threadIdx.x];
  }
  const int lane = threadIdx.x & 63;
  for (int side = 0; side < sides; ++side) {
    const GfPpSide& in = side ? R : L;
    const GfPpOut& out = side ? out_r : out_l;
    for (int r = threadIdx.x >> 6; r < in_tile; r += GF_SCAN_THREADS / 64) {
      const long long to = s_at[side][r], len = s_at[side][r + 1] - to;
      if (len <= 0) continue;
      const int64_t from = in.off[tile0 + r];
      const uint8_t* __restrict__ b = in.bases + from;
      const uint8_t* __restrict__ q = in.quals + from;
#pragma unroll 1
      for (long long j = lane; j < len; j += 64) {
        out.bases[to + j] = b[j];
        out.quals[to + j] = q[j];
      }
    }
  }
}
