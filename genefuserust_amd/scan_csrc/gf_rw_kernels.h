// The FASTQ output of libgfwrite.so (include/gf_read_write.h) over records in HBM, three kernels:
//
//   sizes    the output bytes of every record, both sides, scanned        gf_rw_k_sizes (a block per tile of 256 records,
//            inside the tile; the first token's length of a tagged name;    a thread per record)
//            the totals, one atomic per counter and block
//   offsets  where each tile's records go, per side                        gf_pp_k_scan (gf_pp_kernels.h, as it is)
//   format   the tile's offsets made absolute, the records' text           gf_rw_k_format (a block per tile, G lanes per
//                                                                           record)
//
// Format: a group of G = 16 lanes takes a record, as in gf_dd_k_keys and gf_pp_k_decide: a pair's record of 150 bases
// and a name of 50 bytes is 355 bytes, 23 pieces (gf_rw_core.h says what a segment and a piece are), two rounds of a
// group.  A lane builds its piece from aligned 16-byte loads of the sources — the chunk the piece starts in and the one
// behind it, its neighbour's, from the cache — funnel-shifted and masked, and stores it with one 16-byte store at an
// aligned output address.  The partial pieces at a record's head and tail go out by byte stores: two records may share
// a piece, and no lane writes a byte outside its own record's span.  gather GF_RW_BYTES is the plain gather the
// project's other libraries have, a byte per lane and store over the same segment table, kept so that a run can
// measure one against the other.
#pragma once

#include "gf_pp_kernels.h"
#include "gf_rw_core.h"

struct GfRwOut {
  uint8_t* text;
  int64_t cap;
  int64_t* off;
};

struct GfRwSides {
  gf_rw_in in[2];
};

// ---- sizes: thread t of block b takes record GF_PP_TILE b + t, both sides.  Leaves the sizes as offsets inside the
// tile (out.off[i], made absolute by gf_rw_k_format), the tile's bytes per side, and with a tag the first token's
// length of every written record's name line (tok[side n + i]).
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_rw_k_sizes(gf_rw_settings s, GfRwSides sides_in, int sides,
                                                                 int64_t n, int64_t* __restrict__ off_l,
                                                                 int64_t* __restrict__ off_r,
                                                                 int64_t* __restrict__ tile_sum_l,
                                                                 int64_t* __restrict__ tile_sum_r,
                                                                 int64_t* __restrict__ tok,
                                                                 unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long s_tot[GF_RW_TOTALS];
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t i = (int64_t)blockIdx.x * GF_PP_TILE + threadIdx.x;
  if (threadIdx.x < GF_RW_TOTALS) s_tot[threadIdx.x] = 0;
  __syncthreads();
  long long size[2] = {0, 0};
  int64_t lens[2] = {0, 0};
  if (i < n) {
    for (int side = 0; side < sides; ++side) {
      gf_rw_record r;
      gf_rw_sources S;
      size[side] = gf_rw_describe(s.umi_source, s.umi_length, sides_in.in, sides, side, i, -1, r, S, lens);
      if (size[side] > 0 && r.tag.len) tok[side * n + i] = r.start[1];
    }
  }
  // the block's share of the totals: a wavefront's sums first
  const bool written = i < n && size[0] > 0;
  unsigned long long w = written ? 1 : 0, b = written ? (unsigned long long)(lens[0] + lens[1]) : 0,
                     d = i < n && !written ? 1 : 0;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    w += __shfl_xor(w, o);
    b += __shfl_xor(b, o);
    d += __shfl_xor(d, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (w) atomicAdd(&s_tot[0], w);
    if (b) atomicAdd(&s_tot[1], b);
    if (d) atomicAdd(&s_tot[4], d);
  }
  int ea, ta;
  long long el, tl, er, tr;
  gf_scan_block_scan2(0, size[0], s_a, s_b, ea, el, ta, tl);
  gf_scan_block_scan2(0, size[1], s_a, s_b, ea, er, ta, tr);
  if (i < n) {
    off_l[i] = el;
    if (sides == 2) off_r[i] = er;
  }
  if (threadIdx.x == 0) {
    tile_sum_l[blockIdx.x] = tl;
    s_tot[2] = (unsigned long long)tl;
    if (sides == 2) {
      tile_sum_r[blockIdx.x] = tr;
      s_tot[3] = (unsigned long long)tr;
    }
  }
  __syncthreads();
  if (threadIdx.x < GF_RW_TOTALS && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

// the aligned 16-byte chunk at `address`
__device__ __forceinline__ gf_dd_chunk gf_rw_load(uintptr_t address, uintptr_t, uintptr_t) {
  const uint4 v = *reinterpret_cast<const uint4*>(address);
  return gf_dd_chunk{{(uint64_t)v.x | (uint64_t)v.y << 32, (uint64_t)v.z | (uint64_t)v.w << 32}};
}

// ---- format: block b makes the offsets of its tile absolute and writes its records, a group of G lanes a record at a
// time, one side after the other.  A record that would end behind out.cap is left out.
template <int G, bool WIDE>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_rw_k_format(gf_rw_settings s, GfRwSides sides_in, int sides,
                                                                  int64_t n, GfRwOut out_l, GfRwOut out_r,
                                                                  const int64_t* __restrict__ tile_start_l,
                                                                  const int64_t* __restrict__ tile_start_r,
                                                                  const int64_t* __restrict__ tok) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ long long s_at[2][GF_PP_TILE + 1];
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t tile0 = (int64_t)blockIdx.x * GF_PP_TILE, mine = tile0 + threadIdx.x;
  const int64_t in_tile = n - tile0 < GF_PP_TILE ? n - tile0 : GF_PP_TILE;
  for (int side = 0; side < sides; ++side) {
    const GfRwOut& out = side ? out_r : out_l;
    const int64_t* tile_start = side ? tile_start_r : tile_start_l;
    const long long first = tile_start[blockIdx.x], bytes = tile_start[blockIdx.x + 1] - first;
    s_at[side][threadIdx.x] = first + (mine < n ? out.off[mine] : bytes);
    if (threadIdx.x == 0) s_at[side][GF_PP_TILE] = first + bytes;
  }
  __syncthreads();
  for (int side = 0; side < sides; ++side) {
    const GfRwOut& out = side ? out_r : out_l;
    if (mine < n) out.off[mine] = s_at[side][threadIdx.x];
  }
  const bool tagged = gf_um_inline_source(s.umi_source);
  for (int side = 0; side < sides; ++side) {
    const GfRwOut& out = side ? out_r : out_l;
    for (int r = g; r < in_tile; r += GROUPS) {
      const long long to = s_at[side][r], size = s_at[side][r + 1] - to;
      if (size <= 0 || to + size > out.cap) continue;  // (the same in every lane of the group)
      const int64_t i = tile0 + r;
      gf_rw_record rec;
      gf_rw_sources S;
      int64_t lens[2];
      gf_rw_describe(s.umi_source, s.umi_length, sides_in.in, sides, side, i, tagged ? tok[side * n + i] : 0, rec, S,
                     lens);
      uint8_t* const dst = out.text + to;
      if (WIDE) {
        const int a = (int)((uintptr_t)dst & 15);
        const int64_t pieces = gf_rw_pieces(a, size);
#pragma unroll 1
        for (int64_t q = gl; q < pieces; q += G) {
          const int64_t p = gf_rw_piece_pos(a, q);
          const gf_dd_chunk v = gf_rw_piece(rec, S, p, gf_rw_load);
          if (gf_rw_piece_full(p, size)) {
            *reinterpret_cast<uint4*>(dst + p) =
                make_uint4((uint32_t)v.q[0], (uint32_t)(v.q[0] >> 32), (uint32_t)v.q[1], (uint32_t)(v.q[1] >> 32));
          } else {
            int k_lo, k_hi;
            gf_rw_piece_part(p, size, k_lo, k_hi);
            for (int k = k_lo; k < k_hi; ++k) dst[p + k] = (uint8_t)(v.q[k >> 3] >> (8 * (k & 7)));
          }
        }
      } else {
#pragma unroll 1
        for (int64_t j = gl; j < size; j += G) dst[j] = gf_rw_byte(rec, S, j);
      }
    }
  }
}
