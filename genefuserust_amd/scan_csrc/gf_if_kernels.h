// The kernels of libgfinflate.so (include/gf_inflate.h): BGZF members inflated on the device, one wavefront a member.
//
// The decoder is gf_if_core.h, the text the host tests run; the whole wave runs it with the same values (the decoder's
// state is uniform, the compiler keeps it in scalar registers) and shares what a match copies.  A member's text, at most
// 64 KiB, lives in LDS until it is complete and its CRC-32 is right: a byte that another lane stored to global memory
// is not safely visible to a later load, a byte in LDS is after a barrier.  Only then is the window written out, in
// 16-byte stores where the output's address allows and bytewise at the member's unaligned head and tail — never past its
// own range, the neighbouring members' bytes are next to it.  A member that fails writes nothing but its status.
//
// No scratch, no communication between workgroups, no atomics: the totals are a second, one-block kernel's.
#pragma once

#include <hip/hip_runtime.h>

#include "gf_if_core.h"

#define GF_IF_THREADS 64            // one wavefront: gf_if_core.h's GF_IF_LEADER and GF_IF_UNIFORM rest on it
#define GF_IF_MAX_BLOCKS 512        // 64 KiB of window + tables: two workgroups a CU, 256 CUs
#define GF_IF_TOTALS_THREADS 256
static_assert(GF_IF_THREADS == GF_IF_LANES, "the CRC's pieces are a lane each");

// where a member's bytes go on the device: the window in LDS
struct GfIfWindow {
  uint8_t* w;

  __device__ void put(uint32_t pos, uint8_t v) {
    if (threadIdx.x == 0) w[pos] = v;
  }
  __device__ void raw(uint32_t pos, const uint8_t* src, uint32_t len) {
    for (uint32_t i = threadIdx.x; i < len; i += GF_IF_THREADS) w[pos + i] = src[i];
  }
  // byte pos + i is byte pos - dist + (i % dist): every source lies before pos, where the bytes are final
  __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
    __syncthreads();  // (the literals and copies before this one are in the window)
    const uint8_t* from = w + pos - dist;
    for (uint32_t i = threadIdx.x; i < len; i += GF_IF_THREADS) w[pos + i] = from[dist >= len ? i : i % dist];
  }
};

__global__ __launch_bounds__(GF_IF_THREADS) void gf_if_k_inflate(const uint8_t* __restrict__ comp, int64_t comp_bytes,
                                                                  const int64_t* __restrict__ table, int64_t n_members,
                                                                  uint8_t* __restrict__ out, int64_t out_cap,
                                                                  int32_t* __restrict__ status) {
  // (the window starts up to 15 bytes into its block, where its address is the output's modulo 16)
  __shared__ __attribute__((aligned(16))) uint8_t s_win[GF_IF_MAX_TEXT + 16];
  __shared__ GfIfTables s_tables;
  __shared__ uint32_t s_crc_table[256];
  __shared__ uint32_t s_pieces[GF_IF_LANES];
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < 256; i += GF_IF_THREADS) s_crc_table[i] = gf_if_crc_table_entry(i);
  __syncthreads();

  for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
    const int64_t* row = table + m * GF_IF_ROW;
    int st = GF_IF_BAD_ROW;
    if (gf_if_row_ok(row, comp_bytes, out_cap)) {
      const uint32_t n_bytes = (uint32_t)row[1], isize = (uint32_t)row[3];
      uint8_t* dst = out + row[2];
      const uint32_t shift = (uint32_t)((uintptr_t)dst & 15u);
      GfIfWindow win{s_win + shift};
      st = gf_if_inflate_member(comp + row[0], n_bytes, isize, s_tables, win);
      __syncthreads();  // (the window is complete)
      if (st == GF_IF_OK) {
        s_pieces[lane] = gf_if_crc_piece(s_crc_table, win.w, isize, lane);
        __syncthreads();
        if (gf_if_crc_join(s_pieces, isize) != (uint32_t)row[4]) st = GF_IF_CRC;
      }
      if (st == GF_IF_OK) {
        // [0, head): up to the first 16-byte boundary of the output; [head, body): whole 16-byte pieces; [body, isize)
        const uint32_t lead = (16u - shift) & 15u, head = lead < isize ? lead : isize;
        const uint32_t body = head + ((isize - head) & ~15u);
        for (uint32_t i = lane; i < head; i += GF_IF_THREADS) dst[i] = win.w[i];
        for (uint32_t i = head + 16u * lane; i < body; i += 16u * GF_IF_THREADS)
          *(uint4*)(dst + i) = *(const uint4*)(win.w + i);
        for (uint32_t i = body + lane; i < isize; i += GF_IF_THREADS) dst[i] = win.w[i];
      }
    }
    if (lane == 0) status[m] = st;
    __syncthreads();  // (the window and the pieces are read; the next member may overwrite them)
  }
}

// d_totals (int64[4]): members inflated, the first failed member or -1, its status, bytes of text written.  One block.
__global__ __launch_bounds__(GF_IF_TOTALS_THREADS) void gf_if_k_totals(const int32_t* __restrict__ status,
                                                                        const int64_t* __restrict__ table, int64_t n_members,
                                                                        int64_t* __restrict__ totals) {
  __shared__ int64_t s_ok[GF_IF_TOTALS_THREADS], s_first[GF_IF_TOTALS_THREADS], s_bytes[GF_IF_TOTALS_THREADS];
  const uint32_t t = threadIdx.x;
  int64_t ok = 0, first = INT64_MAX, bytes = 0;
  for (int64_t m = t; m < n_members; m += GF_IF_TOTALS_THREADS) {
    if (status[m] == GF_IF_OK) ok++, bytes += table[m * GF_IF_ROW + 3];
    else if (m < first) first = m;
  }
  s_ok[t] = ok, s_first[t] = first, s_bytes[t] = bytes;
  __syncthreads();
  for (uint32_t half = GF_IF_TOTALS_THREADS / 2; half > 0; half >>= 1) {
    if (t < half) {
      s_ok[t] += s_ok[t + half];
      s_bytes[t] += s_bytes[t + half];
      if (s_first[t + half] < s_first[t]) s_first[t] = s_first[t + half];
    }
    __syncthreads();
  }
  if (t == 0) {
    const int64_t f = s_first[0];
    totals[0] = s_ok[0];
    totals[1] = f == INT64_MAX ? -1 : f;
    totals[2] = f == INT64_MAX ? 0 : status[f];
    totals[3] = s_bytes[0];
  }
}
