// The kernels of libgfreport.so (include/gf_report.h): the filter reason of every match, and the refined break of every
// match of every cluster.
//
// The arithmetic is gf_rp_core.h, the text the host tests run.  A wavefront is that header's Wave: a lane holds one
// symbol of the pattern block, one symbol of the text chunk and one word of each carry vector, all in registers; the
// match mask of a text symbol is one ballot, a symbol or a carry word reaches the scalar side through a readlane.  The
// recurrence's state is the same in every lane, so the compiler keeps it in scalar registers and the inner loop of a
// distance issues one vector compare and no memory instruction.
//
// gf_rp_k_adjust: one workgroup of 14 wavefronts per match, one wavefront per (shift, side): the 20-base window and the
// whole overlap of that side.  The 28 numbers meet in LDS and the first lane chooses the shift.  gf_rp_k_filter: one
// wavefront per match.  Both stride over the matches with a capped grid.  No scratch, no atomics, no communication
// between workgroups; every offset is checked against its array before anything is read through it.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/gfmatch.h"
#include "gf_rp_core.h"

#define GF_RP_ADJUST_WAVES (2 * GF_RP_SHIFTS)          // a wavefront per (shift, side)
#define GF_RP_ADJUST_THREADS (64 * GF_RP_ADJUST_WAVES)
#define GF_RP_ADJUST_MAX_BLOCKS 2048
#define GF_RP_FILTER_THREADS 256
#define GF_RP_FILTER_MAX_BLOCKS 2048

struct GfRpWave {
  uint32_t lane;
  uint32_t pat, sym;                    // this lane's symbol of the pattern block and of the text chunk
  uint32_t cp_lo, cp_hi, cn_lo, cn_hi;  // this lane's word of the carry vectors

  __device__ explicit GfRpWave(uint32_t lane_) : lane(lane_), pat(GF_RP_NO_SYMBOL), sym(GF_RP_NO_SYMBOL), cp_lo(0), cp_hi(0), cn_lo(0), cn_hi(0) {}

  __device__ void load_pattern(const uint8_t* p, int32_t n) { pat = (int32_t)lane < n ? p[lane] : GF_RP_NO_SYMBOL; }
  __device__ void load_symbols(const uint8_t* p, int32_t n) { sym = (int32_t)lane < n ? p[lane] : GF_RP_NO_SYMBOL; }
  __device__ uint32_t symbol(int32_t j) const { return (uint32_t)__builtin_amdgcn_readlane((int)sym, j); }
  __device__ uint64_t eq(uint32_t c) const { return __ballot(pat == c); }
  __device__ void carry_load(int32_t k, uint64_t& p, uint64_t& n) const {
    p = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cp_lo, k) |
        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cp_hi, k) << 32);
    n = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cn_lo, k) |
        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cn_hi, k) << 32);
  }
  __device__ void carry_store(int32_t k, uint64_t p, uint64_t n) {
    if ((int32_t)lane == k) cp_lo = (uint32_t)p, cp_hi = (uint32_t)(p >> 32), cn_lo = (uint32_t)n, cn_hi = (uint32_t)(n >> 32);
  }
  __device__ int64_t unequal_neighbours(const uint8_t* s, int64_t n) const {
    int64_t diff = 0;
    for (int64_t base = 0; base + 1 < n; base += 64) {
      const int64_t i = base + lane;
      diff += __popcll(__ballot(i + 1 < n && s[i] != s[i + 1]));
    }
    return diff;
  }
};

// a value every lane loaded from the same address, in a scalar register
__device__ __forceinline__ int64_t gf_rp_uniform(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int32_t gf_rp_uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the read of match i inside bases[0, bases_bytes): false when its offsets point outside or it is too long
__device__ __forceinline__ bool gf_rp_read_of(const int64_t* __restrict__ offsets, int64_t i, int64_t bases_bytes, int64_t& start,
                                              int64_t& len) {
  start = gf_rp_uniform(offsets[i]);
  const int64_t end = gf_rp_uniform(offsets[i + 1]);
  len = end - start;
  return start >= 0 && end >= start && end <= bases_bytes && len <= GF_RP_MAX_LEN;
}

__global__ __launch_bounds__(GF_RP_FILTER_THREADS) void gf_rp_k_filter(const uint8_t* __restrict__ bases, int64_t bases_bytes,
                                                                        const int64_t* __restrict__ offsets,
                                                                        const gf_readmatch* __restrict__ rm, int64_t n,
                                                                        int32_t deletion_threshold, int32_t* __restrict__ reason) {
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t waves = (int64_t)gridDim.x * (GF_RP_FILTER_THREADS / 64);
  GfRpWave w(lane);
  for (int64_t i = (int64_t)blockIdx.x * (GF_RP_FILTER_THREADS / 64) + gf_rp_uniform((int32_t)(threadIdx.x >> 6)); i < n; i += waves) {
    int64_t start, len;
    int32_t why = GF_RP_BAD_READ;
    if (gf_rp_read_of(offsets, i, bases_bytes, start, len)) {
      const gf_readmatch r = rm[i];
      GfRpMatch m;
      m.read_break = gf_rp_uniform(r.read_break);
      m.left_distance = gf_rp_uniform(r.left_distance), m.right_distance = gf_rp_uniform(r.right_distance);
      m.left_position = gf_rp_uniform(r.left_position), m.right_position = gf_rp_uniform(r.right_position);
      m.left_contig = gf_rp_uniform((int32_t)r.left_contig), m.right_contig = gf_rp_uniform((int32_t)r.right_contig);
      why = gf_rp_filter_reason(w, m, bases + start, len, deletion_threshold);
    }
    if (lane == 0) reason[i] = why;
  }
}

// out[i] = {shift, left_distance, right_distance, status} (int32 x 4)
__global__ __launch_bounds__(GF_RP_ADJUST_THREADS) void gf_rp_k_adjust(const uint8_t* __restrict__ bases, int64_t bases_bytes,
                                                                        const int64_t* __restrict__ offsets,
                                                                        const gf_readmatch* __restrict__ rm,
                                                                        const int32_t* __restrict__ cluster, int64_t n,
                                                                        const uint8_t* __restrict__ refs, int64_t refs_bytes,
                                                                        const int64_t* __restrict__ ref_offsets, int64_t n_clusters,
                                                                        int32_t* __restrict__ out) {
  __shared__ GfRpSide s_sides[GF_RP_ADJUST_WAVES];
  const uint32_t lane = threadIdx.x & 63u;
  // 2 * (shift + 3) + side; through the first lane, so that the compiler knows it is the same in every lane and keeps
  // what follows from it — lengths, loop counters, the recurrence — in scalar registers
  const int32_t wave = gf_rp_uniform((int32_t)(threadIdx.x >> 6));
  GfRpWave w(lane);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    int64_t start, len;
    int32_t status = GF_RP_BAD_ROW;
    const int64_t c = gf_rp_uniform(cluster[i]);
    if (gf_rp_read_of(offsets, i, bases_bytes, start, len) && c >= 0 && c < n_clusters) {
      const bool right = wave & 1;
      // the cluster's row: left reference [l0, l1), right reference [l1, l2)
      const int64_t l0 = gf_rp_uniform(ref_offsets[2 * c]), l1 = gf_rp_uniform(ref_offsets[2 * c + 1]);
      const int64_t l2 = gf_rp_uniform(ref_offsets[2 * c + 2]);
      if (l0 >= 0 && l1 >= l0 && l2 >= l1 && l2 <= refs_bytes && l1 - l0 <= INT32_MAX && l2 - l1 <= INT32_MAX) {
        const int64_t r0 = right ? l1 : l0, r1 = right ? l2 : l1;
        const int32_t read_break = gf_rp_uniform(rm[i].read_break);
        status = GF_RP_OUT_OF_DOMAIN;
        if (gf_rp_in_domain(read_break, len)) {
          status = GF_RP_OK;
          const int32_t left_len = read_break + (wave >> 1) - 3 + 1;
          const GfRpSide side = gf_rp_calc_ed_side(w, right, bases + start, (int32_t)len, left_len, refs + r0, (int32_t)(r1 - r0));
          if (lane == 0) s_sides[wave] = side;
        }
      }
    }
    __syncthreads();  // (the sides are in LDS; status is the same in every wavefront)
    if (threadIdx.x == 0) {
      GfRpAdjust a = {0, 0, 0, status};
      if (status == GF_RP_OK) a = gf_rp_choose_shift(s_sides);
      int32_t* o = out + 4 * i;
      o[0] = a.shift, o[1] = a.left_distance, o[2] = a.right_distance, o[3] = a.status;
    }
    __syncthreads();  // (the sides are read; the next match may overwrite them)
  }
}
