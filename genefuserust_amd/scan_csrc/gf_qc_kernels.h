// The read QC of libgfqc.so (include/gf_read_qc.h) over records in HBM, two kernels that only read the records:
//
//   stats    one side's table: length_hist and the 513 x 8 per-cycle counts      gf_qc_k_stats  (a wavefront a record,
//                                                                                  a byte a lane)
//   insert   the pairs' insert histogram: I* by the overlap walk of gf_at_core.h  gf_qc_k_insert (G lanes a pair, the
//                                                                                  packing of gf_at_kernels.h)
//
// Stats reads two bytes per base and writes 37 KB per call, so what could ruin it is an atomic per base: qualities and
// bases cluster on a few values and reads on one length, and the lanes of a wavefront would queue on one address.
// There is none.  A wavefront walks its records with lane = cycle mod 64 (gf_qc_core.h: gf_qc_lane_record is this
// kernel's walk for one lane): 64 consecutive bytes of bases and of qualities per load, every lane a cycle of its own.
// A lane keeps the 8 columns of its 8 cycles below 512, and of the tail row, in registers across all the records of
// its wavefront; the base classes are counted by compares (v_cmp and an add of the carry), never by an indexed
// register, so the accumulators stay registers.  The wavefront's records are strided by the launch's wavefronts
// (GF_QC_GRID blocks at the most), its record index is made scalar, and so the offsets are scalar loads and the
// per-record branches scalar branches; the bytes of a record's full rounds are all loaded before the first is counted
// (its last, partial round after them: asking for the next record's offsets ahead, or folding that round in, cost a
// spill to scratch at three wavefronts a SIMD, so neither is done).  At its end a wavefront adds its counts that are not 0 into the block's table
// in LDS (64-bit, 37 KB; the registers allow three blocks a CU, and GF_QC_GRID is three a CU), and the block adds the table's words that are not 0 to the caller's with
// one global atomic each.  length_hist gets one LDS add per record, by one lane.
//
// The 32-bit accumulators cannot overflow for any n: a wavefront flushes them into LDS after every
// GF_QC_FLUSH_RECORDS records (gf_qc_core.h has the bound: 222 * 2^20 < 2^28); no n is refused for it.  The flush is
// the wavefront's own, LDS atomics and no barrier, so wavefronts of a block need not take the same number of records.
//
// Insert takes a pair per group of G = 16 lanes exactly as gf_at_k_decide does: planes zeroed, a packed forwards, b
// as its reverse complement, then a lane an insert, in rounds of G from the largest downwards; only the group's
// maximum leaves the walk, as one LDS add into the block's histogram.  The groups are strided by the launch's groups.
//
// Deterministic: every atomic is an integer sum.
#pragma once

#include "gf_at_kernels.h"
#include "gf_qc_core.h"

#define GF_QC_GRID 768                           // blocks of a launch, at the most: three a CU, all resident
#define GF_QC_BLOCK_WAVES (GF_SCAN_THREADS / 64)  // wavefronts of a block: a launch has at most GF_QC_GRID times this

// ---- stats: wavefront w of the launch takes the records w, w + W, .. (W the launch's wavefronts) of one side and adds
// them to table[GF_QC_SIDE_WORDS].
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_qc_k_stats(const uint8_t* __restrict__ bases,
                                                                 const uint8_t* __restrict__ quals,
                                                                 const int64_t* __restrict__ off, int64_t n,
                                                                 unsigned long long* __restrict__ table) {
  __shared__ unsigned long long s_table[GF_QC_SIDE_WORDS];
  for (int k = threadIdx.x; k < GF_QC_SIDE_WORDS; k += GF_SCAN_THREADS) s_table[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GF_QC_BLOCK_WAVES + (threadIdx.x >> 6)));
  const int64_t waves = (int64_t)gridDim.x * GF_QC_BLOCK_WAVES;
  uint32_t acc[GF_QC_LANE_CYCLES][GF_QC_COLUMNS] = {};
  uint64_t tail[GF_QC_COLUMNS] = {};
  // (the halves of a word apart, the carry by hand: a 64-bit add would make every accumulator a register pair)
  uint32_t* const s_half = reinterpret_cast<uint32_t*>(s_table);
  const auto into_lds = [&](int word, uint64_t v) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    const uint32_t carry = lo ? (uint32_t)(atomicAdd(&s_half[2 * word], lo) + lo < lo) : 0u;
    if (hi + carry) atomicAdd(&s_half[2 * word + 1], hi + carry);
  };
  int taken = 0;
  for (int64_t i = wave; i < n; i += waves) {
    const int64_t start = off[i];
    const int64_t L = gf_qc_length(start, off[i + 1]);
    if (lane == 0) atomicAdd(&s_table[gf_qc_length_entry(L)], 1ull);
    const uint8_t* __restrict__ b = bases + start;
    const uint8_t* __restrict__ q = quals + start;
    gf_qc_lane_record([&](int64_t pos) { return (uint32_t)b[pos]; }, [&](int64_t pos) { return (uint32_t)q[pos]; }, L,
                      lane, acc, tail);
    if (++taken == GF_QC_FLUSH_RECORDS) {
      gf_qc_lane_flush(lane, acc, tail, into_lds);
      taken = 0;
    }
  }
  gf_qc_lane_flush(lane, acc, tail, into_lds);
  __syncthreads();
  for (int k = threadIdx.x; k < GF_QC_SIDE_WORDS; k += GF_SCAN_THREADS)
    if (s_table[k]) atomicAdd(&table[k], s_table[k]);
}

// ---- insert: group g of the launch takes the pairs g, g + GROUPS, .. and adds them to hist[GF_QC_INSERT_WORDS].
template <int G>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_qc_k_insert(const uint8_t* __restrict__ l_bases,
                                                                  const int64_t* __restrict__ l_off,
                                                                  const uint8_t* __restrict__ r_bases,
                                                                  const int64_t* __restrict__ r_off, int64_t n,
                                                                  unsigned long long* __restrict__ hist) {
  constexpr int GROUPS = GF_SCAN_THREADS / G;
  __shared__ uint32_t s_planes[GROUPS][2][GF_AT_READ_WORDS];
  __shared__ unsigned long long s_hist[GF_QC_INSERT_WORDS];
  for (int k = threadIdx.x; k < GF_QC_INSERT_WORDS; k += GF_SCAN_THREADS) s_hist[k] = 0;
  __syncthreads();
  const int g = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const gf_at_settings s = gf_qc_insert_settings();
  uint32_t* const s_a = s_planes[g][0];
  uint32_t* const s_r = s_planes[g][1];
  for (int64_t i = (int64_t)blockIdx.x * GROUPS + g; i < n; i += (int64_t)gridDim.x * GROUPS) {
    const int64_t start_l = l_off[i], len_l = l_off[i + 1] - start_l;
    const int64_t start_r = r_off[i], len_r = r_off[i + 1] - start_r;
    int entry = GF_QC_INSERT_UNMEASURED;
    if (gf_qc_measured(len_l) && gf_qc_measured(len_r)) {
      const int32_t L1 = (int32_t)len_l, L2 = (int32_t)len_r;
      gf_at_group_sync();  // (the pair before this one has been read to its end)
      gf_at_zero_group<G>(s_a);
      gf_at_zero_group<G>(s_r);
      gf_at_group_sync();
      gf_at_pack_group<G>(l_bases + start_l, L1, false, s_a);
      gf_at_pack_group<G>(r_bases + start_r, L2, true, s_r);
      gf_at_group_sync();
      const int32_t first = gf_at_first_insert(s);
      int32_t insert = -1;
      for (int32_t top = gf_at_last_insert(L1, L2, s); top >= first; top -= G) {
        const int32_t I = top - gl;
        const bool ok = I >= first && gf_at_try_insert(s_a, s_r, L1, L2, I, s);
        insert = gf_at_group_max<G>(ok ? I : -1);
        if (insert >= 0) break;
      }
      entry = gf_qc_insert_entry(insert);
    }
    if (gl == 0) atomicAdd(&s_hist[entry], 1ull);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < GF_QC_INSERT_WORDS; k += GF_SCAN_THREADS)
    if (s_hist[k]) atomicAdd(&hist[k], s_hist[k]);
}
