// The single-end policy of SingleEndScanner::scan_single_end (src/core/sescanner.rs:183-205) for a batch of reads
// resident in HBM, around two passes of gf_map_reads_device (libgfmatch.so, public ABI):
//
//   map every read                                      gf_map_reads_device over the n reads
//   two segments in the required direction: a hit      gf_se_k_classify (status per read, retries per tile)
//   two segments, wrong direction: retry the reverse    gf_se_k_scan, gf_se_k_retry_write, gf_se_k_retry_tail,
//   complement                                          gf_map_reads_device over the retry slots
//   hits in read order, with their bases and quals      gf_se_k_final<false> (count), gf_se_k_scan,
//                                                       gf_se_k_final<true> (write), gf_se_k_totals
//
// Deterministic (two-level exclusive scans, no atomics on the outputs).  A tile is GF_SE_TILE consecutive reads,
// GF_SE_PER per thread, so that a batch of 20 M reads has 4 883 tiles and one block scans them.
#pragma once

#include "../../include/gf_single_end.h"
#include "gf_scan_common.h"

#define GF_SE_PER 16
#define GF_SE_TILE (GF_SCAN_THREADS * GF_SE_PER)

// the thread's GF_SE_PER bytes of a per-read byte array: one 16-byte load where the address allows it, 0 beyond n
__device__ __forceinline__ void gf_se_bytes16(const uint8_t* __restrict__ a, int64_t r0, int64_t n,
                                              uint8_t (&c)[GF_SE_PER]) {
  static_assert(GF_SE_PER == 16, "one uint4 per thread");
  if (r0 + GF_SE_PER <= n && (((uintptr_t)(a + r0)) & 15u) == 0) {
    const uint4 q = *(const uint4*)(a + r0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < GF_SE_PER; ++k) c[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (int k = 0; k < GF_SE_PER; ++k) c[k] = r0 + k < n ? a[r0 + k] : (uint8_t)0;
  }
}

// ---- classify: status per read (GF_SCAN_NONE / _HIT / _RETRY), retries (reads, bytes) per tile ----
// st holds GF_SE_TILE bytes per tile (zeros beyond n); too_long counts the reads whose count is GF_COUNT_TOO_LONG.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_se_k_classify(
    const uint8_t* __restrict__ counts, const gf_seqmatch* __restrict__ matches, const int64_t* __restrict__ offsets,
    int64_t n, const uint8_t* __restrict__ rev, int n_genes, uint8_t* __restrict__ st, uint32_t* __restrict__ tile_rc,
    uint32_t* __restrict__ tile_rb, unsigned long long* __restrict__ too_long) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t r0 = (int64_t)blockIdx.x * GF_SE_TILE + (int64_t)threadIdx.x * GF_SE_PER;
  uint8_t c[GF_SE_PER];
  gf_se_bytes16(counts, r0, n, c);
  int rc = 0, tl = 0;
  long long rb = 0;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < GF_SE_PER; ++k) {
    uint32_t v = GF_SCAN_NONE;
    if (c[k] == 2) {  // mapping.len() == 2: mapable (fusion_mapper.rs:107-115)
      const int64_t r = r0 + k;
      const bool fwd = gf_scan_required_direction(matches[2 * r], matches[2 * r + 1], rev, n_genes);
      v = fwd ? GF_SCAN_HIT : GF_SCAN_RETRY;
      if (!fwd) {
        rc += 1;
        rb += offsets[r + 1] - offsets[r];
      }
    } else if (c[k] == GF_COUNT_TOO_LONG && r0 + k < n) {
      tl += 1;
    }
    w[k >> 2] |= v << (8 * (k & 3));
  }
  *(uint4*)(st + r0) = make_uint4(w[0], w[1], w[2], w[3]);  // (st is whole tiles long)
  if (tl) atomicAdd(too_long, (unsigned long long)tl);
  int ea, ta; long long eb, tb;
  gf_scan_block_scan2(rc, rb, s_a, s_b, ea, eb, ta, tb);
  if (threadIdx.x == 0) {
    tile_rc[blockIdx.x] = (uint32_t)ta;
    tile_rb[blockIdx.x] = (uint32_t)tb;
  }
}

// ---- exclusive scan of per-tile totals: block b scans job b (the scans come in pairs: reads and bytes) ----
// (gf_scan_totals_block.)  A batch of 20 M reads has 4 883 tiles: five totals per thread.
struct GfSeScanJobs { GfScanJob j[2]; };

__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_se_k_scan(GfSeScanJobs jobs, int64_t ntiles) {
  const GfScanJob& j = jobs.j[blockIdx.x];
  const long long total = gf_scan_totals_block(j.tile_counts, j.tile_offsets, ntiles);
  if (threadIdx.x == 0) *j.d_total = total;
}

// ---- retry_write: the reverse complements of the retried reads, back to back, in read order ----
// r_off[k] = where retry k starts.  A retry beyond the capacities is not written (gf_se_k_retry_tail then empties the
// whole retry pass and raises the overflow bit).
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_se_k_retry_write(
    const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, const int64_t* __restrict__ offsets, int64_t n,
    const uint8_t* __restrict__ st, const int64_t* __restrict__ tile_off_rc, const int64_t* __restrict__ tile_off_rb,
    int64_t cap_reads, int64_t cap_bytes, int64_t* __restrict__ r_off, uint8_t* __restrict__ r_bases,
    uint8_t* __restrict__ r_quals) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t r0 = (int64_t)blockIdx.x * GF_SE_TILE + (int64_t)threadIdx.x * GF_SE_PER;
  uint8_t v[GF_SE_PER];
  gf_se_bytes16(st, r0, n, v);
  int rc = 0;
  long long rb = 0;
#pragma unroll
  for (int k = 0; k < GF_SE_PER; ++k)
    if (v[k] == GF_SCAN_RETRY) {
      rc += 1;
      rb += offsets[r0 + k + 1] - offsets[r0 + k];
    }
  int ea, ta; long long eb, tb;
  gf_scan_block_scan2(rc, rb, s_a, s_b, ea, eb, ta, tb);
  if (__ballot(rc != 0) == 0) return;  // (whole wavefronts: the reads are written by all 64 lanes)
  int64_t k_out = tile_off_rc[blockIdx.x] + ea;
  int64_t b_out = tile_off_rb[blockIdx.x] + eb;
#pragma unroll 1
  for (int k = 0; k < GF_SE_PER; ++k) {
    const bool mine = v[k] == GF_SCAN_RETRY;
    const uint8_t* b = nullptr;
    const uint8_t* q = nullptr;
    int len = 0;
    bool fits = false;
    if (mine) {
      const int64_t o = offsets[r0 + k];
      len = (int)(offsets[r0 + k + 1] - o);
      b = bases + o;
      q = quals + o;
      fits = k_out < cap_reads && b_out + len <= cap_bytes;
      if (fits) r_off[k_out] = b_out;
    }
    gf_scan_wave_write(__ballot(fits), b, q, len, (long long)b_out, r_bases, r_quals, true);
    if (mine) {
      k_out += 1;
      b_out += len;
    }
  }
}

// the unused retry slots emptied, the overflow bit (gf_scan_common.h)
__global__ void gf_se_k_retry_tail(const int64_t* __restrict__ d_n_retry, const int64_t* __restrict__ d_retry_bytes,
                                   int64_t cap_reads, int64_t cap_bytes, int64_t* __restrict__ r_off,
                                   int64_t* __restrict__ totals) {
  gf_scan_retry_tail(d_n_retry, d_retry_bytes, cap_reads, cap_bytes, r_off, totals,
                     (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// ---- final: the hits of the batch in read order.  WRITE = false: hits and their bytes per tile; true: the records,
// bases and qualities.  A retry's slot is its place among the retries: the tile's offset (the scan of the classify
// counts) plus the thread's exclusive prefix of them.
struct GfSeFinalIn {
  const uint8_t *bases, *quals;
  const int64_t* offsets;
  const gf_seqmatch* m1;         // first pass, gf_seqmatch[2n]
  const uint8_t* st;
  const int64_t* tile_off_rc;    // retries before each tile
  const uint8_t* cR;             // retry pass: counts and matches of the retry slots
  const gf_seqmatch* mR;
  const int64_t *r_off;
  const uint8_t *r_bases, *r_quals;
  int64_t cap_reads;
  const uint8_t* rev;
  int n_genes;
};

template <bool WRITE>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_se_k_final(
    GfSeFinalIn F, int64_t n, int64_t read_id_base, uint32_t* __restrict__ tile_hc, uint32_t* __restrict__ tile_hb,
    const int64_t* __restrict__ tile_off_hc, const int64_t* __restrict__ tile_off_hb, gf_pair_hit* __restrict__ hits,
    int64_t hits_cap, uint8_t* __restrict__ out_bases, uint8_t* __restrict__ out_quals, int64_t bytes_cap) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t r0 = (int64_t)blockIdx.x * GF_SE_TILE + (int64_t)threadIdx.x * GF_SE_PER;
  uint8_t v[GF_SE_PER];
  gf_se_bytes16(F.st, r0, n, v);
  int rc = 0;
#pragma unroll
  for (int k = 0; k < GF_SE_PER; ++k) rc += v[k] == GF_SCAN_RETRY;
  int er, tr; long long e0, t0;
  gf_scan_block_scan2(rc, 0, s_a, s_b, er, e0, tr, t0);
  // slot[k] >= 0: the hit is on the reverse complement in retry slot slot[k]; hit bit k: read r0 + k is a hit
  int64_t slot0 = F.tile_off_rc[blockIdx.x] + er;
  uint32_t hit = 0, on_rc = 0;
  int hc = 0;
  long long hb = 0;
#pragma unroll
  for (int k = 0; k < GF_SE_PER; ++k) {
    bool h = v[k] == GF_SCAN_HIT;
    if (v[k] == GF_SCAN_RETRY) {
      const int64_t s = slot0++;
      if (s < F.cap_reads && F.cR[s] == 2 &&
          gf_scan_required_direction(F.mR[2 * s], F.mR[2 * s + 1], F.rev, F.n_genes)) {
        h = true;
        on_rc |= 1u << k;
      }
    }
    if (h) {
      hit |= 1u << k;
      hc += 1;
      hb += F.offsets[r0 + k + 1] - F.offsets[r0 + k];
    }
  }
  int ea, ta; long long eb, tb;
  gf_scan_block_scan2(hc, hb, s_a, s_b, ea, eb, ta, tb);
  if (!WRITE) {
    if (threadIdx.x == 0) {
      tile_hc[blockIdx.x] = (uint32_t)ta;
      tile_hb[blockIdx.x] = (uint32_t)tb;
    }
    return;
  }
  if (__ballot(hc != 0) == 0) return;  // (whole wavefronts: the reads are written by all 64 lanes)
  int64_t k_out = tile_off_hc[blockIdx.x] + ea;
  int64_t b_out = tile_off_hb[blockIdx.x] + eb;
  int64_t slot = F.tile_off_rc[blockIdx.x] + er;
#pragma unroll 1
  for (int k = 0; k < GF_SE_PER; ++k) {
    const bool mine = (hit >> k) & 1u;
    const bool rcm = (on_rc >> k) & 1u;
    const int64_t my_slot = slot;
    if (v[k] == GF_SCAN_RETRY) slot += 1;
    const uint8_t* b = nullptr;
    const uint8_t* q = nullptr;
    int len = 0;
    bool bytes_fit = false;
    if (mine) {
      const int64_t r = r0 + k;
      const int64_t o = F.offsets[r];
      len = (int)(F.offsets[r + 1] - o);
      const gf_seqmatch* m = F.m1 + 2 * r;
      b = F.bases + o;
      q = F.quals + o;
      if (rcm) {  // the hit is on the reverse complement: its bases, its qualities, its mapping
        b = F.r_bases + F.r_off[my_slot];
        q = F.r_quals + F.r_off[my_slot];
        m = F.mR + 2 * my_slot;
      }
      if (k_out < hits_cap) {
        gf_pair_hit h;
        h.pair_id = read_id_base + r;
        h.source = 1;
        // bit 0: found on the reverse complement; bit 1: ReadMatch.m_reversed (set_reversed(true), sescanner.rs:193)
        h.flags = rcm ? 3 : 0;
        h.read_len = len;
        h.merge_diff = 0;
        h.seq_offset = b_out;
        h.m[0] = m[0];
        h.m[1] = m[1];
        hits[k_out] = h;
      }
      bytes_fit = b_out + len <= bytes_cap;
    }
    gf_scan_wave_write(__ballot(bytes_fit), b, q, len, (long long)b_out, out_bases, out_quals, false);
    if (mine) {
      k_out += 1;
      b_out += len;
    }
  }
}

// totals: [0] hits, [1] hit bytes, [2] 0, [3] retries (gf_se_k_retry_tail), [4] overflow bits, [5] too-long reads
__global__ void gf_se_k_totals(const int64_t* __restrict__ d_hits, const int64_t* __restrict__ d_hit_bytes,
                               const unsigned long long* __restrict__ too_long, int64_t hits_cap, int64_t bytes_cap,
                               int64_t* __restrict__ totals) {
  totals[0] = *d_hits;
  totals[1] = *d_hit_bytes;
  totals[5] = (int64_t)*too_long;
  if (*d_hits > hits_cap || *d_hit_bytes > bytes_cap) totals[4] |= 2;
}
