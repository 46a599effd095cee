// The paired-end policy of PairEndScanner::scan_pair_end (src/core/pescanner.rs:427-518) cut in two for multi-CSV
// mode (fusion_scan.rs:62-188), around libgfmatch.so's public ABI:
//
//   ONCE per read set (gf_mc_pairs_prepare_device)
//   merged = pair.fast_merge()                          gf_fast_merge_find_device
//   the reads a scan maps, in two contiguous lists      gf_mc_k_tile_counts, gf_mc_k_scan, gf_mc_k_gather,
//   (R1, R2 of the unmerged pairs | the merged reads)   gf_mc_k_list_tail, gf_fast_merge_write_device
//   their packed form                                   gf_pack_bases_device
//
//   ONCE per index (gf_mc_pairs_scan_device)
//   map both lists                                      gf_map_reads_packed_device x 2
//   two segments in the required direction: a hit;      gf_mc_k_classify
//   two segments, wrong direction: retry the reverse    gf_mc_k_scan, gf_mc_k_retry_write, gf_mc_k_retry_tail,
//   complement                                          gf_map_reads_device over the retry slots
//   hits in push order (pair, then merged | R1, R2)     gf_mc_k_final<false> (count), gf_mc_k_scan,
//                                                       gf_mc_k_final<true> (write), gf_mc_k_totals
//
// Deterministic (two-level exclusive scans, no atomics).  A tile is GF_MC_TILE consecutive pairs, one per thread, so
// that a wavefront reads and writes consecutive pairs.
#pragma once

#include "../../include/gf_multi_csv.h"
#include "gf_scan_common.h"

#define GF_MC_TILE GF_SCAN_THREADS
#define GF_MC_SCAN_JOBS 4

// ---- exclusive scan of per-tile totals: block b scans job b ----
// (gf_scan_totals_block.)  10 M pairs are 39 063 tiles: 39 totals per thread.
struct GfMcScanJobs { GfScanJob j[GF_MC_SCAN_JOBS]; };

__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_mc_k_scan(GfMcScanJobs jobs, int64_t ntiles) {
  const GfScanJob& j = jobs.j[blockIdx.x];
  const long long total = gf_scan_totals_block(j.tile_counts, j.tile_offsets, ntiles);
  if (threadIdx.x == 0) *j.d_total = total;
}

// ======================================= the CSV-independent half =======================================

// What a tile's pairs put into the two lists.  tc: four uint32 arrays of ntiles — unmerged pairs, the bytes of their
// R1 + R2, merged pairs, the bytes of their merged reads.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_mc_k_tile_counts(
    const int32_t* __restrict__ m_len, const int64_t* __restrict__ l_off, const int64_t* __restrict__ r_off, int64_t n,
    uint32_t* __restrict__ tc_uc, uint32_t* __restrict__ tc_ub, uint32_t* __restrict__ tc_mc,
    uint32_t* __restrict__ tc_mb) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t p = (int64_t)blockIdx.x * GF_MC_TILE + threadIdx.x;
  const int ml = p < n ? m_len[p] : 0;
  const bool un = p < n && ml <= 0;
  long long ub = 0;
  if (un) ub = (l_off[p + 1] - l_off[p]) + (r_off[p + 1] - r_off[p]);
  int e, tu, tm; long long eb, tub, tmb;
  gf_scan_block_scan2(un ? 1 : 0, ub, s_a, s_b, e, eb, tu, tub);
  gf_scan_block_scan2(ml > 0 ? 1 : 0, ml > 0 ? ml : 0, s_a, s_b, e, eb, tm, tmb);
  if (threadIdx.x == 0) {
    tc_uc[blockIdx.x] = (uint32_t)tu;
    tc_ub[blockIdx.x] = (uint32_t)tub;
    tc_mc[blockIdx.x] = (uint32_t)tm;
    tc_mb[blockIdx.x] = (uint32_t)tmb;
  }
}

// Per pair: its place in its list (rank: among the merged pairs, or among the unmerged ones — the unmerged pair of
// rank k owns reads 2k (R1) and 2k + 1 (R2) of the unmerged list) and, merged, where its read goes (m_pos: what
// gf_fast_merge_write_device takes as d_out_pos).  The lists' offsets.  And the scatter of the tile's unmerged
// reads: the unmerged list lies at bytes [0, ub) of `out`, the merged one behind it at [ub, ub + mb), so that one
// packed stream serves both.  A tile's reads are one contiguous range of `out`; a lane takes one aligned 16-byte
// chunk of that range at a time, finds the read it starts in by a binary search over the tile's (at most 512) starts
// in LDS, and where the whole chunk lies inside one read — all but two chunks per read — moves it with one 16-byte
// load and one aligned 16-byte store; the chunks across a read boundary, and the range's ragged ends, go byte by byte.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_mc_k_gather(
    const uint8_t* __restrict__ l_bases, const int64_t* __restrict__ l_off, const uint8_t* __restrict__ r_bases,
    const int64_t* __restrict__ r_off, const int32_t* __restrict__ m_len, int64_t n,
    const int64_t* __restrict__ to_uc, const int64_t* __restrict__ to_ub, const int64_t* __restrict__ to_mc,
    const int64_t* __restrict__ to_mb, const int64_t* __restrict__ d_ub_total, int32_t* __restrict__ rank,
    int64_t* __restrict__ u_off, int64_t* __restrict__ m_off, int64_t* __restrict__ m_pos, uint8_t* __restrict__ out) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  __shared__ uint32_t s_rel[2 * GF_MC_TILE + 1];        // start of the tile's unmerged read j within the tile's bytes
  __shared__ const uint8_t* s_src[2 * GF_MC_TILE];      // where it comes from
  const int tid = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * GF_MC_TILE + tid;
  const int ml = p < n ? m_len[p] : 0;
  const bool un = p < n && ml <= 0;
  int64_t lo = 0, ro = 0;
  int len1 = 0, len2 = 0;
  if (un) {
    lo = l_off[p]; len1 = (int)(l_off[p + 1] - lo);
    ro = r_off[p]; len2 = (int)(r_off[p + 1] - ro);
  }
  int eu, tu, em, tm; long long ebu, tbu, ebm, tbm;
  gf_scan_block_scan2(un ? 1 : 0, (long long)len1 + len2, s_a, s_b, eu, ebu, tu, tbu);
  gf_scan_block_scan2(ml > 0 ? 1 : 0, ml > 0 ? ml : 0, s_a, s_b, em, ebm, tm, tbm);
  const int64_t U = to_uc[blockIdx.x], UB = to_ub[blockIdx.x];
  if (un) {
    const int64_t k = U + eu;
    rank[p] = (int32_t)k;
    *(longlong2*)(u_off + 2 * k) = make_longlong2(UB + ebu, UB + ebu + len1);  // (u_off is 16-byte aligned)
    s_rel[2 * eu] = (uint32_t)ebu;
    s_rel[2 * eu + 1] = (uint32_t)(ebu + len1);
    s_src[2 * eu] = l_bases + lo;
    s_src[2 * eu + 1] = r_bases + ro;
  } else if (p < n) {
    const int64_t k = to_mc[blockIdx.x] + em;
    const int64_t pos = *d_ub_total + to_mb[blockIdx.x] + ebm;
    rank[p] = (int32_t)k;
    m_off[k] = pos;
    m_pos[p] = pos;
  }
  if (tid == 0) s_rel[2 * tu] = (uint32_t)tbu;
  __syncthreads();
  if (tbu == 0) return;
  const int nslots = 2 * tu;
  const int64_t D0 = UB, D1 = UB + tbu;
  for (int64_t c = (D0 >> 4) + tid; c < ((D1 + 15) >> 4); c += GF_SCAN_THREADS) {
    const int64_t b0 = c * 16 > D0 ? c * 16 : D0;
    const int64_t b1 = c * 16 + 16 < D1 ? c * 16 + 16 : D1;
    const uint32_t rel = (uint32_t)(b0 - D0);
    int a = 0, b = nslots;  // s_rel[a] <= rel < s_rel[b]
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (s_rel[mid] <= rel) a = mid; else b = mid;
    }
    int j = a;
    if (b1 - b0 == 16 && rel + 16 <= s_rel[j + 1]) {
      uint4 v;
      __builtin_memcpy(&v, s_src[j] + (rel - s_rel[j]), 16);  // (16 bytes inside the read, at any alignment)
      *(uint4*)(out + b0) = v;
    } else {
      for (int64_t d = b0; d < b1; ++d) {
        const uint32_t x = (uint32_t)(d - D0);
        while (x >= s_rel[j + 1]) ++j;  // (x < s_rel[nslots]: ends; empty reads are stepped over)
        out[d] = s_src[j][x - s_rel[j]];
      }
    }
  }
}

// the empty reads behind the real ones of both lists, and the closing offsets
__global__ void gf_mc_k_list_tail(const int64_t* __restrict__ hdr, int64_t n, int64_t* __restrict__ u_off,
                                  int64_t* __restrict__ m_off) {
  const int64_t nu = hdr[0], ub = hdr[1], nm = hdr[2], mb = hdr[3];
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = 2 * nu + i0; k <= 2 * n; k += step) u_off[k] = ub;
  for (int64_t k = nm + i0; k <= n; k += step) m_off[k] = ub + mb;
}

// ========================================= the per-index half =========================================

struct GfMcIn {
  const uint8_t *l_bases, *l_quals, *r_bases, *r_quals;
  const int64_t *l_off, *r_off;
  const uint8_t* p_bases;   // the prepared lists' bases (merged read of pair p at m_pos[p])
  const uint8_t* p_mquals;  // the merged reads' qualities, at the same positions
  const int32_t *m_len, *m_diff, *rank;
  const int64_t* m_pos;
  const uint8_t *cU, *cM;   // counts of the two mapping passes: unmerged list (2n slots), merged list (n slots)
  const gf_seqmatch *mU, *mM;
  const uint8_t* rev;       // Fusion::is_reversed() per gene; null = all false
  int n_genes;
};

// candidate s of pair p: 0 = merged read, 1 = R1, 2 = R2
__device__ __forceinline__ void gf_mc_candidate(const GfMcIn& P, int64_t p, int s, const uint8_t*& bases,
                                                const uint8_t*& quals, int32_t& len, uint8_t& cnt,
                                                const gf_seqmatch*& m) {
  const int64_t k = P.rank[p];
  if (s == 0) {
    const int64_t o = P.m_pos[p];
    bases = P.p_bases + o; quals = P.p_mquals + o; len = P.m_len[p]; cnt = P.cM[k]; m = P.mM + 2 * k;
  } else if (s == 1) {
    const int64_t o = P.l_off[p];
    bases = P.l_bases + o; quals = P.l_quals + o; len = (int32_t)(P.l_off[p + 1] - o); cnt = P.cU[2 * k]; m = P.mU + 4 * k;
  } else {
    const int64_t o = P.r_off[p];
    bases = P.r_bases + o; quals = P.r_quals + o; len = (int32_t)(P.r_off[p + 1] - o); cnt = P.cU[2 * k + 1];
    m = P.mU + 4 * k + 2;
  }
}

__device__ __forceinline__ uint32_t gf_mc_status(const GfMcIn& P, int64_t p, int s, int32_t& len) {
  const uint8_t* b; const uint8_t* q; uint8_t cnt; const gf_seqmatch* m;
  gf_mc_candidate(P, p, s, b, q, len, cnt, m);
  if (cnt != 2) return GF_SCAN_NONE;  // mapping.len() < 2: not mapable (fusion_mapper.rs:107-115)
  return gf_scan_required_direction(m[0], m[1], P.rev, P.n_genes) ? GF_SCAN_HIT : GF_SCAN_RETRY;
}

// ---- classify: which candidates matched as they are, which are searched again reversed ----
// st[3p + s]; tile_rc / tile_rb: retries (reads / bytes) per tile.
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_mc_k_classify(GfMcIn P, int64_t n, uint8_t* __restrict__ st,
                                                                  uint32_t* __restrict__ tile_rc,
                                                                  uint32_t* __restrict__ tile_rb) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t p = (int64_t)blockIdx.x * GF_MC_TILE + threadIdx.x;
  int rc = 0;
  long long rb = 0;
  if (p < n) {
    const bool is_merged = P.m_len[p] > 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      uint32_t v = GF_SCAN_NONE;
      int32_t len = 0;
      if (is_merged ? s == 0 : s != 0) v = gf_mc_status(P, p, s, len);
      st[3 * p + s] = (uint8_t)v;
      if (v == GF_SCAN_RETRY) { rc += 1; rb += len; }
    }
  }
  int ea, ta; long long eb, tb;
  gf_scan_block_scan2(rc, rb, s_a, s_b, ea, eb, ta, tb);
  if (threadIdx.x == 0) {
    tile_rc[blockIdx.x] = (uint32_t)ta;
    tile_rb[blockIdx.x] = (uint32_t)tb;
  }
}

// ---- retry_write: the reverse complements of the retried reads, back to back, in candidate order ----
// slot_of[3p + s] = index of the candidate in the retry batch, -1 for one beyond the capacities (gf_mc_k_retry_tail
// then empties the whole retry pass and raises the overflow bit).
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_mc_k_retry_write(
    GfMcIn P, int64_t n, const uint8_t* __restrict__ st, const int64_t* __restrict__ tile_off_rc,
    const int64_t* __restrict__ tile_off_rb, int64_t cap_reads, int64_t cap_bytes, int64_t* __restrict__ r_off,
    uint8_t* __restrict__ r_bases, uint8_t* __restrict__ r_quals, int32_t* __restrict__ slot_of) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t p = (int64_t)blockIdx.x * GF_MC_TILE + threadIdx.x;
  int rc = 0;
  long long rb = 0;
  if (p < n) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (st[3 * p + s] == GF_SCAN_RETRY) {
        const uint8_t* b; const uint8_t* q; int32_t len; uint8_t cnt; const gf_seqmatch* m;
        gf_mc_candidate(P, p, s, b, q, len, cnt, m);
        rc += 1;
        rb += len;
      }
  }
  int ea, ta; long long eb, tb;
  gf_scan_block_scan2(rc, rb, s_a, s_b, ea, eb, ta, tb);
  if (__ballot(rc != 0) == 0) return;  // (whole wavefronts: the reads are written by all 64 lanes)
  int64_t k_out = tile_off_rc[blockIdx.x] + ea;
  int64_t b_out = tile_off_rb[blockIdx.x] + eb;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const bool mine = p < n && st[3 * p + s] == GF_SCAN_RETRY;
    const uint8_t* b = nullptr; const uint8_t* q = nullptr; int32_t len = 0; uint8_t cnt; const gf_seqmatch* m;
    bool fits = false;
    if (mine) {
      gf_mc_candidate(P, p, s, b, q, len, cnt, m);
      fits = k_out < cap_reads && b_out + len <= cap_bytes;
      slot_of[3 * p + s] = fits ? (int32_t)k_out : -1;
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
__global__ void gf_mc_k_retry_tail(const int64_t* __restrict__ d_n_retry, const int64_t* __restrict__ d_retry_bytes,
                                   int64_t cap_reads, int64_t cap_bytes, int64_t* __restrict__ r_off,
                                   int64_t* __restrict__ totals) {
  gf_scan_retry_tail(d_n_retry, d_retry_bytes, cap_reads, cap_bytes, r_off, totals,
                     (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// ---- final: the matches of the pairs, in the reference's push order.  WRITE = false: hits and their bytes per
// tile; true: the records, bases and qualities. ----
struct GfMcFinalIn {
  const uint8_t* st;
  const int32_t* slot_of;
  const uint8_t* cR;        // retry pass: counts and matches of the retry slots
  const gf_seqmatch* mR;
  const int64_t* r_off;
  const uint8_t *r_bases, *r_quals;
};

// is candidate s of pair p a hit?  rc_slot >= 0: on the reverse complement in that retry slot
__device__ __forceinline__ bool gf_mc_is_hit(const GfMcIn& P, const GfMcFinalIn& F, int64_t p, int s, int& rc_slot) {
  const uint8_t v = F.st[3 * p + s];
  rc_slot = -1;
  if (v == GF_SCAN_HIT) return true;
  if (v != GF_SCAN_RETRY) return false;
  const int32_t k = F.slot_of[3 * p + s];
  if (k < 0 || F.cR[k] != 2) return false;
  if (!gf_scan_required_direction(F.mR[2 * (int64_t)k], F.mR[2 * (int64_t)k + 1], P.rev, P.n_genes)) return false;
  rc_slot = k;
  return true;
}

template <bool WRITE>
__global__ __launch_bounds__(GF_SCAN_THREADS) void gf_mc_k_final(
    GfMcIn P, GfMcFinalIn F, int64_t n, int64_t pair_id_base, uint32_t* __restrict__ tile_hc,
    uint32_t* __restrict__ tile_hb, const int64_t* __restrict__ tile_off_hc, const int64_t* __restrict__ tile_off_hb,
    gf_pair_hit* __restrict__ hits, int64_t hits_cap, uint8_t* __restrict__ out_bases, uint8_t* __restrict__ out_quals,
    int64_t bytes_cap) {
  __shared__ int s_a[GF_SCAN_THREADS / 64];
  __shared__ long long s_b[GF_SCAN_THREADS / 64];
  const int64_t p = (int64_t)blockIdx.x * GF_MC_TILE + threadIdx.x;
  int hc = 0;
  long long hb = 0;
  int slot[3] = {-1, -1, -1};
  uint32_t hit = 0;
  if (p < n) {
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (F.st[3 * p + s] == GF_SCAN_NONE) continue;
      if (gf_mc_is_hit(P, F, p, s, slot[s])) {
        const uint8_t* b; const uint8_t* q; int32_t len; uint8_t cnt; const gf_seqmatch* m;
        gf_mc_candidate(P, p, s, b, q, len, cnt, m);
        hit |= 1u << s;
        hc += 1;
        hb += len;
      }
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
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const bool mine = (hit >> s) & 1u;
    const uint8_t* b = nullptr; const uint8_t* q = nullptr; int32_t len = 0; uint8_t cnt; const gf_seqmatch* m;
    bool bytes_fit = false;
    if (mine) {
      gf_mc_candidate(P, p, s, b, q, len, cnt, m);
      if (slot[s] >= 0) {  // the match is on the reverse complement: its bases, its qualities, its mapping
        b = F.r_bases + F.r_off[slot[s]];
        q = F.r_quals + F.r_off[slot[s]];
        m = F.mR + 2 * (int64_t)slot[s];
      }
      if (k_out < hits_cap) {
        gf_pair_hit h;
        h.pair_id = pair_id_base + p;
        h.source = s;
        // bit 0: found on the reverse complement; bit 1: ReadMatch.m_reversed as the reference sets it — for R1 / R2
        // (pescanner.rs:489,:511), not for a merged read (:465-468)
        h.flags = (slot[s] >= 0 ? 1 : 0) | ((slot[s] >= 0 && s != 0) ? 2 : 0);
        h.read_len = len;
        h.merge_diff = s == 0 ? P.m_diff[p] : 0;
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

// totals: [0] hits, [1] hit bytes, [2] merged pairs, [3] retries (gf_mc_k_retry_tail), [4] overflow bits
__global__ void gf_mc_k_totals(const int64_t* __restrict__ d_hits, const int64_t* __restrict__ d_hit_bytes,
                               const int64_t* __restrict__ n_merged, int64_t hits_cap, int64_t bytes_cap,
                               int64_t* __restrict__ totals) {
  totals[0] = *d_hits;
  totals[1] = *d_hit_bytes;
  totals[2] = *n_merged;
  if (*d_hits > hits_cap || *d_hit_bytes > bytes_cap) totals[4] |= 2;
}
