// libgfse.so: the single-end scan (include/gf_single_end.h) on top of libgfmatch.so's public ABI.
#include "gf_se_kernels.h"
#include "gf_scan_host.h"

namespace {

// The workspace (scalar [4] of the retry part: the too-long reads).
struct Layout {
  int64_t n = 0, ntiles = 0;
  size_t o_cnt = 0, o_st = 0, o_m1 = 0, o_tc = 0, o_to = 0;
  RetryWork retry;
  size_t bytes = 0;
};

int64_t resolve_retry_cap(int64_t n, int64_t retry_cap) {
  const int64_t r = retry_cap <= 0 ? gf_se_retry_capacity(n) : retry_cap;
  return std::min(r, n);  // (no more retries than reads)
}

Layout layout(int64_t n, int32_t max_read_len, int64_t retry_cap) {
  Layout L;
  L.n = n;
  L.ntiles = (n + GF_SE_TILE - 1) / GF_SE_TILE;
  size_t off = 0;
  L.o_cnt = take(off, (size_t)n);                                 // first pass: counts
  L.o_st = take(off, (size_t)L.ntiles * GF_SE_TILE);              // status per read, whole tiles
  L.o_m1 = take(off, (size_t)n * 2 * sizeof(gf_seqmatch));        // first pass: matches
  L.o_tc = take(off, (size_t)L.ntiles * 2 * sizeof(uint32_t));    // two uint32 per tile: reads, bytes
  L.o_to = take(off, (size_t)L.ntiles * 4 * sizeof(int64_t));     // their offsets: retries (2), hits (2)
  const int64_t R = resolve_retry_cap(n, retry_cap);
  L.retry.carve(off, R, R * (int64_t)std::max(max_read_len, 1));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

void launch_scan(hipStream_t st, int64_t ntiles, const uint32_t* c0, int64_t* o0, int64_t* t0, const uint32_t* c1,
                 int64_t* o1, int64_t* t1) {
  GfSeScanJobs J;
  J.j[0] = GfScanJob{c0, o0, t0};
  J.j[1] = GfScanJob{c1, o1, t1};
  hipLaunchKernelGGL(gf_se_k_scan, dim3(2), dim3(GF_SCAN_TOTALS_THREADS), 0, st, J, ntiles);
}

}  // namespace

extern "C" {

// The retry pass maps every slot, the number of retries being on the device.  Per 20 M reads of 150 bases (PANEL mix,
// 0.04 % retried) the scan took 2.44 ms with 16 650 slots, 2.44 with n / 256, 2.51 with n / 64 and 2.77 with n / 16
// (gf_map_reads_device alone: 2.14): n / 64 leaves room for 1.6 % retries at 0.07 ms.
int64_t gf_se_retry_capacity(int64_t n) { return n < 0 ? 0 : std::max<int64_t>(4096, n / 64); }

int64_t gf_se_workspace_bytes(int64_t n, int32_t max_read_len, int64_t retry_cap) {
  if (n < 0 || max_read_len < 0) return 0;
  return (int64_t)layout(n, max_read_len, retry_cap).bytes;
}

const char* gf_se_last_error(void) { return g_err.c_str(); }

int gf_se_scan_device(const gf_index* idx, const void* d_bases, const void* d_quals, const void* d_offsets,
                      int64_t n_bytes, int64_t n, int32_t max_read_len, const void* d_gene_reversed, int32_t n_genes,
                      int64_t read_id_base, int64_t retry_cap, void* d_workspace, int64_t workspace_bytes, void* d_hits,
                      int64_t hits_cap, void* d_hit_bases, void* d_hit_quals, int64_t hit_bytes_cap, void* d_totals,
                      void* stream) {
  // every check before the device is touched
  if (n < 0 || n_bytes < 0 || max_read_len < 0 || n_genes < 0 || hits_cap < 0 || hit_bytes_cap < 0 ||
      workspace_bytes < 0)
    return fail(GF_ERR_ARG, "negative size");
  if (max_read_len > GF_MAX_READ_LEN) return fail(GF_ERR_READ_TOO_LONG, "max_read_len exceeds GF_MAX_READ_LEN");
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (n > 0 && (!d_bases || !d_quals || !d_offsets)) return fail(GF_ERR_ARG, "null device pointer");
  if ((hits_cap > 0 && !d_hits) || (hit_bytes_cap > 0 && (!d_hit_bases || !d_hit_quals)))
    return fail(GF_ERR_ARG, "null output pointer");
  if (n_genes > 0 && !d_gene_reversed) return fail(GF_ERR_ARG, "null gene flags");
  if (n > (int64_t)0x7FFFFFFF) return fail(GF_ERR_CAPACITY, "more than 2^31 reads in one batch");
  const Layout L = layout(n, max_read_len, retry_cap);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)L.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_se_workspace_bytes");
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  int64_t* totals = (int64_t*)d_totals;
  GF_SCAN_HIP(hipMemsetAsync(totals, 0, 8 * sizeof(int64_t), st));
  if (n == 0) return GF_OK;

  const RetryWork& W = L.retry;
  uint8_t* wp = aligned(d_workspace);
  uint8_t* cnt = wp + L.o_cnt;
  uint8_t* stt = wp + L.o_st;
  gf_seqmatch* m1 = (gf_seqmatch*)(wp + L.o_m1);
  uint32_t* tcA = (uint32_t*)(wp + L.o_tc);
  uint32_t* tcB = tcA + L.ntiles;
  int64_t* toRC = (int64_t*)(wp + L.o_to);
  int64_t *toRB = toRC + L.ntiles, *toHC = toRB + L.ntiles, *toHB = toHC + L.ntiles;
  int64_t* scal = (int64_t*)(wp + W.o_scal);
  int64_t* r_off = (int64_t*)(wp + W.o_roff);
  uint8_t *rb = wp + W.o_rb, *rq = wp + W.o_rq, *cR = wp + W.o_cR;
  gf_seqmatch* mR = (gf_seqmatch*)(wp + W.o_mR);
  const uint8_t* rev = (const uint8_t*)d_gene_reversed;
  const unsigned grid = (unsigned)L.ntiles;
  GF_SCAN_HIP(hipMemsetAsync(scal, 0, 256, st));

  // 1. every read as it is
  int rc = gf_map_reads_device(idx, d_bases, d_offsets, n, std::max(max_read_len, 1), cnt, m1, st);
  if (rc != GF_OK) return passed_on("gf_map_reads_device", rc);
  // 2. hit / retry / neither, and the retries per tile
  hipLaunchKernelGGL(gf_se_k_classify, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, (const uint8_t*)cnt,
                     (const gf_seqmatch*)m1, (const int64_t*)d_offsets, n, rev, (int)n_genes, stt, tcA, tcB,
                     (unsigned long long*)(scal + 4));
  // 3. where each tile's retries go
  launch_scan(st, L.ntiles, tcA, toRC, scal + 0, tcB, toRB, scal + 1);
  // 4. the reverse complements, back to back; unused slots empty; over capacity the pass is emptied
  hipLaunchKernelGGL(gf_se_k_retry_write, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, (const uint8_t*)d_bases,
                     (const uint8_t*)d_quals, (const int64_t*)d_offsets, n, (const uint8_t*)stt, (const int64_t*)toRC,
                     (const int64_t*)toRB, W.R, W.Rb, r_off, rb, rq);
  hipLaunchKernelGGL(gf_se_k_retry_tail, dim3(retry_tail_blocks(W.R)), dim3(256), 0, st,
                     (const int64_t*)(scal + 0), (const int64_t*)(scal + 1), W.R, W.Rb, r_off, totals);
  GF_SCAN_HIP(hipGetLastError());
  // 5. the retry slots (the number of retries is on the device: every slot is mapped, the empty ones give count 0)
  rc = gf_map_reads_device(idx, rb, r_off, W.R, std::max(max_read_len, 1), cR, mR, st);
  if (rc != GF_OK) return passed_on("gf_map_reads_device", rc);
  // 6. the hits in read order: count per tile, scan, write; the totals
  GfSeFinalIn F;
  F.bases = (const uint8_t*)d_bases; F.quals = (const uint8_t*)d_quals; F.offsets = (const int64_t*)d_offsets;
  F.m1 = m1; F.st = stt; F.tile_off_rc = toRC; F.cR = cR; F.mR = mR; F.r_off = r_off; F.r_bases = rb; F.r_quals = rq;
  F.cap_reads = W.R; F.rev = rev; F.n_genes = (int)n_genes;
  hipLaunchKernelGGL(gf_se_k_final<false>, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, F, n, read_id_base, tcA, tcB,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, (gf_pair_hit*)nullptr, (int64_t)0,
                     (uint8_t*)nullptr, (uint8_t*)nullptr, (int64_t)0);
  launch_scan(st, L.ntiles, tcA, toHC, scal + 2, tcB, toHB, scal + 3);
  hipLaunchKernelGGL(gf_se_k_final<true>, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, F, n, read_id_base,
                     (uint32_t*)nullptr, (uint32_t*)nullptr, (const int64_t*)toHC, (const int64_t*)toHB,
                     (gf_pair_hit*)d_hits, hits_cap, (uint8_t*)d_hit_bases, (uint8_t*)d_hit_quals, hit_bytes_cap);
  hipLaunchKernelGGL(gf_se_k_totals, dim3(1), dim3(1), 0, st, (const int64_t*)(scal + 2), (const int64_t*)(scal + 3),
                     (const unsigned long long*)(scal + 4), hits_cap, hit_bytes_cap, totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
