// libgfmcsv.so: the paired-end scan of multi-CSV mode (include/gf_multi_csv.h) on top of libgfmatch.so's public ABI.
#include "gf_mc_kernels.h"
#include "gf_scan_host.h"

namespace {

int64_t tiles_of(int64_t n) { return (n + GF_MC_TILE - 1) / GF_MC_TILE; }

// The prepared buffer, carved in 256-byte aligned pieces from a 256-byte aligned base.
struct Prepared {
  int64_t ntiles = 0, cap_bases = 0, chunks = 0;
  size_t o_hdr = 0, o_mlen = 0, o_mdiff = 0, o_rank = 0, o_mpos = 0, o_uoff = 0, o_moff = 0, o_bases = 0, o_mq = 0,
         o_pk = 0, o_iv = 0, o_tc = 0, o_to = 0;
  size_t bytes = 0;
};

Prepared prepared_layout(int64_t n, int64_t l_bytes, int64_t r_bytes) {
  Prepared L;
  L.ntiles = tiles_of(n);
  L.cap_bases = l_bytes + r_bytes;  // (a merged read is shorter than its pair: both lists together fit)
  L.chunks = gf_packed_chunks(L.cap_bases);
  size_t off = 0;
  L.o_hdr = take(off, 256);  // int64: [0] unmerged pairs, [1] their bytes, [2] merged pairs, [3] their bytes
  L.o_mlen = take(off, (size_t)n * 4);
  L.o_mdiff = take(off, (size_t)n * 4);
  L.o_rank = take(off, (size_t)n * 4);
  L.o_mpos = take(off, (size_t)n * 8);
  L.o_uoff = take(off, (2 * (size_t)n + 1) * 8);
  L.o_moff = take(off, ((size_t)n + 1) * 8);
  // the mapping and merge kernels read whole 16-byte chunks around a span (gfmatch.h), inside this buffer
  L.o_bases = take(off, (size_t)L.cap_bases + 64);
  L.o_mq = take(off, (size_t)L.cap_bases + 64);
  L.o_pk = take(off, (size_t)L.chunks * 4);
  L.o_iv = take(off, (size_t)L.chunks * 2);
  L.o_tc = take(off, (size_t)L.ntiles * GF_MC_SCAN_JOBS * sizeof(uint32_t));
  L.o_to = take(off, (size_t)L.ntiles * GF_MC_SCAN_JOBS * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

int64_t resolve_retry_cap(int64_t n, int64_t retry_cap) {
  const int64_t r = retry_cap <= 0 ? gf_mc_retry_capacity(n) : retry_cap;
  return std::min(r, 3 * n);  // (no more retries than candidates)
}

// The scan's workspace.
struct Work {
  int64_t ntiles = 0;
  size_t o_cU = 0, o_cM = 0, o_mU = 0, o_mM = 0, o_st = 0, o_slot = 0, o_tc = 0, o_to = 0;
  RetryWork retry;
  size_t bytes = 0;
};

Work work_layout(int64_t n, int32_t max_read_len, int64_t retry_cap) {
  Work L;
  L.ntiles = tiles_of(n);
  size_t off = 0;
  L.o_cU = take(off, 2 * (size_t)n);
  L.o_cM = take(off, (size_t)n);
  L.o_mU = take(off, 2 * (size_t)n * 2 * sizeof(gf_seqmatch));
  L.o_mM = take(off, (size_t)n * 2 * sizeof(gf_seqmatch));
  L.o_st = take(off, 3 * (size_t)n);
  L.o_slot = take(off, 3 * (size_t)n * sizeof(int32_t));
  L.o_tc = take(off, (size_t)L.ntiles * 2 * sizeof(uint32_t));
  L.o_to = take(off, (size_t)L.ntiles * 2 * sizeof(int64_t));
  const int64_t R = resolve_retry_cap(n, retry_cap);
  // (a retried merged read is up to twice as long)
  L.retry.carve(off, R, R * std::max<int64_t>(2 * (int64_t)max_read_len, 1));
  L.bytes = off + 256;
  return L;
}

void launch_scan(hipStream_t st, int64_t ntiles, int jobs, const GfScanJob* j) {
  GfMcScanJobs J;
  for (int k = 0; k < GF_MC_SCAN_JOBS; ++k) J.j[k] = j[k < jobs ? k : 0];
  hipLaunchKernelGGL(gf_mc_k_scan, dim3((unsigned)jobs), dim3(GF_SCAN_TOTALS_THREADS), 0, st, J, ntiles);
}

// what both calls check about the pairs, before the device is touched
int check_pairs(const gf_index* idx, const void* d_l_bases, const void* d_l_quals, const void* d_l_offsets, int64_t l_bytes,
                const void* d_r_bases, const void* d_r_quals, const void* d_r_offsets, int64_t r_bytes, int64_t n,
                int32_t max_read_len) {
  if (n < 0 || l_bytes < 0 || r_bytes < 0 || max_read_len < 0) return fail(GF_ERR_ARG, "negative size");
  if (2 * (int64_t)max_read_len > GF_MAX_READ_LEN)
    return fail(GF_ERR_READ_TOO_LONG, "2 * max_read_len exceeds GF_MAX_READ_LEN");
  if (!idx) return fail(GF_ERR_ARG, "null index");
  if (n > 0 && (!d_l_bases || !d_l_quals || !d_l_offsets || !d_r_bases || !d_r_quals || !d_r_offsets))
    return fail(GF_ERR_ARG, "null device pointer");
  if (n > (int64_t)0x7FFFFFFF / 3) return fail(GF_ERR_CAPACITY, "more than 2^31 / 3 pairs in one batch");
  return GF_OK;
}

}  // namespace

extern "C" {

int64_t gf_mc_prepared_bytes(int64_t n, int64_t l_bytes, int64_t r_bytes, int32_t max_read_len) {
  if (n < 0 || l_bytes < 0 || r_bytes < 0 || max_read_len < 0) return 0;
  return (int64_t)prepared_layout(n, l_bytes, r_bytes).bytes;
}

int64_t gf_mc_retry_capacity(int64_t n) { return n < 0 ? 0 : std::max<int64_t>(4096, n / 32); }

int64_t gf_mc_scan_workspace_bytes(int64_t n, int32_t max_read_len, int64_t retry_cap) {
  if (n < 0 || max_read_len < 0) return 0;
  return (int64_t)work_layout(n, max_read_len, retry_cap).bytes;
}

const char* gf_mc_last_error(void) { return g_err.c_str(); }

int gf_mc_pairs_prepare_device(const gf_index* idx, const void* d_l_bases, const void* d_l_quals, const void* d_l_offsets,
                               int64_t l_bytes, const void* d_r_bases, const void* d_r_quals, const void* d_r_offsets,
                               int64_t r_bytes, int64_t n, int32_t max_read_len, void* d_prepared, int64_t prepared_bytes,
                               void* stream) {
  // every check before the device is touched
  if (prepared_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  int rc = check_pairs(idx, d_l_bases, d_l_quals, d_l_offsets, l_bytes, d_r_bases, d_r_quals, d_r_offsets, r_bytes, n,
                       max_read_len);
  if (rc != GF_OK) return rc;
  const Prepared L = prepared_layout(n, l_bytes, r_bytes);
  if (!d_prepared || prepared_bytes < (int64_t)L.bytes)
    return fail(GF_ERR_CAPACITY, "prepared buffer smaller than gf_mc_prepared_bytes");
  gf_index_info info;
  rc = gf_index_info_get(idx, &info);
  if (rc != GF_OK) return passed_on("gf_index_info_get", rc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;

  uint8_t* pp = aligned(d_prepared);
  int64_t* hdr = (int64_t*)(pp + L.o_hdr);
  int32_t *m_len = (int32_t*)(pp + L.o_mlen), *m_diff = (int32_t*)(pp + L.o_mdiff), *rank = (int32_t*)(pp + L.o_rank);
  int64_t *m_pos = (int64_t*)(pp + L.o_mpos), *u_off = (int64_t*)(pp + L.o_uoff), *m_off = (int64_t*)(pp + L.o_moff);
  uint8_t *pb = pp + L.o_bases, *mq = pp + L.o_mq;
  uint32_t* tc = (uint32_t*)(pp + L.o_tc);
  int64_t* to = (int64_t*)(pp + L.o_to);
  GF_SCAN_HIP(hipMemsetAsync(hdr, 0, 256, st));
  // (offsets of two lists without a read: what n = 0 leaves, and harmless before the kernels write them)
  GF_SCAN_HIP(hipMemsetAsync(u_off, 0, sizeof(int64_t), st));
  GF_SCAN_HIP(hipMemsetAsync(m_off, 0, sizeof(int64_t), st));
  if (n == 0) return GF_OK;

  // 1. fast_merge: the merged length (0 = not merged) and merged_diff per pair
  rc = gf_fast_merge_find_device(idx, d_l_bases, d_l_quals, d_l_offsets, d_r_bases, d_r_quals, d_r_offsets, n,
                                 std::max(max_read_len, 1), m_len, m_diff, st);
  if (rc != GF_OK) return passed_on("gf_fast_merge_find_device", rc);
  // 2. the two lists: what each tile puts into them, where each tile starts, the scatter of the unmerged reads
  const unsigned grid = (unsigned)L.ntiles;
  uint32_t *tc_uc = tc, *tc_ub = tc + L.ntiles, *tc_mc = tc + 2 * L.ntiles, *tc_mb = tc + 3 * L.ntiles;
  int64_t *to_uc = to, *to_ub = to + L.ntiles, *to_mc = to + 2 * L.ntiles, *to_mb = to + 3 * L.ntiles;
  hipLaunchKernelGGL(gf_mc_k_tile_counts, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, (const int32_t*)m_len,
                     (const int64_t*)d_l_offsets, (const int64_t*)d_r_offsets, n, tc_uc, tc_ub, tc_mc, tc_mb);
  const GfScanJob jobs[4] = {{tc_uc, to_uc, hdr + 0}, {tc_ub, to_ub, hdr + 1}, {tc_mc, to_mc, hdr + 2}, {tc_mb, to_mb, hdr + 3}};
  launch_scan(st, L.ntiles, 4, jobs);
  hipLaunchKernelGGL(gf_mc_k_gather, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, (const uint8_t*)d_l_bases,
                     (const int64_t*)d_l_offsets, (const uint8_t*)d_r_bases, (const int64_t*)d_r_offsets,
                     (const int32_t*)m_len, n, (const int64_t*)to_uc, (const int64_t*)to_ub, (const int64_t*)to_mc,
                     (const int64_t*)to_mb, (const int64_t*)(hdr + 1), rank, u_off, m_off, m_pos, pb);
  hipLaunchKernelGGL(gf_mc_k_list_tail, dim3((unsigned)std::min<int64_t>((2 * n + 256) / 256, 2048)), dim3(256), 0, st,
                     (const int64_t*)hdr, n, u_off, m_off);
  GF_SCAN_HIP(hipGetLastError());
  // 3. the merged reads and their qualities, behind the unmerged reads
  rc = gf_fast_merge_write_device(idx, d_l_bases, d_l_quals, d_l_offsets, d_r_bases, d_r_quals, d_r_offsets, n, m_len,
                                  m_pos, pb, mq, st);
  if (rc != GF_OK) return passed_on("gf_fast_merge_write_device", rc);
  // 4. both lists in the packed form
  rc = gf_pack_bases_device(idx, pb, L.cap_bases, pp + L.o_pk, pp + L.o_iv, st);
  if (rc != GF_OK) return passed_on("gf_pack_bases_device", rc);
  return GF_OK;
}

int gf_mc_pairs_scan_device(const gf_index* idx, const void* d_prepared, const void* d_l_bases, const void* d_l_quals,
                            const void* d_l_offsets, int64_t l_bytes, const void* d_r_bases, const void* d_r_quals,
                            const void* d_r_offsets, int64_t r_bytes, int64_t n, int32_t max_read_len,
                            const void* d_gene_reversed, int32_t n_genes, int64_t pair_id_base, int64_t retry_cap,
                            void* d_workspace, int64_t workspace_bytes, void* d_hits, int64_t hits_cap, void* d_hit_bases,
                            void* d_hit_quals, int64_t hit_bytes_cap, void* d_totals, void* stream) {
  // every check before the device is touched
  if (n_genes < 0 || hits_cap < 0 || hit_bytes_cap < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  int rc = check_pairs(idx, d_l_bases, d_l_quals, d_l_offsets, l_bytes, d_r_bases, d_r_quals, d_r_offsets, r_bytes, n,
                       max_read_len);
  if (rc != GF_OK) return rc;
  if (!d_totals) return fail(GF_ERR_ARG, "null totals");
  if (n > 0 && !d_prepared) return fail(GF_ERR_ARG, "null prepared buffer");
  if ((hits_cap > 0 && !d_hits) || (hit_bytes_cap > 0 && (!d_hit_bases || !d_hit_quals)))
    return fail(GF_ERR_ARG, "null output pointer");
  if (n_genes > 0 && !d_gene_reversed) return fail(GF_ERR_ARG, "null gene flags");
  const Work K = work_layout(n, max_read_len, retry_cap);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)K.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_mc_scan_workspace_bytes");
  gf_index_info info;
  rc = gf_index_info_get(idx, &info);
  if (rc != GF_OK) return passed_on("gf_index_info_get", rc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  int64_t* totals = (int64_t*)d_totals;
  GF_SCAN_HIP(hipMemsetAsync(totals, 0, 8 * sizeof(int64_t), st));
  if (n == 0) return GF_OK;

  const Prepared L = prepared_layout(n, l_bytes, r_bytes);
  const uint8_t* pp = aligned(d_prepared);
  const int64_t* hdr = (const int64_t*)(pp + L.o_hdr);
  uint8_t* wp = aligned(d_workspace);
  const RetryWork& W = K.retry;
  uint8_t *cU = wp + K.o_cU, *cM = wp + K.o_cM;
  gf_seqmatch *mU = (gf_seqmatch*)(wp + K.o_mU), *mM = (gf_seqmatch*)(wp + K.o_mM);
  uint8_t* stt = wp + K.o_st;
  int32_t* slot_of = (int32_t*)(wp + K.o_slot);
  uint32_t *tcA = (uint32_t*)(wp + K.o_tc), *tcB = tcA + K.ntiles;
  int64_t *toA = (int64_t*)(wp + K.o_to), *toB = toA + K.ntiles;
  int64_t* scal = (int64_t*)(wp + W.o_scal);
  int64_t* r_off = (int64_t*)(wp + W.o_roff);
  uint8_t *rb = wp + W.o_rb, *rq = wp + W.o_rq, *cR = wp + W.o_cR;
  gf_seqmatch* mR = (gf_seqmatch*)(wp + W.o_mR);
  const unsigned grid = (unsigned)K.ntiles;
  const int32_t merged_max = (int32_t)std::max<int64_t>(2 * (int64_t)max_read_len, 1);
  GF_SCAN_HIP(hipMemsetAsync(scal, 0, 256, st));

  // 1. both lists, from the packed form: R1 / R2 of the pairs that did not merge at the width of max_read_len, the
  //    merged reads at twice that (the unused slots of either list are empty reads: count 0)
  rc = gf_map_reads_packed_device(idx, pp + L.o_pk, pp + L.o_iv, pp + L.o_uoff, 2 * n, std::max(max_read_len, 1), cU, mU, st);
  if (rc != GF_OK) return passed_on("gf_map_reads_packed_device", rc);
  rc = gf_map_reads_packed_device(idx, pp + L.o_pk, pp + L.o_iv, pp + L.o_moff, n, merged_max, cM, mM, st);
  if (rc != GF_OK) return passed_on("gf_map_reads_packed_device", rc);
  // 2. hit / retry / neither per candidate, and the retries per tile
  GfMcIn P;
  P.l_bases = (const uint8_t*)d_l_bases; P.l_quals = (const uint8_t*)d_l_quals; P.l_off = (const int64_t*)d_l_offsets;
  P.r_bases = (const uint8_t*)d_r_bases; P.r_quals = (const uint8_t*)d_r_quals; P.r_off = (const int64_t*)d_r_offsets;
  P.p_bases = pp + L.o_bases; P.p_mquals = pp + L.o_mq;
  P.m_len = (const int32_t*)(pp + L.o_mlen); P.m_diff = (const int32_t*)(pp + L.o_mdiff);
  P.rank = (const int32_t*)(pp + L.o_rank); P.m_pos = (const int64_t*)(pp + L.o_mpos);
  P.cU = cU; P.cM = cM; P.mU = mU; P.mM = mM;
  P.rev = (const uint8_t*)d_gene_reversed; P.n_genes = (int)n_genes;
  hipLaunchKernelGGL(gf_mc_k_classify, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, P, n, stt, tcA, tcB);
  // 3. where each tile's retries go; the reverse complements, back to back; unused slots empty
  const GfScanJob rj[2] = {{tcA, toA, scal + 0}, {tcB, toB, scal + 1}};
  launch_scan(st, K.ntiles, 2, rj);
  hipLaunchKernelGGL(gf_mc_k_retry_write, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, P, n, (const uint8_t*)stt,
                     (const int64_t*)toA, (const int64_t*)toB, W.R, W.Rb, r_off, rb, rq, slot_of);
  hipLaunchKernelGGL(gf_mc_k_retry_tail, dim3(retry_tail_blocks(W.R)), dim3(256), 0, st,
                     (const int64_t*)(scal + 0), (const int64_t*)(scal + 1), W.R, W.Rb, r_off, totals);
  GF_SCAN_HIP(hipGetLastError());
  // 4. the retry slots (the number of retries is on the device: every slot is mapped, the empty ones give count 0)
  rc = gf_map_reads_device(idx, rb, r_off, W.R, merged_max, cR, mR, st);
  if (rc != GF_OK) return passed_on("gf_map_reads_device", rc);
  // 5. the hits in push order: count per tile, scan, write; the totals
  GfMcFinalIn F;
  F.st = stt; F.slot_of = slot_of; F.cR = cR; F.mR = mR; F.r_off = r_off; F.r_bases = rb; F.r_quals = rq;
  hipLaunchKernelGGL(gf_mc_k_final<false>, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, P, F, n, pair_id_base, tcA, tcB,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, (gf_pair_hit*)nullptr, (int64_t)0,
                     (uint8_t*)nullptr, (uint8_t*)nullptr, (int64_t)0);
  const GfScanJob hj[2] = {{tcA, toA, scal + 2}, {tcB, toB, scal + 3}};
  launch_scan(st, K.ntiles, 2, hj);
  hipLaunchKernelGGL(gf_mc_k_final<true>, dim3(grid), dim3(GF_SCAN_THREADS), 0, st, P, F, n, pair_id_base,
                     (uint32_t*)nullptr, (uint32_t*)nullptr, (const int64_t*)toA, (const int64_t*)toB,
                     (gf_pair_hit*)d_hits, hits_cap, (uint8_t*)d_hit_bases, (uint8_t*)d_hit_quals, hit_bytes_cap);
  hipLaunchKernelGGL(gf_mc_k_totals, dim3(1), dim3(1), 0, st, (const int64_t*)(scal + 2), (const int64_t*)(scal + 3),
                     hdr + 2, hits_cap, hit_bytes_cap, totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
