// libgfqc.so: per-cycle quality and base-content tables and the insert-size histogram of FASTQ records in HBM
// (include/gf_read_qc.h).  Of libgfmatch.so's public ABI it uses gf_index_info_get, for the index's device.
#include "gf_qc_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a pair in gf_qc_k_insert (gf_at_kernels.h says why)
constexpr int kLanesPerPair = 16;

// blocks of a launch in which every block has `per_block` records of its own in its first round
unsigned blocks_for(int64_t n, int per_block) {
  return (unsigned)std::min<int64_t>((n + per_block - 1) / per_block, GF_QC_GRID);
}

// the checks both calls share, before the device is touched
int checked(const gf_index* idx, const void* d_off, int64_t n, const void* d_out) {
  if (n < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > (int64_t)1 << 38) return fail(GF_ERR_ARG, "record count out of range");
  if (!idx || !d_out) return fail(GF_ERR_ARG, "null index or table");
  if (!d_off) return fail(GF_ERR_ARG, "null offsets");
  return GF_OK;
}

}  // namespace

extern "C" {

const char* gf_qc_last_error(void) { return g_err.c_str(); }

int gf_qc_stats_device(const gf_index* idx, const void* d_bases, const void* d_quals, const void* d_off, int64_t n,
                       void* d_table, void* stream) {
  if (const int rc = checked(idx, d_off, n, d_table)) return rc;
  if (n > 0 && (!d_bases || !d_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_table, "the table", off_device)) return drc;
  if (const int drc = device_of(d_off, "the offsets", off_device)) return drc;
  if (n == 0) return GF_OK;
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_qc_k_stats, dim3(blocks_for(n, GF_QC_BLOCK_WAVES)), dim3(GF_SCAN_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)d_bases, (const uint8_t*)d_quals, (const int64_t*)d_off, n,
                     (unsigned long long*)d_table);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_qc_insert_device(const gf_index* idx, const void* d_l_bases, const void* d_l_off, const void* d_r_bases,
                        const void* d_r_off, int64_t n, void* d_hist, void* stream) {
  if (const int rc = checked(idx, d_l_off, n, d_hist)) return rc;
  if (!d_r_off) return fail(GF_ERR_ARG, "null offsets");
  if (n > 0 && (!d_l_bases || !d_r_bases)) return fail(GF_ERR_ARG, "null bases with records");
  int off_device = -1;
  if (const int drc = device_of(d_hist, "the histogram", off_device)) return drc;
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  if (n == 0) return GF_OK;
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_qc_k_insert<kLanesPerPair>, dim3(blocks_for(n, GF_SCAN_THREADS / kLanesPerPair)),
                     dim3(GF_SCAN_THREADS), 0, (hipStream_t)stream, (const uint8_t*)d_l_bases,
                     (const int64_t*)d_l_off, (const uint8_t*)d_r_bases, (const int64_t*)d_r_off, n,
                     (unsigned long long*)d_hist);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
