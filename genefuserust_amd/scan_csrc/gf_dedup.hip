// libgfdedup.so: duplicate records found with a hash table in HBM and emptied (include/gf_dedup.h).  Of libgfmatch.so's
// public ABI it uses gf_index_info_get, for the index's device.
#include "gf_dd_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a record in gf_dd_k_keys (gf_dd_kernels.h says why)
constexpr int kLanesPerRecord = 16;

// The workspace of the removal, as the read filter's: per side the kept bytes of every tile of GF_PP_TILE records,
// scanned in place to where the tile starts, and one entry more for the sum.
struct Layout {
  int64_t tiles = 0;
  size_t o_sum_l = 0, o_sum_r = 0;
  size_t bytes = 0;
};

Layout layout(int64_t n) {
  Layout L;
  L.tiles = (n + GF_PP_TILE - 1) / GF_PP_TILE;
  size_t off = 0;
  L.o_sum_l = take(off, ((size_t)L.tiles + 1) * sizeof(int64_t));
  L.o_sum_r = take(off, ((size_t)L.tiles + 1) * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

unsigned blocks_over(int64_t n) { return (unsigned)((n + GF_SCAN_THREADS - 1) / GF_SCAN_THREADS); }

int checked_count(int64_t n) {
  if (n < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > (int64_t)1 << 38) return fail(GF_ERR_ARG, "record count out of range");
  return GF_OK;
}

int checked_slots(int64_t slots) {
  if (!gf_dd_slots_ok(slots) || slots > (int64_t)1 << 38)
    return fail(GF_ERR_ARG, "slots must be a power of two, at least 1024");
  return GF_OK;
}

// the index's device
int device_of_index(const gf_index* idx, int& device) {
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  device = info.device;
  return GF_OK;
}

}  // namespace

extern "C" {

int64_t gf_dd_workspace_bytes(int64_t n) { return n < 0 ? 0 : (int64_t)layout(n).bytes; }

const char* gf_dd_last_error(void) { return g_err.c_str(); }

int gf_dd_keys_device(const gf_index* idx, const void* d_l_bases, const void* d_l_off, const void* d_r_bases,
                      const void* d_r_off, int64_t n, void* d_rec_keys, void* stream) {
  // every check before the device is touched
  if (const int rc = checked_count(n)) return rc;
  if (!idx) return fail(GF_ERR_ARG, "null index");
  if (!d_l_off) return fail(GF_ERR_ARG, "null offsets");
  const bool pairs = d_r_bases || d_r_off;
  if (pairs && !d_r_off) return fail(GF_ERR_ARG, "null offsets");
  if (n > 0 && (!d_l_bases || (pairs && !d_r_bases))) return fail(GF_ERR_ARG, "null bases with records");
  if (n > 0 && !d_rec_keys) return fail(GF_ERR_ARG, "null record keys");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  if (n == 0) return GF_OK;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_dd_k_keys<kLanesPerRecord>, dim3((unsigned)layout(n).tiles), dim3(GF_SCAN_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)d_l_bases, (const int64_t*)d_l_off,
                     (const uint8_t*)d_r_bases, (const int64_t*)d_r_off, n, (unsigned long long*)d_rec_keys);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_dd_insert_device(const gf_index* idx, const void* d_rec_keys, int64_t n, int64_t first_index, void* d_keys,
                        void* d_first, void* d_count, int64_t slots, void* d_rec_slot, void* d_totals, void* stream) {
  if (const int rc = checked_count(n)) return rc;
  if (first_index < 0 || first_index > INT64_MAX - n) return fail(GF_ERR_ARG, "first_index out of range");
  if (const int rc = checked_slots(slots)) return rc;
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_keys || !d_first) return fail(GF_ERR_ARG, "null table");
  if (n > 0 && (!d_rec_keys || !d_rec_slot)) return fail(GF_ERR_ARG, "null record keys or slots");
  int off_device = -1;
  if (const int drc = device_of(d_keys, "the table", off_device)) return drc;
  if (const int drc = device_of(d_totals, "the totals", off_device)) return drc;
  if (n == 0) return GF_OK;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_dd_k_insert, dim3(blocks_over(n)), dim3(GF_SCAN_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)d_rec_keys, n, first_index, (unsigned long long*)d_keys,
                     (long long*)d_first, (unsigned int*)d_count, slots, (int64_t*)d_rec_slot,
                     (unsigned long long*)d_totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_dd_remove_device(const gf_index* idx, const void* d_l_bases, const void* d_l_quals, const void* d_l_off,
                        const void* d_r_bases, const void* d_r_quals, const void* d_r_off, int64_t n,
                        int64_t first_index, const void* d_rec_slot, const void* d_first, void* d_workspace,
                        int64_t workspace_bytes, void* d_l_out_bases, void* d_l_out_quals, void* d_l_out_off,
                        void* d_r_out_bases, void* d_r_out_quals, void* d_r_out_off, void* d_dup, void* d_totals,
                        void* stream) {
  if (n < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = checked_count(n)) return rc;
  if (first_index < 0 || first_index > INT64_MAX - n) return fail(GF_ERR_ARG, "first_index out of range");
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_first) return fail(GF_ERR_ARG, "null table");
  if (!d_l_off || !d_l_out_off) return fail(GF_ERR_ARG, "null offsets");
  const bool pairs = d_r_bases || d_r_quals || d_r_off;
  if (pairs && !(d_r_bases && d_r_quals && d_r_off)) return fail(GF_ERR_ARG, "some of the mates' pointers are null");
  if (pairs && !d_r_out_off) return fail(GF_ERR_ARG, "null offsets");
  if (n > 0 && (!d_l_bases || !d_l_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  if (n > 0 && (!d_l_out_bases || !d_l_out_quals || (pairs && (!d_r_out_bases || !d_r_out_quals))))
    return fail(GF_ERR_ARG, "null output pointer");
  if (n > 0 && (!d_rec_slot || !d_dup)) return fail(GF_ERR_ARG, "null record slots or duplicate flags");
  const Layout W = layout(n);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)W.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_dd_workspace_bytes");
  int off_device = -1;
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  if (const int drc = device_of(d_first, "the table", off_device)) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    GF_SCAN_HIP(hipMemsetAsync(d_l_out_off, 0, sizeof(int64_t), st));
    if (pairs) GF_SCAN_HIP(hipMemsetAsync(d_r_out_off, 0, sizeof(int64_t), st));
    return GF_OK;
  }
  const int sides = pairs ? 2 : 1;
  const GfPpSide L{(const uint8_t*)d_l_bases, (const uint8_t*)d_l_quals, (const int64_t*)d_l_off};
  const GfPpSide R{(const uint8_t*)d_r_bases, (const uint8_t*)d_r_quals, (const int64_t*)d_r_off};
  const GfPpOut out_l{(uint8_t*)d_l_out_bases, (uint8_t*)d_l_out_quals, (int64_t*)d_l_out_off};
  const GfPpOut out_r{(uint8_t*)d_r_out_bases, (uint8_t*)d_r_out_quals, (int64_t*)d_r_out_off};
  int64_t* sum_l = (int64_t*)(aligned(d_workspace) + W.o_sum_l);
  int64_t* sum_r = (int64_t*)(aligned(d_workspace) + W.o_sum_r);
  const dim3 grid((unsigned)W.tiles);
  hipLaunchKernelGGL(gf_dd_k_decide, grid, dim3(GF_SCAN_THREADS), 0, st, L, R, sides, n, first_index,
                     (const int64_t*)d_rec_slot, (const long long*)d_first, out_l, out_r, sum_l, sum_r,
                     (uint8_t*)d_dup, (unsigned long long*)d_totals);
  if (pairs)
    hipLaunchKernelGGL(gf_pp_k_scan<2>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  else
    hipLaunchKernelGGL(gf_pp_k_scan<1>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  hipLaunchKernelGGL(gf_pp_k_gather, grid, dim3(GF_SCAN_THREADS), 0, st, L, R, sides, n, out_l, out_r,
                     (const int64_t*)sum_l, (const int64_t*)sum_r);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_dd_rehash_device(const gf_index* idx, const void* d_old_keys, const void* d_old_first, const void* d_old_count,
                        int64_t old_slots, void* d_new_keys, void* d_new_first, void* d_new_count, int64_t new_slots,
                        void* stream) {
  if (const int rc = checked_slots(old_slots)) return rc;
  if (const int rc = checked_slots(new_slots)) return rc;
  if (new_slots <= old_slots) return fail(GF_ERR_ARG, "a rehash only grows the table");
  if (!idx) return fail(GF_ERR_ARG, "null index");
  if (!d_old_keys || !d_old_first || !d_new_keys || !d_new_first) return fail(GF_ERR_ARG, "null table");
  int off_device = -1;
  if (const int drc = device_of(d_old_keys, "the table", off_device)) return drc;
  if (const int drc = device_of(d_new_keys, "the table", off_device)) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gf_dd_k_fill, dim3(blocks_over(new_slots)), dim3(GF_SCAN_THREADS), 0, st,
                     (unsigned long long*)d_new_keys, (long long*)d_new_first, (unsigned int*)d_new_count, new_slots);
  hipLaunchKernelGGL(gf_dd_k_rehash, dim3(blocks_over(old_slots)), dim3(GF_SCAN_THREADS), 0, st,
                     (const unsigned long long*)d_old_keys, (const long long*)d_old_first,
                     (const unsigned int*)d_old_count, old_slots, (unsigned long long*)d_new_keys,
                     (long long*)d_new_first, (unsigned int*)d_new_count, new_slots);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_dd_histogram_device(const gf_index* idx, const void* d_keys, const void* d_count, int64_t slots, void* d_hist,
                           void* stream) {
  if (const int rc = checked_slots(slots)) return rc;
  if (!idx || !d_hist) return fail(GF_ERR_ARG, "null index or histogram");
  if (!d_keys || !d_count) return fail(GF_ERR_ARG, "null table");
  int off_device = -1;
  if (const int drc = device_of(d_keys, "the table", off_device)) return drc;
  if (const int drc = device_of(d_hist, "the histogram", off_device)) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_dd_k_histogram, dim3(blocks_over(slots)), dim3(GF_SCAN_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)d_keys, (const unsigned int*)d_count, slots,
                     (unsigned long long*)d_hist);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
