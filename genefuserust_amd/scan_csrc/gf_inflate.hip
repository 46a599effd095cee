// libgfinflate.so: BGZF members walked on the host and inflated on the device (include/gf_inflate.h).  It takes no
// gf_index and finds its device from the pointers it is given.
#include "gf_if_kernels.h"
#include "gf_scan_host.h"

#include "../../include/gf_inflate.h"

static_assert(GF_IF_ROW == GF_IF_ROW_INT64 && GF_IF_CRC == GF_IF_STATUS_CRC && GF_IF_BAD_ROW == GF_IF_STATUS_BAD_ROW,
              "gf_if_core.h and gf_inflate.h name the same rows and statuses");

namespace {

uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

}  // namespace

extern "C" {

const char* gf_if_last_error(void) { return g_err.c_str(); }

int gf_if_walk_blocks(const void* comp_, int64_t comp_bytes, int64_t file_offset, int64_t text_budget, int64_t max_members,
                      int64_t* table, int64_t* result) {
  if (comp_bytes < 0 || text_budget < 0 || max_members < 0 || file_offset < 0) return fail(GF_ERR_ARG, "negative size");
  if (!result || (comp_bytes > 0 && !comp_) || (max_members > 0 && !table)) return fail(GF_ERR_ARG, "null pointer");
  const uint8_t* comp = (const uint8_t*)comp_;
  static const uint8_t magic[4] = {0x1f, 0x8b, 0x08, 0x04};
  int64_t off = 0, text = 0, rows = 0, why = GF_IF_WALK_END;
  while (off < comp_bytes) {
    const int64_t left = comp_bytes - off;
    const uint8_t* h = comp + off;
    bool magic_ok = true;
    for (int64_t k = 0; k < std::min<int64_t>(left, 4); k++) magic_ok = magic_ok && h[k] == magic[k];
    if (!magic_ok) { why = GF_IF_WALK_NOT_BGZF; break; }
    if (left < 12) { why = GF_IF_WALK_INSIDE; break; }
    const int64_t xlen = le16(h + 10);
    if (left < 12 + xlen) { why = GF_IF_WALK_INSIDE; break; }
    // the extra subfields: SI1 SI2 SLEN data
    int64_t bsize = -1;
    for (int64_t p = 12; p + 4 <= 12 + xlen; p += 4 + le16(h + p + 2)) {
      if (h[p] == 'B' && h[p + 1] == 'C' && le16(h + p + 2) == 2 && p + 6 <= 12 + xlen) {
        bsize = (int64_t)le16(h + p + 4) + 1;
        break;
      }
    }
    if (bsize < 12 + xlen + 8) { why = GF_IF_WALK_NOT_BGZF; break; }
    if (left < bsize) { why = GF_IF_WALK_INSIDE; break; }
    const int64_t crc = le32(h + bsize - 8), isize = le32(h + bsize - 4);
    if (isize > GF_IF_MAX_TEXT) { why = GF_IF_WALK_NOT_BGZF; break; }
    if (text + isize > text_budget) { why = GF_IF_WALK_BUDGET; break; }
    if (rows >= max_members) { why = GF_IF_WALK_CAPACITY; break; }
    int64_t* row = table + rows * GF_IF_ROW;
    row[0] = off + 12 + xlen, row[1] = bsize - xlen - 20, row[2] = text, row[3] = isize, row[4] = crc;
    row[5] = file_offset + off;
    rows++, off += bsize, text += isize;
  }
  result[0] = rows, result[1] = off, result[2] = text, result[3] = why, result[4] = off;
  return GF_OK;
}

int64_t gf_if_workspace_bytes(int64_t n_members) {
  (void)n_members;
  return 0;
}

int gf_if_inflate_device(const void* d_comp, int64_t comp_bytes, const void* d_table, int64_t n_members, void* d_out,
                         int64_t out_cap, void* d_status, void* d_totals, void* d_workspace, int64_t workspace_bytes,
                         void* stream) {
  // every check before the device is touched
  (void)d_workspace;
  if (comp_bytes < 0 || n_members < 0 || out_cap < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (!d_totals) return fail(GF_ERR_ARG, "null totals");
  if (n_members > 0 && (!d_table || !d_status)) return fail(GF_ERR_ARG, "null table or statuses");
  if (comp_bytes > 0 && !d_comp) return fail(GF_ERR_ARG, "null compressed bytes");
  if (out_cap > 0 && !d_out) return fail(GF_ERR_ARG, "null output pointer");
  if (workspace_bytes < gf_if_workspace_bytes(n_members)) return fail(GF_ERR_CAPACITY, "workspace smaller than gf_if_workspace_bytes");
  int dev = 0;
  const int drc = n_members > 0 ? device_of(d_table, "the table", dev) : device_of(d_totals, "the totals", dev);
  if (drc != GF_OK) return drc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the table's device");
  hipStream_t st = (hipStream_t)stream;
  // the grid is capped and strides over the members
  const unsigned blocks = (unsigned)std::min<int64_t>(n_members, GF_IF_MAX_BLOCKS);
  if (n_members > 0)
    hipLaunchKernelGGL(gf_if_k_inflate, dim3(blocks), dim3(GF_IF_THREADS), 0, st, (const uint8_t*)d_comp, comp_bytes,
                       (const int64_t*)d_table, n_members, (uint8_t*)d_out, out_cap, (int32_t*)d_status);
  hipLaunchKernelGGL(gf_if_k_totals, dim3(1), dim3(GF_IF_TOTALS_THREADS), 0, st, (const int32_t*)d_status,
                     (const int64_t*)d_table, n_members, (int64_t*)d_totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_if_copy_from_host_device(const void* h_src, void* d_dst, int64_t nbytes, void* stream) {
  if (nbytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (nbytes == 0) return GF_OK;
  if (!h_src) return fail(GF_ERR_ARG, "null source");
  int dev = 0;
  const int drc = device_of(d_dst, "the destination", dev);
  if (drc != GF_OK) return drc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the destination's device");
  GF_SCAN_HIP(hipMemcpyAsync(d_dst, h_src, (size_t)nbytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return GF_OK;
}

}  // extern "C"
