// libgfdeflate.so: text deflated into BGZF members on the device, and the same members on the host
// (include/gf_deflate.h).  It takes no gf_index and finds its device from the pointers it is given.
#include <vector>

#include "gf_df_kernels.h"
#include "gf_scan_host.h"

#include "../../include/gf_deflate.h"

static_assert(GF_DF_TEXT == GF_DF_TEXT_BYTES && GF_DF_STORED_OVER == GF_DF_STORED_BYTES_OVER,
              "gf_df_core.h and gf_deflate.h name the same sizes");
static_assert(sizeof(GF_DF_EOF_MARKER) - 1 == GF_DF_EOF_MARKER_BYTES, "the end-of-file marker is 28 bytes");

namespace {

// The workspace: per member its slot, its tokens' units and its size.
struct Layout {
  int64_t members = 0;
  size_t o_slots = 0, o_units = 0, o_sizes = 0;
  size_t bytes = 0;
};

int64_t members_of(int64_t text_cap) { return text_cap <= 0 ? 0 : (text_cap + GF_DF_TEXT - 1) / GF_DF_TEXT; }

Layout layout(int64_t text_cap) {
  Layout L;
  L.members = members_of(text_cap);
  size_t off = 0;
  L.o_slots = take(off, (size_t)L.members * GF_DF_SLOT);
  L.o_units = take(off, (size_t)L.members * GF_DF_UNITS_BYTES);
  L.o_sizes = take(off, (size_t)L.members * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

}  // namespace

extern "C" {

const char* gf_df_last_error(void) { return g_err.c_str(); }

int64_t gf_df_members(int64_t text_cap) { return members_of(text_cap); }

int64_t gf_df_out_cap(int64_t text_cap) {
  return text_cap <= 0 ? 0 : text_cap + (int64_t)GF_DF_STORED_OVER * members_of(text_cap);
}

int64_t gf_df_workspace_bytes(int64_t text_cap) { return (int64_t)layout(text_cap).bytes; }

int gf_df_deflate_device(const void* d_text, int64_t text_cap, const void* d_text_bytes, void* d_out, int64_t out_cap,
                         void* d_member_off, void* d_totals, void* d_workspace, int64_t workspace_bytes, void* stream) {
  // every check before the device is touched
  if (text_cap < 0 || out_cap < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (text_cap > (int64_t)1 << 40) return fail(GF_ERR_ARG, "text_cap out of range");
  if (!d_member_off || !d_totals) return fail(GF_ERR_ARG, "null member offsets or totals");
  if (text_cap > 0 && (!d_text || !d_out)) return fail(GF_ERR_ARG, "null text or output with text_cap > 0");
  if (out_cap < gf_df_out_cap(text_cap)) return fail(GF_ERR_CAPACITY, "output smaller than gf_df_out_cap(text_cap)");
  const Layout W = layout(text_cap);
  if (text_cap > 0 && (!d_workspace || workspace_bytes < (int64_t)W.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_df_workspace_bytes(text_cap)");
  int dev = -1;  // (host memory is refused: there is no CPU fallback)
  if (const int drc = device_of(d_member_off, "the member offsets", dev)) return drc;
  if (const int drc = device_of(d_totals, "the totals", dev)) return drc;
  if (d_text_bytes)
    if (const int drc = device_of(d_text_bytes, "the text's length", dev)) return drc;
  if (text_cap > 0) {
    if (const int drc = device_of(d_text, "the text", dev)) return drc;
    if (const int drc = device_of(d_workspace, "the workspace", dev)) return drc;
    if (const int drc = device_of(d_out, "the output", dev)) return drc;
  }
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the output's device");
  hipStream_t st = (hipStream_t)stream;
  if (W.members == 0) {
    GF_SCAN_HIP(hipMemsetAsync(d_member_off, 0, sizeof(int64_t), st));
    return GF_OK;
  }
  uint8_t* slots = aligned(d_workspace) + W.o_slots;
  uint16_t* units = (uint16_t*)(aligned(d_workspace) + W.o_units);
  int64_t* sizes = (int64_t*)(aligned(d_workspace) + W.o_sizes);
  const dim3 grid((unsigned)W.members);
  hipLaunchKernelGGL(gf_df_k_members, grid, dim3(GF_DF_THREADS), 0, st, (const uint8_t*)d_text, text_cap,
                     (const int64_t*)d_text_bytes, slots, units, sizes, (unsigned long long*)d_totals);
  hipLaunchKernelGGL(gf_df_k_scan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, (const int64_t*)sizes,
                     (int64_t*)d_member_off, W.members);
  hipLaunchKernelGGL(gf_df_k_move, grid, dim3(GF_DF_MOVE_THREADS), 0, st, (const uint8_t*)slots, (const int64_t*)sizes,
                     (const int64_t*)d_member_off, (uint8_t*)d_out, out_cap);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_df_member_host(const void* text, int64_t n, void* out, int64_t out_cap, int64_t* out_bytes) {
  if (!text || !out || !out_bytes) return fail(GF_ERR_ARG, "null pointer");
  if (n < 1 || n > (int64_t)GF_DF_TEXT) return fail(GF_ERR_ARG, "a member holds 1 .. 65280 bytes of text");
  if (out_cap < 0) return fail(GF_ERR_ARG, "negative size");
  std::vector<uint8_t> member((size_t)n + GF_DF_STORED_OVER);
  std::vector<uint16_t> units((size_t)n);
  std::vector<uint32_t> table(GF_DF_HASH_SIZE);
  int kind = 0;
  const uint32_t size = gf_df_member((const uint8_t*)text, (uint32_t)n, member.data(), units.data(), table.data(), kind);
  if (out_cap < (int64_t)size) return fail(GF_ERR_CAPACITY, "the member is longer than out_cap (text + 31 always suffices)");
  std::copy(member.begin(), member.begin() + size, (uint8_t*)out);
  *out_bytes = size;
  return GF_OK;
}

}  // extern "C"
