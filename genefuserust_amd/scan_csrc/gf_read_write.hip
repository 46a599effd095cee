// libgfwrite.so: the records that pass the preparation steps formatted as FASTQ text in HBM (include/gf_read_write.h).
// Of libgfmatch.so's public ABI it uses gf_index_info_get, for the index's device.
#include <initializer_list>

#include "gf_rw_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a record in gf_rw_k_format (gf_rw_kernels.h says why); the plain gather takes a wavefront, as
// gf_pp_k_gather does
constexpr int kLanesPerRecord = 16;
constexpr int kLanesPerRecordBytes = 64;

// The workspace: per side the output bytes of every tile of GF_PP_TILE records, scanned in place to where the tile
// starts, and one entry more for the sum; and per side and record the length of the name line's first token.
struct Layout {
  int64_t tiles = 0;
  size_t o_sum_l = 0, o_sum_r = 0, o_tok = 0;
  size_t bytes = 0;
};

Layout layout(int64_t n) {
  Layout L;
  L.tiles = (n + GF_PP_TILE - 1) / GF_PP_TILE;
  size_t off = 0;
  L.o_sum_l = take(off, ((size_t)L.tiles + 1) * sizeof(int64_t));
  L.o_sum_r = take(off, ((size_t)L.tiles + 1) * sizeof(int64_t));
  L.o_tok = take(off, 2 * (size_t)n * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

int checked_count(int64_t n) {
  if (n < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > (int64_t)1 << 38) return fail(GF_ERR_ARG, "record count out of range");
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

// every pointer a kernel of the call dereferences, host memory refused: (pointer, what it is called in the message)
struct Named {
  const void* p;
  const char* what;
};

int all_on_device(std::initializer_list<Named> pointers) {
  int device = -1;
  for (const Named& x : pointers)
    if (const int drc = device_of(x.p, x.what, device)) return drc;
  return GF_OK;
}

// the checks of one side that need no device: NULLs and sizes
int checked_side(const gf_rw_side& x, int64_t n, bool tagged) {
  if (x.text_bytes < 0 || x.newlines < 0 || x.out_cap < 0) return fail(GF_ERR_ARG, "negative size");
  if (x.text_bytes > 0 && !x.d_text) return fail(GF_ERR_ARG, "null text");
  if (x.newlines > 0 && !x.d_nl_pos) return fail(GF_ERR_ARG, "null newline positions");
  if (!x.d_off || !x.d_out_off) return fail(GF_ERR_ARG, "null offsets");
  if (n > 0 && (!x.d_bases || !x.d_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  if (n > 0 && tagged && (!x.d_pre_bases || !x.d_pre_off))
    return fail(GF_ERR_ARG, "a tag needs the pre-cut bases and offsets of every side");
  if (!x.d_out_text) return fail(GF_ERR_ARG, "null output text");
  if (x.out_cap < gf_rw_capacity(x.text_bytes, n))
    return fail(GF_ERR_CAPACITY, "output smaller than GF_RW_CAPACITY(text_bytes, n)");
  return GF_OK;
}

int side_on_device(const gf_rw_side& x, int64_t n, bool tagged) {
  if (const int drc = all_on_device({{x.d_off, "the offsets"}, {x.d_out_off, "the output offsets"},
                                     {x.d_out_text, "the output text"}}))
    return drc;
  if (x.text_bytes > 0)
    if (const int drc = all_on_device({{x.d_text, "the text"}})) return drc;
  if (x.newlines > 0)
    if (const int drc = all_on_device({{x.d_nl_pos, "the newline positions"}})) return drc;
  if (n > 0) {
    if (const int drc = all_on_device({{x.d_bases, "the bases"}, {x.d_quals, "the qualities"}})) return drc;
    if (tagged)
      if (const int drc = all_on_device({{x.d_pre_bases, "the pre-cut bases"}, {x.d_pre_off, "the pre-cut offsets"}}))
        return drc;
  }
  return GF_OK;
}

gf_rw_in as_input(const gf_rw_side& x) {
  return gf_rw_in{(const uint8_t*)x.d_text,  x.text_bytes,          (const int64_t*)x.d_nl_pos,
                  x.newlines,                (const uint8_t*)x.d_bases, (const uint8_t*)x.d_quals,
                  (const int64_t*)x.d_off,   (const uint8_t*)x.d_pre_bases, (const int64_t*)x.d_pre_off};
}

}  // namespace

extern "C" {

int64_t gf_rw_workspace_bytes(int64_t n) { return n < 0 ? 0 : (int64_t)layout(n).bytes; }

const char* gf_rw_last_error(void) { return g_err.c_str(); }

int gf_rw_format_device(const gf_index* idx, const gf_rw_settings* settings, const gf_rw_side* left,
                        const gf_rw_side* right, int64_t n, void* d_workspace, int64_t workspace_bytes, void* d_totals,
                        void* stream) {
  // every check before the device is touched
  if (n < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = checked_count(n)) return rc;
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!settings) return fail(GF_ERR_ARG, "null settings");
  if (!left) return fail(GF_ERR_ARG, "null side");
  const gf_rw_settings s = *settings;
  if (!gf_rw_settings_ok(s.umi_source, s.umi_length, s.gather))
    return fail(GF_ERR_ARG, "settings out of range: a tag needs an inline umi_source and 1 <= umi_length <= 32, no tag "
                            "umi_source 0 and umi_length 0; gather is GF_RW_WIDE or GF_RW_BYTES");
  const bool pairs = right != nullptr, tagged = gf_um_inline_source(s.umi_source);
  if (!pairs && s.umi_source == GF_UM_READ2)
    return fail(GF_ERR_ARG, "umi_source read2 with single-end input: there is no R2");
  if (const int rc = checked_side(*left, n, tagged)) return rc;
  if (pairs)
    if (const int rc = checked_side(*right, n, tagged)) return rc;
  const Layout W = layout(n);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)W.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_rw_workspace_bytes");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_totals, "the totals", off_device)) return drc;
  if (const int drc = side_on_device(*left, n, tagged)) return drc;
  if (pairs)
    if (const int drc = side_on_device(*right, n, tagged)) return drc;
  if (n > 0)
    if (const int drc = all_on_device({{d_workspace, "the workspace"}})) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    GF_SCAN_HIP(hipMemsetAsync(left->d_out_off, 0, sizeof(int64_t), st));
    if (pairs) GF_SCAN_HIP(hipMemsetAsync(right->d_out_off, 0, sizeof(int64_t), st));
    return GF_OK;
  }
  const int sides = pairs ? 2 : 1;
  GfRwSides in;
  in.in[0] = as_input(*left);
  in.in[1] = pairs ? as_input(*right) : gf_rw_in{};
  const GfRwOut out_l{(uint8_t*)left->d_out_text, left->out_cap, (int64_t*)left->d_out_off};
  const GfRwOut out_r = pairs ? GfRwOut{(uint8_t*)right->d_out_text, right->out_cap, (int64_t*)right->d_out_off}
                              : GfRwOut{nullptr, 0, nullptr};
  int64_t* sum_l = (int64_t*)(aligned(d_workspace) + W.o_sum_l);
  int64_t* sum_r = (int64_t*)(aligned(d_workspace) + W.o_sum_r);
  int64_t* tok = (int64_t*)(aligned(d_workspace) + W.o_tok);
  const dim3 grid((unsigned)W.tiles), block(GF_SCAN_THREADS);
  hipLaunchKernelGGL(gf_rw_k_sizes, grid, block, 0, st, s, in, sides, n, out_l.off, out_r.off, sum_l, sum_r, tok,
                     (unsigned long long*)d_totals);
  if (pairs)
    hipLaunchKernelGGL(gf_pp_k_scan<2>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  else
    hipLaunchKernelGGL(gf_pp_k_scan<1>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  if (s.gather == GF_RW_WIDE)
    hipLaunchKernelGGL((gf_rw_k_format<kLanesPerRecord, true>), grid, block, 0, st, s, in, sides, n, out_l, out_r,
                       (const int64_t*)sum_l, (const int64_t*)sum_r, (const int64_t*)tok);
  else
    hipLaunchKernelGGL((gf_rw_k_format<kLanesPerRecordBytes, false>), grid, block, 0, st, s, in, sides, n, out_l,
                       out_r, (const int64_t*)sum_l, (const int64_t*)sum_r, (const int64_t*)tok);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
