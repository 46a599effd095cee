// libgfumi.so: unique molecular identifiers cut off records in HBM, read from their names, and mixed into the keys of
// the duplicate removal (include/gf_umi.h).  Of libgfmatch.so's public ABI it uses gf_index_info_get, for the index's
// device.
#include <initializer_list>

#include "gf_um_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a record in gf_um_k_decide and gf_um_k_names (gf_um_kernels.h says why)
constexpr int kLanesPerRecord = 16;

// The workspace of the cut, as the read filter's: per side the kept bytes of every tile of GF_PP_TILE records, scanned
// in place to where the tile starts, and one entry more for the sum.
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

}  // namespace

extern "C" {

int64_t gf_um_workspace_bytes(int64_t n) { return n < 0 ? 0 : (int64_t)layout(n).bytes; }

const char* gf_um_last_error(void) { return g_err.c_str(); }

int gf_um_cut_device(const gf_index* idx, const gf_um_settings* settings, const void* d_l_bases, const void* d_l_quals,
                     const void* d_l_off, const void* d_r_bases, const void* d_r_quals, const void* d_r_off, int64_t n,
                     void* d_workspace, int64_t workspace_bytes, void* d_l_out_bases, void* d_l_out_quals,
                     void* d_l_out_off, void* d_r_out_bases, void* d_r_out_quals, void* d_r_out_off, void* d_codes,
                     void* d_totals, void* stream) {
  // every check before the device is touched
  if (n < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = checked_count(n)) return rc;
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!settings) return fail(GF_ERR_ARG, "null settings");
  const gf_um_settings s = *settings;
  if (!gf_um_settings_ok(s.source, s.length, s.skip))
    return fail(GF_ERR_ARG, "settings out of range: an inline source needs 1 <= length <= 32 and 0 <= skip <= 32, the "
                            "name source length 0 and skip 0");
  if (!gf_um_inline_source(s.source))
    return fail(GF_ERR_ARG, "the name source cuts nothing: gf_um_names_device reads the names");
  if (!d_l_off || !d_l_out_off) return fail(GF_ERR_ARG, "null offsets");
  const bool pairs = d_r_bases || d_r_quals || d_r_off;
  if (pairs && !(d_r_bases && d_r_quals && d_r_off)) return fail(GF_ERR_ARG, "some of the mates' pointers are null");
  if (pairs && !d_r_out_off) return fail(GF_ERR_ARG, "null offsets");
  if (!pairs && s.source == GF_UM_READ2) return fail(GF_ERR_ARG, "source read2 with single-end input: there is no R2");
  if (n > 0 && (!d_l_bases || !d_l_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  if (n > 0 && (!d_l_out_bases || !d_l_out_quals || (pairs && (!d_r_out_bases || !d_r_out_quals))))
    return fail(GF_ERR_ARG, "null output pointer");
  if (n > 0 && !d_codes) return fail(GF_ERR_ARG, "null codes");
  const Layout W = layout(n);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)W.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_um_workspace_bytes");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  if (const int drc = device_of(d_totals, "the totals", off_device)) return drc;
  if (const int drc = all_on_device({{d_l_out_off, "the output offsets"}})) return drc;
  if (pairs)
    if (const int drc = all_on_device({{d_r_off, "the mates' offsets"}, {d_r_out_off, "the mates' output offsets"}}))
      return drc;
  if (n > 0) {
    if (const int drc = all_on_device({{d_l_bases, "the bases"}, {d_l_quals, "the qualities"},
                                       {d_l_out_bases, "the output bases"}, {d_l_out_quals, "the output qualities"},
                                       {d_codes, "the codes"}, {d_workspace, "the workspace"}}))
      return drc;
    if (pairs)
      if (const int drc = all_on_device({{d_r_bases, "the mates' bases"}, {d_r_quals, "the mates' qualities"},
                                         {d_r_out_bases, "the mates' output bases"},
                                         {d_r_out_quals, "the mates' output qualities"}}))
        return drc;
  }
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
  const int32_t c = s.length + s.skip;
  const int64_t cut_l = gf_um_takes(s.source, 0) ? c : 0, cut_r = pairs && gf_um_takes(s.source, 1) ? c : 0;
  const GfPpSide L{(const uint8_t*)d_l_bases, (const uint8_t*)d_l_quals, (const int64_t*)d_l_off};
  const GfPpSide R{(const uint8_t*)d_r_bases, (const uint8_t*)d_r_quals, (const int64_t*)d_r_off};
  // what the gather copies from: a record that stays, behind its UMI and spacer
  const GfPpSide from_l{L.bases + cut_l, L.quals + cut_l, L.off};
  const GfPpSide from_r{pairs ? R.bases + cut_r : nullptr, pairs ? R.quals + cut_r : nullptr, R.off};
  const GfPpOut out_l{(uint8_t*)d_l_out_bases, (uint8_t*)d_l_out_quals, (int64_t*)d_l_out_off};
  const GfPpOut out_r{(uint8_t*)d_r_out_bases, (uint8_t*)d_r_out_quals, (int64_t*)d_r_out_off};
  int64_t* sum_l = (int64_t*)(aligned(d_workspace) + W.o_sum_l);
  int64_t* sum_r = (int64_t*)(aligned(d_workspace) + W.o_sum_r);
  const dim3 grid((unsigned)W.tiles);
  hipLaunchKernelGGL(gf_um_k_decide<kLanesPerRecord>, grid, dim3(GF_SCAN_THREADS), 0, st, s, L, R, sides, n, out_l,
                     out_r, sum_l, sum_r, (unsigned long long*)d_codes, (unsigned long long*)d_totals);
  if (pairs)
    hipLaunchKernelGGL(gf_pp_k_scan<2>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  else
    hipLaunchKernelGGL(gf_pp_k_scan<1>, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, sum_l, sum_r, W.tiles, n,
                       out_l.off, out_r.off);
  hipLaunchKernelGGL(gf_pp_k_gather, grid, dim3(GF_SCAN_THREADS), 0, st, from_l, from_r, sides, n, out_l, out_r,
                     (const int64_t*)sum_l, (const int64_t*)sum_r);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_um_names_device(const gf_index* idx, const void* d_text, int64_t text_bytes, const void* d_nl_pos,
                       int64_t newlines, int64_t n, void* d_codes, void* d_totals, void* stream) {
  if (n < 0 || text_bytes < 0 || newlines < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = checked_count(n)) return rc;
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (text_bytes > 0 && !d_text) return fail(GF_ERR_ARG, "null text");
  if (newlines > 0 && !d_nl_pos) return fail(GF_ERR_ARG, "null newline positions");
  if (n > 0 && !d_codes) return fail(GF_ERR_ARG, "null codes");
  int off_device = -1;
  if (const int drc = device_of(d_totals, "the totals", off_device)) return drc;
  if (text_bytes > 0)
    if (const int drc = device_of(d_text, "the text", off_device)) return drc;
  if (n == 0) return GF_OK;
  if (const int drc = all_on_device({{d_codes, "the codes"}})) return drc;
  if (newlines > 0)
    if (const int drc = all_on_device({{d_nl_pos, "the newline positions"}})) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_um_k_names<kLanesPerRecord>, dim3((unsigned)layout(n).tiles), dim3(GF_SCAN_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)d_text, text_bytes, (const int64_t*)d_nl_pos, newlines, n,
                     (unsigned long long*)d_codes, (unsigned long long*)d_totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_um_mix_keys_device(const gf_index* idx, void* d_rec_keys, const void* d_codes, int64_t n, void* stream) {
  if (const int rc = checked_count(n)) return rc;
  if (!idx) return fail(GF_ERR_ARG, "null index");
  if (n > 0 && (!d_rec_keys || !d_codes)) return fail(GF_ERR_ARG, "null record keys or codes");
  if (n == 0) return GF_OK;
  int off_device = -1;
  if (const int drc = device_of(d_rec_keys, "the record keys", off_device)) return drc;
  if (const int drc = device_of(d_codes, "the codes", off_device)) return drc;
  int device = -1;
  if (const int rc = device_of_index(idx, device)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipLaunchKernelGGL(gf_um_k_mix, dim3(blocks_over(n)), dim3(GF_SCAN_THREADS), 0, (hipStream_t)stream,
                     (unsigned long long*)d_rec_keys, (const unsigned long long*)d_codes, n);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
