// libgfadapt.so: adapter trimming of FASTQ records in HBM, by pair overlap and by sequence
// (include/gf_adapter_trim.h).  Of libgfmatch.so's public ABI it uses gf_index_info_get, for the index's device.
#include "gf_at_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a pair in gf_at_k_decide (gf_at_kernels.h says why)
constexpr int kLanesPerPair = 16;

// The workspace, as the read filter's: per side the kept bytes of every tile of GF_PP_TILE records, scanned in place to
// where the tile starts, and one entry more for the sum.
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

}  // namespace

extern "C" {

int64_t gf_at_workspace_bytes(int64_t n) { return n < 0 ? 0 : (int64_t)layout(n).bytes; }

const char* gf_at_last_error(void) { return g_err.c_str(); }

int gf_at_trim_device(const gf_index* idx, const gf_at_settings* settings, const void* d_l_bases,
                      const void* d_l_quals, const void* d_l_off, const void* d_r_bases, const void* d_r_quals,
                      const void* d_r_off, int64_t n, void* d_workspace, int64_t workspace_bytes,
                      void* d_l_out_bases, void* d_l_out_quals, void* d_l_out_off, void* d_r_out_bases,
                      void* d_r_out_quals, void* d_r_out_off, void* d_how, void* d_totals, void* stream) {
  // every check before the device is touched
  if (n < 0 || workspace_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > (int64_t)1 << 38) return fail(GF_ERR_ARG, "record count out of range");
  if (!settings) return fail(GF_ERR_ARG, "null settings");
  const bool pairs = d_r_bases || d_r_quals || d_r_off;
  if (const char* wrong = gf_at_settings_error(*settings, !pairs))
    return fail(GF_ERR_ARG, std::string("settings: ") + wrong);
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_l_off || !d_l_out_off) return fail(GF_ERR_ARG, "null offsets");
  if (pairs && !(d_r_bases && d_r_quals && d_r_off)) return fail(GF_ERR_ARG, "some of the mates' pointers are null");
  if (pairs && !d_r_out_off) return fail(GF_ERR_ARG, "null offsets");
  if (n > 0 && (!d_l_bases || !d_l_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  if (n > 0 && (!d_l_out_bases || !d_l_out_quals || (pairs && (!d_r_out_bases || !d_r_out_quals))))
    return fail(GF_ERR_ARG, "null output pointer");
  if (n > 0 && !d_how) return fail(GF_ERR_ARG, "null how");
  const Layout W = layout(n);
  if (n > 0 && (!d_workspace || workspace_bytes < (int64_t)W.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_at_workspace_bytes");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  GF_SCAN_HIP(hipMemsetAsync(d_totals, 0, GF_AT_TOTALS * sizeof(int64_t), st));
  if (n == 0) {
    GF_SCAN_HIP(hipMemsetAsync(d_l_out_off, 0, sizeof(int64_t), st));
    if (pairs) GF_SCAN_HIP(hipMemsetAsync(d_r_out_off, 0, sizeof(int64_t), st));
    return GF_OK;
  }

  const int sides = pairs ? 2 : 1;
  const gf_at_adapter ad_l = gf_at_adapter_planes(settings->adapter_r1, settings->adapter_r1_len);
  const gf_at_adapter ad_r = gf_at_adapter_planes(settings->adapter_r2, settings->adapter_r2_len);
  const GfPpSide L{(const uint8_t*)d_l_bases, (const uint8_t*)d_l_quals, (const int64_t*)d_l_off};
  const GfPpSide R{(const uint8_t*)d_r_bases, (const uint8_t*)d_r_quals, (const int64_t*)d_r_off};
  const GfPpOut out_l{(uint8_t*)d_l_out_bases, (uint8_t*)d_l_out_quals, (int64_t*)d_l_out_off};
  const GfPpOut out_r{(uint8_t*)d_r_out_bases, (uint8_t*)d_r_out_quals, (int64_t*)d_r_out_off};
  int64_t* sum_l = (int64_t*)(aligned(d_workspace) + W.o_sum_l);
  int64_t* sum_r = (int64_t*)(aligned(d_workspace) + W.o_sum_r);
  const dim3 grid((unsigned)W.tiles);
  hipLaunchKernelGGL(gf_at_k_decide<kLanesPerPair>, grid, dim3(GF_SCAN_THREADS), 0, st, *settings, ad_l, ad_r, L, R,
                     sides, n, out_l, out_r, sum_l, sum_r, (uint8_t*)d_how, (unsigned long long*)d_totals);
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

}  // extern "C"
