// libgfcorrect.so: bases inside the overlap of a pair corrected from the mate, in place, on FASTQ records in HBM
// (include/gf_overlap_correct.h).  Of libgfmatch.so's public ABI it uses gf_index_info_get, for the index's device.
#include "gf_oc_kernels.h"
#include "gf_scan_host.h"

namespace {

// lanes that share a pair in gf_oc_k_correct (as in gf_at_k_decide: gf_at_kernels.h says why)
constexpr int kLanesPerPair = 16;

}  // namespace

extern "C" {

const char* gf_oc_last_error(void) { return g_err.c_str(); }

int gf_oc_correct_device(const gf_index* idx, const gf_oc_settings* settings, void* d_l_bases, void* d_l_quals,
                         const void* d_l_off, void* d_r_bases, void* d_r_quals, const void* d_r_off, int64_t n,
                         void* d_insert, void* d_fixed, void* d_totals, void* stream) {
  // every check before the device is touched
  if (n < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > (int64_t)1 << 38) return fail(GF_ERR_ARG, "record count out of range");
  if (!settings) return fail(GF_ERR_ARG, "null settings");
  if (const char* wrong = gf_oc_settings_error(*settings)) return fail(GF_ERR_ARG, std::string("settings: ") + wrong);
  if (!idx || !d_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_l_off) return fail(GF_ERR_ARG, "null offsets");
  if (!d_r_bases && !d_r_quals && !d_r_off) return fail(GF_ERR_ARG, "no mates: the correction is for pairs");
  if (!(d_r_bases && d_r_quals && d_r_off)) return fail(GF_ERR_ARG, "some of the mates' pointers are null");
  if (n > 0 && (!d_l_bases || !d_l_quals)) return fail(GF_ERR_ARG, "null bases or qualities with records");
  int off_device = -1;  // (host memory is refused here, before the index is looked at: there is no CPU fallback)
  if (const int drc = device_of(d_l_off, "the offsets", off_device)) return drc;
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  GF_SCAN_HIP(hipMemsetAsync(d_totals, 0, GF_OC_TOTALS * sizeof(int64_t), st));
  if (n == 0) return GF_OK;

  const GfOcSide L{(uint8_t*)d_l_bases, (uint8_t*)d_l_quals, (const int64_t*)d_l_off};
  const GfOcSide R{(uint8_t*)d_r_bases, (uint8_t*)d_r_quals, (const int64_t*)d_r_off};
  const dim3 grid((unsigned)((n + GF_PP_TILE - 1) / GF_PP_TILE));
  hipLaunchKernelGGL(gf_oc_k_correct<kLanesPerPair>, grid, dim3(GF_SCAN_THREADS), 0, st, *settings,
                     gf_oc_search_settings(*settings), L, R, n, (int32_t*)d_insert, (int32_t*)d_fixed,
                     (unsigned long long*)d_totals);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
