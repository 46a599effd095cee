// libgfreport.so: the report tail in bulk (include/gf_report.h) — filter reasons and refined breaks on the device,
// first fit on the host.  It takes no gf_index and finds its device from the pointers it is given.
#include "gf_rp_kernels.h"
#include "gf_scan_host.h"

#include <unordered_map>

#include "../../include/gf_report.h"

static_assert(GF_RP_MAX_LEN == GF_MAX_READ_LEN, "a read's symbols fit the carry vectors of a wavefront");
static_assert(GF_RP_OK == GF_RP_STATUS_OK && GF_RP_OUT_OF_DOMAIN == GF_RP_STATUS_OUT_OF_DOMAIN &&
                  GF_RP_BAD_ROW == GF_RP_STATUS_BAD_ROW && GF_RP_BAD_BREAK == GF_RP_REASON_BAD_BREAK &&
                  GF_RP_BAD_READ == GF_RP_REASON_BAD_READ,
              "gf_rp_core.h and gf_report.h name the same statuses and reasons");

namespace {

struct Cell {
  int64_t l, r;
  bool operator==(const Cell& o) const { return l == o.l && r == o.r; }
};
struct CellHash {
  size_t operator()(const Cell& c) const {
    return (size_t)(((uint64_t)c.l * 0x9E3779B97F4A7C15ull) ^ (((uint64_t)c.r + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full));
  }
};

// every check before the device is touched; dev: the device of the matches
int matches_ok(const void* d_bases, int64_t bases_bytes, const void* d_offsets, const void* d_matches, int64_t n, int& dev) {
  if (bases_bytes < 0 || n < 0) return fail(GF_ERR_ARG, "negative size");
  if (n > 0 && (!d_offsets || !d_matches)) return fail(GF_ERR_ARG, "null offsets or matches");
  if (bases_bytes > 0 && !d_bases) return fail(GF_ERR_ARG, "null bases");
  return n > 0 ? device_of(d_matches, "the matches", dev) : GF_OK;
}

}  // namespace

extern "C" {

const char* gf_rp_last_error(void) { return g_err.c_str(); }

int gf_rp_filter_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, const void* d_matches, int64_t n,
                        int32_t deletion_threshold, void* d_reason, void* stream) {
  int dev = 0;
  if (const int rc = matches_ok(d_bases, bases_bytes, d_offsets, d_matches, n, dev)) return rc;
  if (n == 0) return GF_OK;
  if (!d_reason) return fail(GF_ERR_ARG, "null reasons");
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the matches' device");
  // the grid is capped and strides over the matches, a wavefront each
  const int64_t per_block = GF_RP_FILTER_THREADS / 64;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + per_block - 1) / per_block, GF_RP_FILTER_MAX_BLOCKS);
  hipLaunchKernelGGL(gf_rp_k_filter, dim3(blocks), dim3(GF_RP_FILTER_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)d_bases, bases_bytes, (const int64_t*)d_offsets, (const gf_readmatch*)d_matches, n,
                     deletion_threshold, (int32_t*)d_reason);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_rp_adjust_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, const void* d_matches,
                        const void* d_cluster, int64_t n, const void* d_refs, int64_t refs_bytes,
                        const void* d_ref_offsets, int64_t n_clusters, void* d_out, void* stream) {
  int dev = 0;
  if (refs_bytes < 0 || n_clusters < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = matches_ok(d_bases, bases_bytes, d_offsets, d_matches, n, dev)) return rc;
  if (n == 0) return GF_OK;
  if (!d_cluster || !d_out) return fail(GF_ERR_ARG, "null clusters or output");
  if (n_clusters > 0 && !d_ref_offsets) return fail(GF_ERR_ARG, "null reference offsets");
  if (refs_bytes > 0 && !d_refs) return fail(GF_ERR_ARG, "null references");
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the matches' device");
  // the grid is capped and strides over the matches, a workgroup each
  const unsigned blocks = (unsigned)std::min<int64_t>(n, GF_RP_ADJUST_MAX_BLOCKS);
  hipLaunchKernelGGL(gf_rp_k_adjust, dim3(blocks), dim3(GF_RP_ADJUST_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)d_bases, bases_bytes, (const int64_t*)d_offsets, (const gf_readmatch*)d_matches,
                     (const int32_t*)d_cluster, n, (const uint8_t*)d_refs, refs_bytes, (const int64_t*)d_ref_offsets,
                     n_clusters, (int32_t*)d_out);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_rp_first_fit(const int32_t* lp, const int32_t* rp, const int64_t* group_off, int64_t n_groups,
                    int64_t* founder_out) {
  if (n_groups < 0) return fail(GF_ERR_ARG, "negative size");
  if (n_groups == 0) return GF_OK;
  if (!group_off) return fail(GF_ERR_ARG, "null group offsets");
  if (group_off[0] != 0) return fail(GF_ERR_ARG, "group offsets start at 0");
  for (int64_t g = 0; g < n_groups; g++)
    if (group_off[g + 1] < group_off[g]) return fail(GF_ERR_ARG, "group offsets decrease");
  if (group_off[n_groups] > 0 && (!lp || !rp || !founder_out)) return fail(GF_ERR_ARG, "null positions or output");
  // Clusters are made in processing order, so the first cluster that holds a supporting match is the smallest founder
  // among the earlier matches within 3 on both sides: the minimum over 49 cells of the smallest founder seen in each.
  std::unordered_map<Cell, int64_t, CellHash> smallest;
  for (int64_t g = 0; g < n_groups; g++) {
    smallest.clear();
    for (int64_t i = group_off[g]; i < group_off[g + 1]; i++) {
      int64_t founder = i;
      for (int64_t a = -3; a <= 3; a++)
        for (int64_t b = -3; b <= 3; b++) {
          const auto it = smallest.find(Cell{(int64_t)lp[i] + a, (int64_t)rp[i] + b});
          if (it != smallest.end() && it->second < founder) founder = it->second;
        }
      founder_out[i] = founder;
      const auto ins = smallest.emplace(Cell{(int64_t)lp[i], (int64_t)rp[i]}, founder);
      if (!ins.second && founder < ins.first->second) ins.first->second = founder;
    }
  }
  return GF_OK;
}

}  // extern "C"
