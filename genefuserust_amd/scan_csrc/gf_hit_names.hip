// libgfnames.so: the names of a scan's hit records (include/gf_hit_names.h) and their whole FASTQ records
// (include/gf_hit_records.h), gathered on the device.  Of libgfmatch.so's public ABI it uses gf_index_info_get, for the
// index's device.
#include "gf_hn_kernels.h"
#include "gf_scan_host.h"

namespace {

// The workspace: where each record's name line starts in its text.
struct Layout {
  size_t o_start = 0;
  size_t bytes = 0;
};

Layout layout(int64_t hits_cap) {
  Layout L;
  size_t off = 0;
  L.o_start = take(off, (size_t)hits_cap * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

// The records' workspace: where each span starts in its text, for the two sides a record can have.
Layout records_layout(int64_t hits_cap) {
  Layout L;
  size_t off = 0;
  L.o_start = take(off, (size_t)hits_cap * 2 * sizeof(int64_t));
  L.bytes = off + 256;
  return L;
}

}  // namespace

extern "C" {

int64_t gf_hn_workspace_bytes(int64_t hits_cap) { return hits_cap < 0 ? 0 : (int64_t)layout(hits_cap).bytes; }

const char* gf_hn_last_error(void) { return g_err.c_str(); }

int gf_hn_names_device(const gf_index* idx, const void* d_hits, const void* d_totals, int64_t hits_cap,
                       int64_t pair_id_base, const void* d_l_text, int64_t l_text_bytes, const void* d_l_nl_pos,
                       int64_t l_newlines, const void* d_r_text, int64_t r_text_bytes, const void* d_r_nl_pos,
                       int64_t r_newlines, void* d_workspace, int64_t workspace_bytes, void* d_names,
                       int64_t names_cap, void* d_name_off, void* d_name_totals, void* stream) {
  // every check before the device is touched
  if (hits_cap < 0 || l_text_bytes < 0 || l_newlines < 0 || r_text_bytes < 0 || r_newlines < 0 || names_cap < 0 ||
      workspace_bytes < 0)
    return fail(GF_ERR_ARG, "negative size");
  if (!idx || !d_totals || !d_name_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_name_off) return fail(GF_ERR_ARG, "null name offsets");
  if (hits_cap > 0 && !d_hits) return fail(GF_ERR_ARG, "null records");
  if (hits_cap > 0 && !d_l_text) return fail(GF_ERR_ARG, "null text with records");
  if ((l_newlines > 0 && !d_l_nl_pos) || (r_newlines > 0 && !d_r_nl_pos)) return fail(GF_ERR_ARG, "null newline index");
  if (!d_r_text && (r_text_bytes > 0 || r_newlines > 0)) return fail(GF_ERR_ARG, "a size for the second text, but no text");
  if (names_cap > 0 && !d_names) return fail(GF_ERR_ARG, "null output pointer");
  const Layout L = layout(hits_cap);
  if (hits_cap > 0 && (!d_workspace || workspace_bytes < (int64_t)L.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_hn_workspace_bytes");
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  int64_t* totals = (int64_t*)d_name_totals;
  int64_t* off = (int64_t*)d_name_off;
  GF_SCAN_HIP(hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), st));
  if (hits_cap == 0) {
    GF_SCAN_HIP(hipMemsetAsync(off, 0, sizeof(int64_t), st));
    return GF_OK;
  }

  int64_t* start = (int64_t*)(aligned(d_workspace) + L.o_start);
  const gf_pair_hit* hits = (const gf_pair_hit*)d_hits;
  const int64_t* scan_totals = (const int64_t*)d_totals;
  const GfHnText TL{(const uint8_t*)d_l_text, (const int64_t*)d_l_nl_pos, l_text_bytes, l_newlines};
  const GfHnText TR{(const uint8_t*)d_r_text, (const int64_t*)d_r_nl_pos, r_text_bytes, r_newlines};
  // the number of records is on the device: the grids cover hits_cap, up to a size that fills the device, and stride
  const unsigned g_len = (unsigned)std::min<int64_t>((hits_cap + GF_SCAN_THREADS - 1) / GF_SCAN_THREADS, 1024);
  const int64_t per_block = GF_SCAN_THREADS / 64;
  const unsigned g_copy = (unsigned)std::min<int64_t>((hits_cap + per_block - 1) / per_block, 2048);
  hipLaunchKernelGGL(gf_hn_k_lengths, dim3(g_len), dim3(GF_SCAN_THREADS), 0, st, hits, scan_totals, hits_cap,
                     pair_id_base, TL, TR, start, off, (unsigned long long*)(totals + 3));
  hipLaunchKernelGGL(gf_hn_k_scan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, scan_totals, hits_cap, names_cap, off,
                     totals);
  hipLaunchKernelGGL(gf_hn_k_copy, dim3(g_copy), dim3(GF_SCAN_THREADS), 0, st, hits, scan_totals, hits_cap,
                     TL.text, TR.text, (const int64_t*)start, (const int64_t*)off, (uint8_t*)d_names, names_cap);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int64_t gf_hn_records_workspace_bytes(int64_t hits_cap) {
  return hits_cap < 0 ? 0 : (int64_t)records_layout(hits_cap).bytes;
}

int gf_hn_records_device(const gf_index* idx, const void* d_hits, const void* d_totals, int64_t hits_cap,
                         int64_t pair_id_base, const void* d_l_text, int64_t l_text_bytes, const void* d_l_nl_pos,
                         int64_t l_newlines, const void* d_r_text, int64_t r_text_bytes, const void* d_r_nl_pos,
                         int64_t r_newlines, void* d_workspace, int64_t workspace_bytes, void* d_records,
                         int64_t records_cap, void* d_record_off, void* d_record_totals, void* stream) {
  // every check before the device is touched
  if (hits_cap < 0 || l_text_bytes < 0 || l_newlines < 0 || r_text_bytes < 0 || r_newlines < 0 || records_cap < 0 ||
      workspace_bytes < 0)
    return fail(GF_ERR_ARG, "negative size");
  if (hits_cap > (int64_t)1 << 60) return fail(GF_ERR_ARG, "record capacity out of range");
  if (!idx || !d_totals || !d_record_totals) return fail(GF_ERR_ARG, "null index or totals");
  if (!d_record_off) return fail(GF_ERR_ARG, "null record offsets");
  if (hits_cap > 0 && !d_hits) return fail(GF_ERR_ARG, "null records");
  if (hits_cap > 0 && !d_l_text) return fail(GF_ERR_ARG, "null text with records");
  if ((l_newlines > 0 && !d_l_nl_pos) || (r_newlines > 0 && !d_r_nl_pos)) return fail(GF_ERR_ARG, "null newline index");
  if (!d_r_text && (r_text_bytes > 0 || r_newlines > 0)) return fail(GF_ERR_ARG, "a size for the second text, but no text");
  if (records_cap > 0 && !d_records) return fail(GF_ERR_ARG, "null output pointer");
  const Layout L = records_layout(hits_cap);
  if (hits_cap > 0 && (!d_workspace || workspace_bytes < (int64_t)L.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_hn_records_workspace_bytes");
  gf_index_info info;
  const int irc = gf_index_info_get(idx, &info);
  if (irc != GF_OK) return passed_on("gf_index_info_get", irc);
  DeviceGuard guard(info.device);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the index's device");
  hipStream_t st = (hipStream_t)stream;
  int64_t* totals = (int64_t*)d_record_totals;
  int64_t* off = (int64_t*)d_record_off;
  GF_SCAN_HIP(hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), st));
  if (hits_cap == 0) {
    GF_SCAN_HIP(hipMemsetAsync(off, 0, sizeof(int64_t), st));
    return GF_OK;
  }

  int64_t* start = (int64_t*)(aligned(d_workspace) + L.o_start);
  const gf_pair_hit* hits = (const gf_pair_hit*)d_hits;
  const int64_t* scan_totals = (const int64_t*)d_totals;
  const GfHnText TL{(const uint8_t*)d_l_text, (const int64_t*)d_l_nl_pos, l_text_bytes, l_newlines};
  const GfHnText TR{(const uint8_t*)d_r_text, (const int64_t*)d_r_nl_pos, r_text_bytes, r_newlines};
  const int sides = d_r_text ? 2 : 1;
  // the number of records is on the device: the grids cover the span capacity, up to a size that fills the device
  const int64_t span_cap = hits_cap * sides;
  const unsigned g_spans = (unsigned)std::min<int64_t>((span_cap + GF_SCAN_THREADS - 1) / GF_SCAN_THREADS, 1024);
  const int64_t per_block = GF_SCAN_THREADS / 64;
  const unsigned g_copy = (unsigned)std::min<int64_t>((span_cap + per_block - 1) / per_block, 4096);
  hipLaunchKernelGGL(gf_hn_k_rec_lengths, dim3(g_spans), dim3(GF_SCAN_THREADS), 0, st, hits, scan_totals, hits_cap,
                     pair_id_base, sides, TL, TR, start, off, (unsigned long long*)(totals + 3));
  hipLaunchKernelGGL(gf_hn_k_rec_scan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, scan_totals, hits_cap, sides,
                     records_cap, off, totals);
  hipLaunchKernelGGL(gf_hn_k_rec_copy, dim3(g_copy), dim3(GF_SCAN_THREADS), 0, st, scan_totals, hits_cap, sides,
                     TL.text, TR.text, (const int64_t*)start, (const int64_t*)off, (uint8_t*)d_records, records_cap);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
