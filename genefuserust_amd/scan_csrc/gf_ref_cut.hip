// libgfrefcut.so: the gene slices of a reference FASTA, cut on the device chunk by chunk (include/gf_ref_cut.h).  It
// takes no gf_index — none exists while the reference is cut — and finds its device from the pointers it is given.
#include "gf_rc_kernels.h"
#include "gf_scan_host.h"

namespace {

// The workspace of gf_rc_index_device: the tiles' counts and where each tile's records start.
struct Layout {
  size_t o_gt = 0, o_keep = 0, o_gt_off = 0;
  size_t bytes = 0;
};

int64_t tiles_of(int64_t head, int64_t text_bytes) {
  return text_bytes <= 0 ? 0 : (head + text_bytes + GF_RC_TILE - 1) / GF_RC_TILE;
}

Layout layout(int64_t text_bytes) {
  Layout L;
  const size_t nt = (size_t)tiles_of(GF_RC_PIECE - 1, text_bytes);
  size_t off = 0;
  L.o_gt = take(off, nt * sizeof(uint32_t));
  L.o_keep = take(off, nt * sizeof(uint32_t));
  L.o_gt_off = take(off, nt * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

GfRcText text_of(const void* d_text, int64_t text_bytes) {
  const uintptr_t p = (uintptr_t)d_text;
  return GfRcText{(const uint8_t*)(p & ~(uintptr_t)(GF_RC_PIECE - 1)), (int64_t)(p & (GF_RC_PIECE - 1)), text_bytes};
}

}  // namespace

extern "C" {

int64_t gf_rc_tile_bytes(void) { return GF_RC_TILE; }

int64_t gf_rc_tiles(int64_t text_bytes) { return tiles_of(GF_RC_PIECE - 1, text_bytes); }

int64_t gf_rc_workspace_bytes(int64_t text_bytes) { return text_bytes < 0 ? 0 : (int64_t)layout(text_bytes).bytes; }

const char* gf_rc_last_error(void) { return g_err.c_str(); }

int gf_rc_index_device(const void* d_text, int64_t text_bytes, int64_t cap_records, void* d_workspace,
                       int64_t workspace_bytes, void* d_gt_pos, void* d_gt_rank, void* d_name_end, void* d_seq_rank,
                       void* d_name_off, void* d_names, int64_t names_cap, void* d_tile_kept, void* d_totals,
                       void* stream) {
  // every check before the device is touched
  if (text_bytes < 0 || cap_records < 0 || workspace_bytes < 0 || names_cap < 0) return fail(GF_ERR_ARG, "negative size");
  if (!d_totals || !d_tile_kept || !d_name_off) return fail(GF_ERR_ARG, "null totals, tile ranks or name offsets");
  if (text_bytes > 0 && !d_text) return fail(GF_ERR_ARG, "null text");
  if (cap_records > 0 && (!d_gt_pos || !d_gt_rank || !d_name_end || !d_seq_rank)) return fail(GF_ERR_ARG, "null record output");
  if (names_cap > 0 && !d_names) return fail(GF_ERR_ARG, "null names");
  const Layout L = layout(text_bytes);
  if (text_bytes > 0 && (!d_workspace || workspace_bytes < (int64_t)L.bytes))
    return fail(GF_ERR_CAPACITY, "workspace smaller than gf_rc_workspace_bytes");
  int dev = 0;
  const int drc = text_bytes > 0 ? device_of(d_text, "the text", dev) : device_of(d_totals, "the totals", dev);
  if (drc != GF_OK) return drc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the text's device");
  hipStream_t st = (hipStream_t)stream;

  const GfRcText T = text_of(d_text, text_bytes);
  const int64_t nt = tiles_of(T.head, text_bytes);
  uint8_t* ws = text_bytes > 0 ? aligned(d_workspace) : nullptr;
  uint32_t* tile_gt = (uint32_t*)(ws + L.o_gt);
  uint32_t* tile_keep = (uint32_t*)(ws + L.o_keep);
  int64_t* tile_gt_off = (int64_t*)(ws + L.o_gt_off);
  int64_t* tile_kept = (int64_t*)d_tile_kept;
  int64_t* totals = (int64_t*)d_totals;
  int64_t* gt_pos = (int64_t*)d_gt_pos;
  int64_t* gt_rank = (int64_t*)d_gt_rank;
  int64_t* name_off = (int64_t*)d_name_off;
  GF_SCAN_HIP(hipMemsetAsync(totals, 0, 8 * sizeof(int64_t), st));
  if (nt > 0) hipLaunchKernelGGL(gf_rc_k_count, dim3((unsigned)nt), dim3(GF_RC_THREADS), 0, st, T, tile_gt, tile_keep);
  hipLaunchKernelGGL(gf_rc_k_scan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, (const uint32_t*)tile_gt,
                     (const uint32_t*)tile_keep, nt, cap_records, tile_gt_off, tile_kept, totals);
  if (nt > 0 && cap_records > 0)
    hipLaunchKernelGGL(gf_rc_k_scatter, dim3((unsigned)nt), dim3(GF_RC_THREADS), 0, st, T, (const int64_t*)tile_gt_off,
                       (const int64_t*)tile_kept, cap_records, gt_pos, gt_rank);
  // the number of records is on the device: the grids cover cap_records, up to a size that fills the device, and stride
  const int64_t per_block = GF_RC_THREADS / 64;
  const unsigned g_rec = (unsigned)std::max<int64_t>(1, std::min<int64_t>((cap_records + per_block - 1) / per_block, 1024));
  if (cap_records > 0)
    hipLaunchKernelGGL(gf_rc_k_names, dim3(g_rec), dim3(GF_RC_THREADS), 0, st, T, (const int64_t*)gt_pos,
                       (const int64_t*)gt_rank, cap_records, (int64_t*)d_name_end, (int64_t*)d_seq_rank, name_off, totals);
  hipLaunchKernelGGL(gf_rc_k_name_scan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, cap_records, names_cap, name_off,
                     totals);
  if (cap_records > 0)
    hipLaunchKernelGGL(gf_rc_k_name_copy, dim3(g_rec), dim3(GF_RC_THREADS), 0, st, T, (const int64_t*)gt_pos,
                       (const int64_t*)name_off, (const int64_t*)totals, cap_records, (uint8_t*)d_names, names_cap);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_rc_gather_device(const void* d_text, int64_t text_bytes, const void* d_gt_pos, const void* d_seq_rank,
                        int64_t n_records, const void* d_tile_kept, int64_t carried_kept, const void* d_intervals,
                        int64_t n_intervals, void* d_out, int64_t out_cap, void* stream) {
  if (text_bytes < 0 || n_records < 0 || n_intervals < 0 || out_cap < 0 || carried_kept < 0)
    return fail(GF_ERR_ARG, "negative size");
  if (text_bytes > 0 && !d_text) return fail(GF_ERR_ARG, "null text");
  if (!d_tile_kept) return fail(GF_ERR_ARG, "null tile ranks");
  if (n_records > 0 && (!d_gt_pos || !d_seq_rank)) return fail(GF_ERR_ARG, "null record index");
  if (n_intervals > 0 && !d_intervals) return fail(GF_ERR_ARG, "null intervals");
  if (out_cap > 0 && !d_out) return fail(GF_ERR_ARG, "null output pointer");
  int dev = 0;
  const int drc = text_bytes > 0 ? device_of(d_text, "the text", dev) : device_of(d_tile_kept, "the tile ranks", dev);
  if (drc != GF_OK) return drc;
  if (text_bytes == 0 || n_intervals == 0 || out_cap == 0) return GF_OK;  // nothing is wanted, nothing is written
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the text's device");
  const GfRcText T = text_of(d_text, text_bytes);
  const int64_t nt = tiles_of(T.head, text_bytes);
  hipLaunchKernelGGL(gf_rc_k_gather, dim3((unsigned)nt), dim3(GF_RC_THREADS), 0, (hipStream_t)stream, T,
                     (const int64_t*)d_gt_pos, (const int64_t*)d_seq_rank, n_records, (const int64_t*)d_tile_kept,
                     carried_kept, (const gf_rc_interval*)d_intervals, n_intervals, (uint8_t*)d_out, out_cap);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_rc_copy_from_host_device(const void* h_src, void* d_dst, int64_t nbytes, void* stream) {
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
