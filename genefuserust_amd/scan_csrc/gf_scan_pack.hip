// libgfpack.so: the outputs of K scans and their names packed into one block on the device (include/gf_scan_pack.h).
// It takes no gf_index and finds its device from the block's pointer.
#include "gf_pk_kernels.h"
#include "gf_scan_host.h"

namespace {

int64_t round_piece(int64_t bytes) { return (bytes + GF_PK_PIECE - 1) & ~(int64_t)(GF_PK_PIECE - 1); }

// The workspace: the starts of the body's parts (gf_pk_k_plan).
struct Layout {
  size_t o_start = 0;
  size_t bytes = 0;
};

Layout layout(int64_t k) {
  Layout L;
  size_t off = 0;
  L.o_start = take(off, ((size_t)GF_PK_ENTRIES(k) + 1) * sizeof(int64_t));
  L.bytes = off + 256;  // (room to align the caller's base)
  return L;
}

}  // namespace

extern "C" {

int64_t gf_pk_block_bytes(int64_t k, int64_t records, int64_t read_bytes, int64_t name_bytes) {
  if (k < 0 || records < 0 || read_bytes < 0 || name_bytes < 0) return 0;
  return GF_PK_HEADER_BYTES(k) + records * (int64_t)sizeof(gf_pair_hit) + 2 * round_piece(read_bytes) +
         round_piece(8 * (records + k)) + round_piece(name_bytes);
}

int64_t gf_pk_workspace_bytes(int64_t k) { return k < 0 ? 0 : (int64_t)layout(k).bytes; }

const char* gf_pk_last_error(void) { return g_err.c_str(); }

int gf_pk_pack_device(const void* d_scans, int64_t k, void* d_workspace, int64_t workspace_bytes, void* d_block,
                      int64_t block_bytes, void* stream) {
  // every check before the device is touched
  if (k < 1 || k > GF_PK_MAX_SCANS) return fail(GF_ERR_ARG, "the number of scans is not in 1 .. 1024");
  if (workspace_bytes < 0 || block_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (!d_scans) return fail(GF_ERR_ARG, "null scans");
  if (!d_block || !d_workspace) return fail(GF_ERR_ARG, "null block or workspace");
  if ((uintptr_t)d_block & (GF_PK_PIECE - 1)) return fail(GF_ERR_ARG, "the block is not 16-byte aligned");
  const Layout L = layout(k);
  if (workspace_bytes < (int64_t)L.bytes) return fail(GF_ERR_CAPACITY, "workspace smaller than gf_pk_workspace_bytes");
  if (block_bytes < GF_PK_HEADER_BYTES(k)) return fail(GF_ERR_CAPACITY, "the block does not hold its headers, 64 (k + 1) bytes");
  int dev = 0;
  const int drc = device_of(d_block, "the block", dev);
  if (drc != GF_OK) return drc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the block's device");
  hipStream_t st = (hipStream_t)stream;

  const gf_pk_scan* scans = (const gf_pk_scan*)d_scans;
  int64_t* start = (int64_t*)(aligned(d_workspace) + L.o_start);
  int64_t* block = (int64_t*)d_block;
  hipLaunchKernelGGL(gf_pk_k_plan, dim3(1), dim3(GF_SCAN_TOTALS_THREADS), 0, st, scans, (int)k, start, block, block_bytes);
  // the body's size is on the device: the grid covers the pieces the block has room for, up to its cap, and strides
  const int64_t pieces = (block_bytes - GF_PK_HEADER_BYTES(k)) / GF_PK_PIECE;
  const unsigned g_copy = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((pieces + GF_SCAN_THREADS - 1) / GF_SCAN_THREADS, GF_PK_COPY_BLOCKS));
  hipLaunchKernelGGL(gf_pk_k_copy, dim3(g_copy), dim3(GF_SCAN_THREADS), 0, st, scans, (int)k, (const int64_t*)start, block);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
