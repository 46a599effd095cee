// What the host sides of the companion libraries (gf_single_end.hip, gf_multi_csv.hip, gf_hit_names.hip, gf_ref_cut.hip,
// gf_scan_pack.hip) share.  Each library is one translation unit that includes this header once, so everything here is
// file-local, and each library has its own thread-local error string behind its own gf_*_last_error.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/gfmatch.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// a gfmatch call failed: its message becomes ours
int passed_on(const char* what, int rc) { return fail(rc, std::string(what) + ": " + gf_last_error()); }

#define GF_SCAN_HIP(x)                                                                \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) return fail(GF_ERR_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    else ok = true, prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// the device a pointer's memory is on, for the libraries that take no gf_index (libgfrefcut.so, libgfpack.so);
// anything but device memory is refused
int device_of(const void* p, const char* what, int& dev) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(GF_ERR_NO_DEVICE, std::string(what) + " is not device memory (there is no CPU fallback)");
  }
  if (a.type != hipMemoryTypeDevice)
    return fail(GF_ERR_NO_DEVICE, std::string(what) + " is not device memory (there is no CPU fallback)");
  dev = a.device;
  return GF_OK;
}

// Buffers are carved in 256-byte aligned pieces from the caller's base, aligned to 256 bytes first: every layout ends
// with 256 bytes of room for that.
size_t take(size_t& off, size_t bytes) {
  const size_t o = off;
  off += (bytes + 255) & ~(size_t)255;
  return o;
}

uint8_t* aligned(const void* p) { return (uint8_t*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// The retry part of a scan's workspace: R slots of Rb bytes in all, and the scan's scalars.
struct RetryWork {
  int64_t R = 0, Rb = 0;
  size_t o_scal = 0, o_roff = 0, o_rb = 0, o_rq = 0, o_cR = 0, o_mR = 0;

  void carve(size_t& off, int64_t slots, int64_t bytes) {
    R = slots;
    Rb = bytes;
    o_scal = take(off, 256);  // int64: [0] retries, [1] retry bytes, [2] hits, [3] hit bytes, [4] the scan's own
    o_roff = take(off, ((size_t)R + 1) * sizeof(int64_t));
    // the retry reads: the mapping kernels read whole 16-byte chunks around a span (gfmatch.h), inside this workspace
    o_rb = take(off, (size_t)Rb + 64);
    o_rq = take(off, (size_t)Rb + 64);
    o_cR = take(off, (size_t)R);  // the retry pass: counts and matches of the slots
    o_mR = take(off, (size_t)R * 2 * sizeof(gf_seqmatch));
  }
};

// the grid of gf_*_k_retry_tail (256 threads a block) over the R + 1 offsets of the retry slots
unsigned retry_tail_blocks(int64_t R) { return (unsigned)std::min<int64_t>((R + 256) / 256, 1024); }

}  // namespace
