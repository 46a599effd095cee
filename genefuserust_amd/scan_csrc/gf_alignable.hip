// libgfalign.so: the whole-genome alignable filter (include/gf_alignable.h) — seeds of the candidate reads, the entry
// table of the sorted seeds, the scan of a piece of reference text.  It takes no gf_index and finds its device from the
// pointers it is given.
#include "gf_al_kernels.h"
#include "gf_scan_host.h"

#include "../../include/gf_alignable.h"

static_assert(GF_AL_MAX_LEN == GF_MAX_READ_LEN, "a seed's offset has the bits of a read's length");
static_assert(GF_AL_K == GF_AL_WINDOW && GF_AL_LIMIT == GF_AL_UNCOVERED_LIMIT && GF_AL_MAX_READS == GF_AL_READS_MAX &&
                  GF_AL_MIN_FILTER_LOG2 == GF_AL_FILTER_LOG2_MIN && GF_AL_MAX_FILTER_LOG2 == GF_AL_FILTER_LOG2_MAX &&
                  GF_AL_SEPARATOR == GF_AL_SEPARATOR_BYTE,
              "gf_al_core.h and gf_alignable.h name the same constants");

namespace {

// every check of the reads' arrays before the device is touched
int reads_ok(int64_t bases_bytes, const void* d_offsets, int64_t n_reads, int32_t filter_log2_bits) {
  if (bases_bytes < 0 || n_reads < 0) return fail(GF_ERR_ARG, "negative size");
  if (n_reads > GF_AL_MAX_READS) return fail(GF_ERR_CAPACITY, "more than GF_AL_READS_MAX reads in one call");
  if (bases_bytes > (int64_t)GF_AL_MAX_READS * GF_AL_MAX_LEN) return fail(GF_ERR_CAPACITY, "more bases than GF_AL_READS_MAX reads hold");
  if (filter_log2_bits < GF_AL_MIN_FILTER_LOG2 || filter_log2_bits > GF_AL_MAX_FILTER_LOG2)
    return fail(GF_ERR_ARG, "filter_log2_bits outside GF_AL_FILTER_LOG2_MIN .. GF_AL_FILTER_LOG2_MAX");
  if (n_reads > 0 && !d_offsets) return fail(GF_ERR_ARG, "null offsets");
  return GF_OK;
}

unsigned blocks_for(int64_t items, int64_t per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, GF_AL_MAX_BLOCKS));
}

}  // namespace

extern "C" {

const char* gf_al_last_error(void) { return g_err.c_str(); }

int64_t gf_al_filter_bytes(int32_t filter_log2_bits) {
  if (filter_log2_bits < GF_AL_MIN_FILTER_LOG2 || filter_log2_bits > GF_AL_MAX_FILTER_LOG2) return 0;
  return (int64_t)1 << (filter_log2_bits - 3);
}

int64_t gf_al_bucket_bytes(void) { return (((int64_t)1 << GF_AL_BUCKET_BITS) + 1) * (int64_t)sizeof(int32_t); }

int64_t gf_al_flag_bytes(int64_t n_reads) { return n_reads < 0 ? 0 : (n_reads + 31) / 32 * (int64_t)sizeof(uint32_t); }

int gf_al_seeds_device(const void* d_bases, int64_t bases_bytes, const void* d_offsets, int64_t n_reads, void* d_strands,
                       void* d_seeds, void* d_filter, int32_t filter_log2_bits, void* stream) {
  if (const int rc = reads_ok(bases_bytes, d_offsets, n_reads, filter_log2_bits)) return rc;
  if (!d_filter) return fail(GF_ERR_ARG, "null filter");
  if (bases_bytes > 0 && (!d_bases || !d_strands || !d_seeds)) return fail(GF_ERR_ARG, "null bases, strands or seeds");
  int dev = 0;
  if (const int rc = device_of(d_filter, "the filter", dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the filter's device");
  GF_SCAN_HIP(hipMemsetAsync(d_filter, 0, (size_t)gf_al_filter_bytes(filter_log2_bits), (hipStream_t)stream));
  if (n_reads == 0 || bases_bytes == 0) return GF_OK;
  hipLaunchKernelGGL(gf_al_k_fill, dim3(blocks_for(2 * bases_bytes, GF_AL_THREADS)), dim3(GF_AL_THREADS), 0,
                     (hipStream_t)stream, (int64_t*)d_seeds, 2 * bases_bytes);
  GF_SCAN_HIP(hipGetLastError());
  // the grid is capped and strides over the reads, a workgroup each
  hipLaunchKernelGGL(gf_al_k_seeds, dim3(blocks_for(n_reads, 1)), dim3(GF_AL_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)d_bases, bases_bytes, (const int64_t*)d_offsets, n_reads, (uint8_t*)d_strands,
                     (int64_t*)d_seeds, (uint32_t*)d_filter, filter_log2_bits);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_al_index_device(const void* d_seeds, int64_t n_slots, void* d_bucket_start, void* stream) {
  if (n_slots < 0) return fail(GF_ERR_ARG, "negative size");
  if (n_slots > 2 * (int64_t)GF_AL_MAX_READS * GF_AL_MAX_LEN) return fail(GF_ERR_CAPACITY, "more slots than GF_AL_READS_MAX reads have");
  if (!d_bucket_start) return fail(GF_ERR_ARG, "null bucket starts");
  if (n_slots > 0 && !d_seeds) return fail(GF_ERR_ARG, "null seeds");
  int dev = 0;
  if (const int rc = device_of(d_bucket_start, "the bucket starts", dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the bucket starts' device");
  hipLaunchKernelGGL(gf_al_k_index, dim3(blocks_for(n_slots + 1, GF_AL_THREADS)), dim3(GF_AL_THREADS), 0,
                     (hipStream_t)stream, (const int64_t*)d_seeds, n_slots, (int32_t*)d_bucket_start);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

int gf_al_scan_device(const void* d_text, int64_t text_bytes, const void* d_strands, int64_t bases_bytes,
                      const void* d_offsets, int64_t n_reads, const void* d_seeds, const void* d_bucket_start,
                      const void* d_filter, int32_t filter_log2_bits, void* d_flags, void* stream) {
  if (text_bytes < 0) return fail(GF_ERR_ARG, "negative size");
  if (const int rc = reads_ok(bases_bytes, d_offsets, n_reads, filter_log2_bits)) return rc;
  if (text_bytes < GF_AL_K || n_reads == 0 || bases_bytes == 0) return GF_OK;   // nothing can be alignable
  if (!d_text) return fail(GF_ERR_ARG, "null text");
  if ((uintptr_t)d_text % 16) return fail(GF_ERR_ARG, "the text is not aligned to 16 bytes");
  if (!d_strands || !d_seeds || !d_bucket_start || !d_filter || !d_flags)
    return fail(GF_ERR_ARG, "null strands, seeds, bucket starts, filter or flags");
  int dev = 0;
  if (const int rc = device_of(d_text, "the text", dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return fail(GF_ERR_HIP, "cannot select the text's device");
  // the grid is capped and strides over the text, GF_AL_SCAN_TILE positions a workgroup and round
  hipLaunchKernelGGL(gf_al_k_scan, dim3(blocks_for(text_bytes, GF_AL_SCAN_TILE)), dim3(GF_AL_THREADS), 0,
                     (hipStream_t)stream, (const uint8_t*)d_text, text_bytes, (const uint8_t*)d_strands, bases_bytes,
                     (const int64_t*)d_offsets, n_reads, (const int64_t*)d_seeds, 2 * bases_bytes,
                     (const int32_t*)d_bucket_start, (const uint32_t*)d_filter, filter_log2_bits, (uint32_t*)d_flags);
  GF_SCAN_HIP(hipGetLastError());
  return GF_OK;
}

}  // extern "C"
