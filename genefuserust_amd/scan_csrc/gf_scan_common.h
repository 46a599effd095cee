// What the scans built on libgfmatch.so's public ABI share on the device (libgfse.so: gf_se_kernels.h, libgfmcsv.so:
// gf_mc_kernels.h): the status of a mapped read, the direction rule, the reverse complement, the block-wide scan, the
// wavefront's copy of a read and the retry slots' tail; and, with libgfnames.so and libgfrefcut.so too, the one-block
// scan of the totals.  Inlined device functions and plain structs only, no kernel: every kernel keeps its library's
// name (gf_se_k_*, gf_mc_k_*, ..), so that a profile tells the libraries apart.
//
// The direction rule and the complement are restated from csrc/gf_pair_kernels.h (gf_dev_required_direction,
// gf_complement_base), which these libraries do not include: a second copy of that header's kernels under the same
// names would make two kernels of one name in a profile.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gfmatch.h"

#define GF_SCAN_THREADS 256          // the per-tile kernels' block: four wavefronts
#define GF_SCAN_TOTALS_THREADS 1024  // the one block that scans the per-tile totals

#define GF_SCAN_NONE 0u
#define GF_SCAN_HIT 1u    // two segments in the required direction: a hit on the read as it is
#define GF_SCAN_RETRY 2u  // two segments, wrong direction: its reverse complement is searched

// Indexer::in_required_direction (indexer.rs:541-608) for a two-segment mapping.
__device__ __forceinline__ bool gf_scan_required_direction(const gf_seqmatch& a, const gf_seqmatch& b,
                                                           const uint8_t* __restrict__ rev, int n_genes) {
  const bool swap = a.seq_start > b.seq_start;
  const gf_seqmatch& left = swap ? b : a;
  const gf_seqmatch& right = swap ? a : b;
  if (left.position > 0 && right.position > 0) return true;
  if (left.position < 0 && right.position < 0) return false;
  const bool lrev = rev && left.contig >= 0 && left.contig < n_genes && rev[left.contig] != 0;
  const bool rrev = rev && right.contig >= 0 && right.contig < n_genes && rev[right.contig] != 0;
  if (lrev && !rrev) return false;
  if (!lrev && rrev) return true;
  if (left.contig < right.contig) return true;
  return false;  // (the reference's same-contig test compares left with itself, :598: never true)
}

// SequenceRead::reverse_complement (read.rs:243-261 over sequence.rs:22-60): complement to UPPER case, anything but
// ACGTacgt -> N.
__device__ __forceinline__ uint8_t gf_scan_complement(uint8_t c) {
  switch (c) {
    case 'A': case 'a': return 'T';
    case 'T': case 't': return 'A';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    default: return 'N';
  }
}

// block-wide exclusive scan of two values at once (GF_SCAN_THREADS = 4 wavefronts): ea / eb the thread's exclusive
// prefix, ta / tb the block's totals
__device__ __forceinline__ void gf_scan_block_scan2(int a, long long b, int* s_a, long long* s_b, int& ea,
                                                    long long& eb, int& ta, long long& tb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int xa = a;
  long long xb = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ya = __shfl_up(xa, o);
    const long long yb = __shfl_up(xb, o);
    if (lane >= o) { xa += ya; xb += yb; }
  }
  if (lane == 63) { s_a[wave] = xa; s_b[wave] = xb; }
  __syncthreads();
  int ba = 0; long long bb = 0;
  ta = 0; tb = 0;
#pragma unroll
  for (int w = 0; w < GF_SCAN_THREADS / 64; ++w) {
    if (w < wave) { ba += s_a[w]; bb += s_b[w]; }
    ta += s_a[w]; tb += s_b[w];
  }
  ea = ba + xa - a;
  eb = bb + xb - b;
  __syncthreads();  // (s_a / s_b are reused by the next scan of the block)
}

// The whole body of the one-block scans (gf_se_k_scan, gf_mc_k_scan, gf_hn_k_scan, gf_rc_k_scan, gf_rc_k_name_scan):
// the exclusive scan of S sequences of n elements, in one pass, by one block of GF_SCAN_TOTALS_THREADS threads.
// Thread t takes a run of `per` consecutive elements (the threads past the last run take none), the runs' sums are
// scanned across the block, and every element's offset is its run's base plus its place in the run.  total[s]: the sum
// of sequence s, in every thread.  out[s] may be in[s] (a scan in place): an element is read before its offset is
// stored, a thread reads and writes its own run only, and no pointer here is __restrict__.
template <int S, typename In>
__device__ __forceinline__ void gf_scan_totals_block(In* const (&in)[S], int64_t* const (&out)[S], int64_t n,
                                                     long long (&total)[S]) {
  __shared__ long long s_w[S][GF_SCAN_TOTALS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per = (n + GF_SCAN_TOTALS_THREADS - 1) / GF_SCAN_TOTALS_THREADS;
  const int64_t t0 = (int64_t)threadIdx.x * per < n ? (int64_t)threadIdx.x * per : n;
  const int64_t t1 = t0 + per < n ? t0 + per : n;
  long long mine[S] = {}, y[S], pos[S];
  for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
    for (int s = 0; s < S; ++s) mine[s] += in[s][t];
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    y[s] = mine[s];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long z = __shfl_up(y[s], o);
      if (lane >= o) y[s] += z;
    }
    if (lane == 63) s_w[s][wave] = y[s];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < S; ++s) {
    long long base = 0;
    total[s] = 0;
    for (int w = 0; w < GF_SCAN_TOTALS_THREADS / 64; ++w) {
      if (w < wave) base += s_w[s][w];
      total[s] += s_w[s][w];
    }
    pos[s] = base + y[s] - mine[s];
  }
  for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const long long v = in[s][t];
      out[s][t] = pos[s];
      pos[s] += v;
    }
  }
}

// ... of one sequence: returns its sum
template <typename In>
__device__ __forceinline__ long long gf_scan_totals_block(In* in, int64_t* out, int64_t n) {
  In* const i1[1] = {in};
  int64_t* const o1[1] = {out};
  long long total[1];
  gf_scan_totals_block(i1, o1, n, total);
  return total[0];
}

// One job of gf_se_k_scan / gf_mc_k_scan, the exclusive scan of per-tile totals by one block.
struct GfScanJob {
  const uint32_t* tile_counts;
  int64_t* tile_offsets;
  int64_t* d_total;
};

// The reads that the lanes in `mask` have to write, one after the other, every read by all 64 lanes of the
// wavefront (lane j: bytes j, j + 64, ..): hits and retries are a few per thousand reads, and a lane that copied
// its own read byte by byte would be alone in its wavefront with one round trip per byte.  revcomp: the read's
// reverse complement, its qualities reversed.
__device__ __forceinline__ void gf_scan_wave_write(uint64_t mask, const uint8_t* b, const uint8_t* q, int len,
                                                   long long out, uint8_t* __restrict__ ob, uint8_t* __restrict__ oq,
                                                   bool revcomp) {
  const int lane = threadIdx.x & 63;
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    const uint8_t* bb = (const uint8_t*)__shfl((unsigned long long)b, l);
    const uint8_t* qq = (const uint8_t*)__shfl((unsigned long long)q, l);
    const int ln = __shfl(len, l);
    const long long o = __shfl(out, l);
#pragma unroll 1
    for (int j = lane; j < ln; j += 64) {
      const int src = revcomp ? ln - 1 - j : j;
      ob[o + j] = revcomp ? gf_scan_complement(bb[src]) : bb[src];
      oq[o + j] = qq[src];
    }
  }
}

// The body of gf_se_k_retry_tail / gf_mc_k_retry_tail: offsets of the unused retry slots (empty reads at the end of
// the retry bytes) and the overflow bit.  Over capacity the whole retry pass is emptied (every offset 0): a partly
// searched batch would look like a result.  first / step: the thread's place in the grid and the grid's size, which
// the kernel computes (blockDim and gridDim fold to the launch's values in a kernel's own body only).
__device__ __forceinline__ void gf_scan_retry_tail(const int64_t* d_n_retry, const int64_t* d_retry_bytes,
                                                   int64_t cap_reads, int64_t cap_bytes, int64_t* r_off,
                                                   int64_t* totals, int64_t first, int64_t step) {
  const int64_t nr = *d_n_retry, nb = *d_retry_bytes;
  const bool over = nr > cap_reads || nb > cap_bytes;
  for (int64_t k = first; k <= cap_reads; k += step) {
    if (over) r_off[k] = 0;
    else if (k >= nr) r_off[k] = nb;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[3] = nr;
    if (over) totals[4] |= 1;
  }
}
