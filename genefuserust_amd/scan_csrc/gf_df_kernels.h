// The kernels of libgfdeflate.so (include/gf_deflate.h): text deflated into BGZF members on the device, one workgroup of
// one wavefront a member.
//
// The encoder is gf_df_core.h, the text the host model runs.  gf_df_k_members keeps a member's text in LDS (at the
// offset its address has modulo 16, so that it arrives in aligned 16-byte loads), walks it in rounds of 64 positions —
// a lane a position: the hash table's candidate and the distance-1 candidate, extended — and takes the tokens greedily;
// the tokens' 16-bit units go to the member's part of the workspace, their symbols are counted in LDS.  The first lane
// builds the codes (GfDfPlan), and the units come back in rounds of 64: a prefix sum of their bit lengths, every lane's
// bits ORed into place in LDS, where the text was.  The finished member goes to its slot of the workspace in 16-byte
// stores; gf_df_k_scan turns the members' sizes into offsets and gf_df_k_move packs the slots back to back.
//
// LDS: 65328 bytes of text or member, 8 KiB of hash table, the plan and the CRC's tables: under 80 KiB, two workgroups a
// CU.  The hash table's inserts are atomicMax of the position, the counts atomicAdd, the bits atomicOr: each gives the
// same memory whatever the order of the lanes.  No lane waits for another but at __syncthreads(), no workgroup for
// another at all; the only global atomics are the adds into d_totals.
#pragma once

#include <hip/hip_runtime.h>

#include "gf_df_core.h"
#include "gf_scan_common.h"

#define GF_DF_THREADS 64
#define GF_DF_MOVE_THREADS 256
#define GF_DF_LDS_BYTES 65328u   // the text and the 15 bytes in front of it in whole 16-byte pieces; the largest member
#define GF_DF_SLOT 65536u        // a member's slot in the workspace
#define GF_DF_UNITS_BYTES (2u * GF_DF_TEXT)
static_assert(GF_DF_THREADS == GF_DF_LANES, "a round is one wavefront");
static_assert(GF_DF_LDS_BYTES % 16u == 0 && GF_DF_LDS_BYTES >= GF_DF_TEXT + 15u + 16u &&
                  GF_DF_LDS_BYTES >= ((GF_DF_MEMBER_MAX + 15u) & ~15u) + 8u && GF_DF_SLOT >= GF_DF_LDS_BYTES,
              "the text at any alignment, and the member with the word behind its last bit, fit the LDS block and the slot");

// the true length of the text: *d_text_bytes cut to [0, text_cap], or text_cap
__device__ __forceinline__ int64_t gf_df_text_bytes(const int64_t* d_text_bytes, int64_t text_cap) {
  if (!d_text_bytes) return text_cap;
  const int64_t v = *d_text_bytes;
  return v < 0 ? 0 : v > text_cap ? text_cap : v;
}

// `bits` bits of `value` ORed in at bit position `at` of the words w (LDS)
__device__ __forceinline__ void gf_df_or_bits(uint32_t* w, uint32_t at, uint32_t value, uint32_t bits) {
  if (bits == 0u) return;
  const uint64_t x = (uint64_t)value << (at & 31u);
  atomicOr(&w[at >> 5], (uint32_t)x);
  if ((uint32_t)(x >> 32) != 0u) atomicOr(&w[(at >> 5) + 1u], (uint32_t)(x >> 32));
}

struct GfDfLdsBits {
  uint32_t* w;
  __device__ void operator()(uint32_t at, uint32_t value, uint32_t bits) { gf_df_or_bits(w, at, value, bits); }
};

// sizes[m]: the bytes of member m in its slot, 0 for a member past the text.
__global__ __launch_bounds__(GF_DF_THREADS) void gf_df_k_members(const uint8_t* __restrict__ d_text, int64_t text_cap,
                                                                  const int64_t* __restrict__ d_text_bytes,
                                                                  uint8_t* __restrict__ slots, uint16_t* __restrict__ units_all,
                                                                  int64_t* __restrict__ sizes,
                                                                  unsigned long long* __restrict__ totals) {
  __shared__ uint4 s_block[GF_DF_LDS_BYTES / 16u];
  __shared__ uint32_t s_hash[GF_DF_HASH_SIZE];
  __shared__ GfDfPlan s_plan;
  __shared__ uint32_t s_crc_table[256];
  __shared__ uint32_t s_pieces[GF_IF_LANES];
  const uint32_t lane = threadIdx.x;
  const int64_t member = blockIdx.x;
  const int64_t total_text = gf_df_text_bytes(d_text_bytes, text_cap);
  const int64_t start = member * (int64_t)GF_DF_TEXT;
  if (start >= total_text) {  // (the whole workgroup: nothing of this member exists)
    if (lane == 0) sizes[member] = 0;
    return;
  }
  const uint32_t n = (uint32_t)(total_text - start < (int64_t)GF_DF_TEXT ? total_text - start : (int64_t)GF_DF_TEXT);
  uint8_t* slot = slots + member * (int64_t)GF_DF_SLOT;
  uint16_t* units = units_all + member * (int64_t)GF_DF_TEXT;

  // the text into LDS, in the aligned 16-byte pieces that hold it
  const uint8_t* src = d_text + start;
  const uint32_t shift = (uint32_t)((uintptr_t)src & 15u);
  const uint4* src16 = (const uint4*)(src - shift);
  const uint32_t pieces = (shift + n + 15u) / 16u;
  for (uint32_t q = lane; q < pieces; q += GF_DF_THREADS) s_block[q] = src16[q];
  for (uint32_t i = lane; i < GF_DF_HASH_SIZE; i += GF_DF_THREADS) s_hash[i] = 0;
  for (uint32_t i = lane; i < GF_DF_NSYM; i += GF_DF_THREADS) s_plan.freq[i] = 0;
  for (uint32_t i = lane; i < 256u; i += GF_DF_THREADS) s_crc_table[i] = gf_if_crc_table_entry(i);
  __syncthreads();
  const uint8_t* text = (const uint8_t*)s_block + shift;
  s_pieces[lane] = gf_if_crc_piece(s_crc_table, text, n, lane);
  __syncthreads();
  const uint32_t crc = gf_if_crc_join(s_pieces, n);

  // the rounds
  uint32_t cur = 0, n_units = 0;
  const uint32_t rounds = (n + GF_DF_LANES - 1u) / GF_DF_LANES;
  const uint64_t below = ((uint64_t)1 << lane) - 1u;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t base = r * GF_DF_LANES, p = base + lane;
    const bool hashed = p + 4u <= n;
    uint32_t h = 0, entry = 0;
    if (hashed) {
      h = gf_df_hash(text, p);
      entry = s_hash[h];
    }
    GfDfMatch m{0, 0};
    if (p < n && p >= cur) m = gf_df_match_at(text, n, p, entry);
    __syncthreads();  // (every lane has read the table of the rounds before)
    if (hashed) atomicMax(&s_hash[h], p + 1u);
    // the greedy walk from the cursor: literals up to the next position with a match, the match, and on behind it
    const uint32_t lim = n - base < GF_DF_LANES ? n - base : GF_DF_LANES;
    const uint64_t matches = __ballot(m.len != 0u);
    uint64_t starts = 0;
    uint32_t c = cur - base;  // (cur >= base: the round before ended at or behind its last position)
    for (uint32_t k = 0; k < GF_DF_LANES; k++) {
      if (c >= lim) break;
      const uint64_t ahead = matches & ~(((uint64_t)1 << c) - 1u);
      const uint32_t at = ahead ? (uint32_t)__builtin_ctzll(ahead) : GF_DF_LANES;
      const uint32_t stop = at < lim ? at : lim;
      starts |= (stop >= 64u ? ~(uint64_t)0 : ((uint64_t)1 << stop) - 1u) & ~(((uint64_t)1 << c) - 1u);
      c = stop;
      if (c < lim) {
        starts |= (uint64_t)1 << c;
        c += (uint32_t)__shfl((int)m.len, (int)c);
      }
    }
    cur = base + c;
    const uint64_t taken = starts & matches;
    if ((starts >> lane) & 1u) {
      const uint32_t at = n_units + (uint32_t)__popcll(starts & below) + (uint32_t)__popcll(taken & below);
      if (m.len != 0u) {
        const uint32_t ul = GF_DF_UNIT_LEN | (m.len - 3u), ud = GF_DF_UNIT_DIST | (m.dist - 1u);
        units[at] = (uint16_t)ul, units[at + 1u] = (uint16_t)ud;
        atomicAdd(&s_plan.freq[gf_df_unit_symbol(ul)], 1u);
        atomicAdd(&s_plan.freq[gf_df_unit_symbol(ud)], 1u);
      } else {
        units[at] = text[p];
        atomicAdd(&s_plan.freq[text[p]], 1u);
      }
    }
    n_units += (uint32_t)__popcll(starts) + (uint32_t)__popcll(taken);
    __syncthreads();  // (the inserts are in the table)
  }
  if (lane == 0) s_plan.freq[GF_DF_EOB] += 1u;
  __syncthreads();

  // the symbols in use by (count, symbol), a lane a symbol; the rest of the plan is the first lane's
  for (uint32_t s = lane; s < GF_DF_NLIT; s += GF_DF_THREADS)
    if (s_plan.freq[s] != 0u) s_plan.order[gf_df_rank(s_plan.freq, GF_DF_NLIT, s)] = (uint16_t)s;
  if (lane < GF_DF_NDIST && s_plan.freq[GF_DF_NLIT + lane] != 0u)
    s_plan.order[GF_DF_NLIT + gf_df_rank(s_plan.freq + GF_DF_NLIT, GF_DF_NDIST, lane)] = (uint16_t)lane;
  __syncthreads();
  if (lane == 0) gf_df_plan(s_plan);
  __syncthreads();
  uint32_t payload;
  const int kind = gf_df_kind(n, s_plan.bits, payload);
  const uint32_t size = GF_DF_HEAD + payload + GF_DF_TAIL;

  if (kind == GF_DF_KIND_STORED) {
    for (uint32_t k = lane; k < size; k += GF_DF_THREADS) slot[k] = gf_df_stored_byte(k, text, n, crc);
  } else {
    // the member is put together where the text was, then leaves in 16-byte stores
    uint32_t* words = (uint32_t*)s_block;
    const uint32_t n_words = (size + 3u) / 4u + 1u;
    for (uint32_t i = lane; i < n_words; i += GF_DF_THREADS) words[i] = 0;
    __syncthreads();
    uint32_t at = 0;
    if (lane == 0) {
      GfDfLdsBits put{words};
      for (uint32_t k = 0; k < GF_DF_HEAD; k++) put(8u * k, gf_df_head_byte(k, size), 8u);
      for (uint32_t k = 0; k < GF_DF_TAIL; k++) put(8u * (size - GF_DF_TAIL + k), gf_df_tail_byte(k, crc, n), 8u);
      at = gf_df_block_header(s_plan, 8u * GF_DF_HEAD, put);
    }
    at = (uint32_t)__shfl((int)at, 0);
    const uint32_t unit_rounds = (n_units + GF_DF_LANES - 1u) / GF_DF_LANES;  // (n_units <= n: at most 1020)
    for (uint32_t r = 0; r < unit_rounds; r++) {
      const uint32_t u = r * GF_DF_LANES + lane;
      uint32_t nbits = 0, value = 0;
      if (u < n_units) value = gf_df_unit_bits(s_plan.code, units[u], nbits);
      uint32_t incl = nbits;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= (uint32_t)o) incl += y;
      }
      gf_df_or_bits(words, at + incl - nbits, value, nbits);
      at += (uint32_t)__shfl((int)incl, 63);
    }
    if (lane == 0) gf_df_or_bits(words, at, s_plan.code[GF_DF_EOB] >> 4, s_plan.code[GF_DF_EOB] & 15u);
    __syncthreads();
    uint4* slot16 = (uint4*)slot;
    for (uint32_t q = lane; q < (size + 15u) / 16u; q += GF_DF_THREADS) slot16[q] = s_block[q];
  }
  if (lane == 0) {
    sizes[member] = size;
    atomicAdd(&totals[0], 1ull);
    atomicAdd(&totals[1], (unsigned long long)n);
    atomicAdd(&totals[2], (unsigned long long)size);
    atomicAdd(&totals[kind == GF_DF_KIND_STORED ? 3 : 4], 1ull);
  }
}

// member_off[0, members]: where each member starts in the output, and the output's bytes.  One block.
__global__ __launch_bounds__(GF_SCAN_TOTALS_THREADS) void gf_df_k_scan(const int64_t* sizes, int64_t* member_off,
                                                                        int64_t members) {
  const long long total = gf_scan_totals_block(sizes, member_off, members);
  if (threadIdx.x == 0) member_off[members] = total;
}

// The slots packed back to back: whole words where the output's address allows, bytes at a member's head and tail —
// never past its own range, the neighbouring members' bytes are next to it.  A slot is read up to 3 bytes past the
// member (inside the slot).
__global__ __launch_bounds__(GF_DF_MOVE_THREADS) void gf_df_k_move(const uint8_t* __restrict__ slots,
                                                                    const int64_t* __restrict__ sizes,
                                                                    const int64_t* __restrict__ member_off,
                                                                    uint8_t* __restrict__ out, int64_t out_cap) {
  const int64_t member = blockIdx.x;
  const uint32_t size = (uint32_t)sizes[member];
  const int64_t off = member_off[member];
  if (size == 0u || size > GF_DF_MEMBER_MAX || off < 0 || off > out_cap - (int64_t)size) return;
  const uint8_t* src = slots + member * (int64_t)GF_DF_SLOT;
  uint8_t* dst = out + off;
  const uint32_t lead = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u, head = lead < size ? lead : size;
  const uint32_t words = (size - head) / 4u, body = head + 4u * words;
  for (uint32_t i = threadIdx.x; i < head; i += GF_DF_MOVE_THREADS) dst[i] = src[i];
  const uint32_t* src32 = (const uint32_t*)src;  // (a slot is 256-byte aligned)
  uint32_t* dst32 = (uint32_t*)(dst + head);
  const uint32_t sh = 8u * (head & 3u);
  for (uint32_t w = threadIdx.x; w < words; w += GF_DF_MOVE_THREADS) {
    const uint32_t q = (head + 4u * w) >> 2;
    const uint32_t lo = src32[q], hi = src32[q + 1u];
    dst32[w] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
  }
  for (uint32_t i = body + threadIdx.x; i < size; i += GF_DF_MOVE_THREADS) dst[i] = src[i];
}
