// The host build of genefuserust_amd/scan_csrc/gf_if_core.h, the decoder the kernels of libgfinflate.so run, as a
// stand-alone program for tests/test_inflate_core.py (g++ -fsanitize=address,undefined):
//
//     test_inflate_core <compressed bytes> <table: int64[n][6]> <out_cap> <output> <statuses: int32[n]>
//
// Like gf_if_inflate_device it fills nothing but each good member's own range of the output, which starts out as 0xA5
// bytes.  Every member is decoded from a heap copy of exactly its payload into a heap block of exactly its text, so that
// the sanitizer sees a byte read or written next to either.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_if_core.h"

namespace {

struct HostSink {
  uint8_t* out;
  void put(uint32_t pos, uint8_t v) { out[pos] = v; }
  void raw(uint32_t pos, const uint8_t* src, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[pos + i] = src[i];
  }
  void copy(uint32_t pos, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos - dist + (i % dist)];
  }
};

std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
  fclose(f);
  return v;
}

void spill(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(p, 1, n, f) != n) {
    perror(path);
    exit(2);
  }
  fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s comp table out_cap out statuses\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> comp = slurp(argv[1]), table_bytes = slurp(argv[2]);
  const int64_t out_cap = atoll(argv[3]);
  const size_t n = table_bytes.size() / (GF_IF_ROW * sizeof(int64_t));
  std::vector<int64_t> table(n * GF_IF_ROW);
  memcpy(table.data(), table_bytes.data(), n * GF_IF_ROW * sizeof(int64_t));
  std::vector<uint8_t> out((size_t)out_cap, 0xA5);
  std::vector<int32_t> status(n, -1);
  uint32_t crc_table[256];
  for (uint32_t i = 0; i < 256; i++) crc_table[i] = gf_if_crc_table_entry(i);

  for (size_t m = 0; m < n; m++) {
    const int64_t* row = &table[m * GF_IF_ROW];
    if (!gf_if_row_ok(row, (int64_t)comp.size(), out_cap)) {
      status[m] = GF_IF_BAD_ROW;
      continue;
    }
    const uint32_t n_bytes = (uint32_t)row[1], isize = (uint32_t)row[3];
    uint8_t* payload = (uint8_t*)malloc(n_bytes ? n_bytes : 1);
    uint8_t* text = (uint8_t*)malloc(isize ? isize : 1);
    memcpy(payload, comp.data() + row[0], n_bytes);
    GfIfTables* T = (GfIfTables*)malloc(sizeof(GfIfTables));
    HostSink sink{text};
    int st = gf_if_inflate_member(payload, n_bytes, isize, *T, sink);
    if (st == GF_IF_OK) {
      uint32_t pieces[GF_IF_LANES];
      for (uint32_t lane = 0; lane < GF_IF_LANES; lane++) pieces[lane] = gf_if_crc_piece(crc_table, text, isize, lane);
      if (gf_if_crc_join(pieces, isize) != (uint32_t)row[4]) st = GF_IF_CRC;
    }
    if (st == GF_IF_OK) memcpy(out.data() + row[2], text, isize);
    status[m] = st;
    free(T);
    free(text);
    free(payload);
  }
  spill(argv[4], out.data(), out.size());
  spill(argv[5], status.data(), status.size() * sizeof(int32_t));
  return 0;
}
