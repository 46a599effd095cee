// The host build of genefuserust_amd/scan_csrc/gf_al_core.h, the arithmetic the kernels of libgfalign.so run, as a
// stand-alone program for tests/test_alignable_core.py (g++ -fsanitize=address,undefined):
//
//     test_alignable_core <jobs> <answers>
//
// One job a line, strings in hex ("-" = empty); one line of answers per job:
//     diag <strand> <text> <p>     -> alignable (0 / 1), uncovered positions (-1: the diagonal is refused)
//     strands <read>               -> the reverse complement, in hex
//     keys <strand>                -> per window its key, or -1; then "ok" when every seed unpacks to what was packed
//     read <read> <text>           -> 0 / 1: the scan of one piece for one read as the kernel does it — a seed per valid
//                                     window of both strands, every text position that has a key, the key's seeds, only
//                                     the seeds that open an exact run, the diagonal
// Every string lives in a heap block of exactly its length, so that the sanitizer sees a byte read next to it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_al_core.h"

namespace {

struct Bytes {
  uint8_t* p;
  int64_t n;
  explicit Bytes(const std::string& hex) : n(hex == "-" ? 0 : (int64_t)(hex.size() / 2)) {
    p = (uint8_t*)malloc(n ? n : 1);
    for (int64_t i = 0; i < n; i++) p[i] = (uint8_t)strtol(hex.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
  }
  explicit Bytes(int64_t n_) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_) {}
  ~Bytes() { free(p); }
  Bytes(const Bytes&) = delete;
};

bool scan_read(const Bytes& read, const Bytes& text) {
  if (read.n < GF_AL_K || read.n > GF_AL_MAX_LEN) return false;
  // both strands next to each other, as gf_al_k_seeds lays them out
  Bytes strands(2 * read.n);
  for (int64_t i = 0; i < read.n; i++) {
    strands.p[gf_al_string_start(0, read.n, 0) + i] = read.p[i];
    strands.p[gf_al_string_start(0, read.n, 1) + i] = gf_al_complement(read.p[read.n - 1 - i]);
  }
  std::vector<int64_t> seeds;
  for (int64_t t = 0; t < 2; t++)
    for (int64_t j = 0; j + GF_AL_K <= read.n; j++) {
      uint32_t key;
      if (gf_al_window_key(strands.p + gf_al_string_start(0, read.n, t), j, key)) seeds.push_back(gf_al_seed(key, (uint32_t)t, (uint32_t)j));
    }
  Bytes upper(text.n);
  for (int64_t g = 0; g < text.n; g++) upper.p[g] = gf_al_upper(text.p[g]);
  for (int64_t g = 0; g + GF_AL_K <= text.n; g++) {
    uint32_t key;
    if (!gf_al_window_key(upper.p, g, key)) continue;
    for (const int64_t seed : seeds) {
      if (gf_al_seed_key(seed) != key) continue;
      const int64_t s = gf_al_seed_string(seed), j = gf_al_seed_offset(seed);
      const uint8_t* str = strands.p + gf_al_string_start(0, read.n, s);
      if (!gf_al_opens_run(str, j, text.p, g)) continue;
      if (gf_al_diagonal(str, read.n, text.p, text.n, g - j)) return true;
    }
  }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s jobs answers\n", argv[0]);
    return 2;
  }
  std::ifstream jobs(argv[1]);
  std::ofstream answers(argv[2]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what, s1, s2;
    in >> what;
    if (what == "diag") {
      int64_t p;
      in >> s1 >> s2 >> p;
      Bytes s(s1), text(s2);
      answers << (gf_al_diagonal(s.p, s.n, text.p, text.n, p) ? 1 : 0) << " " << gf_al_uncovered(s.p, s.n, text.p, text.n, p) << "\n";
    } else if (what == "strands") {
      in >> s1;
      Bytes read(s1);
      char hex[3];
      if (read.n == 0) answers << "-";
      for (int64_t i = 0; i < read.n; i++) {
        snprintf(hex, sizeof hex, "%02x", gf_al_complement(read.p[read.n - 1 - i]));
        answers << hex;
      }
      answers << "\n";
    } else if (what == "keys") {
      in >> s1;
      Bytes s(s1);
      bool ok = true;
      for (int64_t j = 0; j + GF_AL_K <= s.n; j++) {
        uint32_t key;
        if (!gf_al_window_key(s.p, j, key)) {
          answers << "-1 ";
          continue;
        }
        answers << key << " ";
        const uint32_t string = (uint32_t)((j * 2654435761u) & 0x7FFFFu), offset = (uint32_t)(j & 0xFFF);
        const int64_t seed = gf_al_seed(key, string, offset);
        ok = ok && seed >= 0 && seed != GF_AL_NO_SEED && gf_al_seed_key(seed) == key && gf_al_seed_string(seed) == string &&
             gf_al_seed_offset(seed) == offset && gf_al_bucket(key) == key >> 14 && gf_al_filter_bit(key, 32) == key &&
             gf_al_filter_bit(key, 16) < 65536u && gf_al_seed(key, 0, 0) <= seed;
      }
      answers << (ok ? "ok" : "bad") << "\n";
    } else if (what == "read") {
      in >> s1 >> s2;
      Bytes read(s1), text(s2);
      answers << (scan_read(read, text) ? 1 : 0) << "\n";
    } else {
      fprintf(stderr, "unknown job: %s\n", line.c_str());
      return 2;
    }
  }
  return jobs.bad() || !answers.flush() ? 2 : 0;
}
