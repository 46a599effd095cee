// genefuserust_amd/scan_csrc/gf_at_core.h on the host, for tests/test_adapter_trim_core.py: a stand-alone program that
// is compiled with -fsanitize=address,undefined.  It reads jobs, one per line, and writes one answer line per job:
//
//   pair G sides al ar junk <a hex> <b hex> <the settings>   ->  "<kept a> <how a> <kept b> <how b>"
//       the record by gf_at_decide_pair<G>, the mates' first bases al / ar bytes into their chunk 0; the bytes of a
//       chunk that are not the read's are junk, as a neighbouring record's would be; sides 1: a alone
//   settings single <the settings>                           ->  "ok", or what is wrong, in one word
//
// The settings: overlap min_overlap max_diff diff_percent min_adapter adapter_r1_len adapter_r2_len <adapter_r1 hex>
// <adapter_r2 hex>.  "-" stands for an empty hex string.  Chunks outside 0 .. (a + L - 1) / 16 are never asked for: the
// loader aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_at_core.h"

namespace {

std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

struct Loader {
  const std::vector<uint8_t>& bytes;
  int a;
  uint8_t junk;
  gf_pp_chunk operator()(int c) const {
    const int L = (int)bytes.size();
    if (c < 0 || L == 0 || c > (a + L - 1) / 16) {
      std::fprintf(stderr, "chunk %d of a read of %d bytes at %d was asked for\n", c, L, a);
      std::abort();
    }
    gf_pp_chunk ch = {{0, 0, 0, 0}};
    for (int k = 0; k < 16; ++k) {
      const int p = 16 * c - a + k;
      const uint32_t b = p >= 0 && p < L ? bytes[(size_t)p] : junk;
      ch.w[k >> 2] |= b << (8 * (k & 3));
    }
    return ch;
  }
};

gf_at_settings settings_from(std::istringstream& in) {
  gf_at_settings s;
  std::memset(&s, 0, sizeof s);
  std::string h1, h2;
  in >> s.overlap >> s.min_overlap >> s.max_diff >> s.diff_percent >> s.min_adapter >> s.adapter_r1_len >>
      s.adapter_r2_len >> h1 >> h2;
  const std::vector<uint8_t> a1 = unhex(h1), a2 = unhex(h2);
  for (size_t j = 0; j < a1.size() && j < sizeof s.adapter_r1; ++j) s.adapter_r1[j] = a1[j];
  for (size_t j = 0; j < a2.size() && j < sizeof s.adapter_r2; ++j) s.adapter_r2[j] = a2[j];
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(gf_at_settings) == 156, "gf_at_settings is 156 bytes");
  if (argc != 3) return 2;
  std::ifstream jobs(argv[1]);
  std::ofstream answers(argv[2]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "pair") {
      int G, sides, al, ar, junk;
      std::string ha, hb;
      in >> G >> sides >> al >> ar >> junk >> ha >> hb;
      const gf_at_settings s = settings_from(in);
      if (!in || gf_at_settings_error(s, sides == 1)) return 3;
      const std::vector<uint8_t> a = unhex(ha), b = unhex(hb);
      const Loader la{a, al, (uint8_t)junk}, lb{b, ar, (uint8_t)junk};
      int64_t kept[2] = {-1, -1};
      int how[2] = {-1, -1};
      if (G == 16) gf_at_decide_pair<16>(la, al, (int64_t)a.size(), lb, ar, (int64_t)b.size(), sides, s, kept, how);
      else if (G == 64) gf_at_decide_pair<64>(la, al, (int64_t)a.size(), lb, ar, (int64_t)b.size(), sides, s, kept, how);
      else return 3;
      answers << kept[0] << " " << how[0] << " " << kept[1] << " " << how[1] << "\n";
    } else if (what == "settings") {
      int single;
      in >> single;
      const gf_at_settings s = settings_from(in);
      if (!in) return 3;
      const char* wrong = gf_at_settings_error(s, single != 0);
      std::string word = wrong ? wrong : "ok";
      for (char& ch : word)
        if (ch == ' ') ch = '_';
      answers << word << "\n";
    } else {
      return 3;
    }
  }
  return 0;
}
