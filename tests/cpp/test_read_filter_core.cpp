// genefuserust_amd/scan_csrc/gf_pp_core.h on the host, for tests/test_read_filter_core.py: a stand-alone program that
// is compiled with -fsanitize=address,undefined.  It reads jobs, one per line, and writes one answer line per job:
//
//   read G ab aq junk_b junk_q <bases hex> <quals hex> <the seven settings>   ->  "<kept length> <reason>"
//       the read by gf_pp_decide_read<G>, its first base ab bytes and its first quality aq bytes into chunk 0; the
//       bytes of a chunk that are not the read's are junk_b / junk_q, as a neighbouring record's would be
//   pair <reason> <reason>                                                     ->  the two reasons after the pair rule
//   settings <the seven settings>                                              ->  "ok", or what is wrong, in one word
//
// "-" stands for an empty hex string.  Chunks outside 0 .. (a + L - 1) / 16 are never asked for: the loader aborts.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_pp_core.h"

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

gf_pp_settings settings_from(std::istringstream& in) {
  gf_pp_settings s;
  in >> s.poly_g_min >> s.cut_tail_window >> s.cut_tail_mean >> s.length_required >> s.n_base_limit >>
      s.qualified_phred >> s.unqualified_percent;
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream jobs(argv[1]);
  std::ofstream answers(argv[2]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "read") {
      int G, ab, aq, junk_b, junk_q;
      std::string hb, hq;
      in >> G >> ab >> aq >> junk_b >> junk_q >> hb >> hq;
      const gf_pp_settings s = settings_from(in);
      const std::vector<uint8_t> b = unhex(hb), q = unhex(hq);
      if (b.size() != q.size() || !in) return 3;
      const Loader lb{b, ab, (uint8_t)junk_b}, lq{q, aq, (uint8_t)junk_q};
      int32_t e2 = -1;
      int reason = -1;
      if (G == 16) reason = gf_pp_decide_read<16>(lb, ab, lq, aq, (int32_t)b.size(), s, &e2);
      else if (G == 64) reason = gf_pp_decide_read<64>(lb, ab, lq, aq, (int32_t)b.size(), s, &e2);
      else return 3;
      answers << e2 << " " << reason << "\n";
    } else if (what == "pair") {
      int l, r;
      in >> l >> r;
      gf_pp_pair_rule(l, r);
      answers << l << " " << r << "\n";
    } else if (what == "settings") {
      const gf_pp_settings s = settings_from(in);
      const char* wrong = gf_pp_settings_error(s);
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
