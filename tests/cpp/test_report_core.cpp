// The host build of genefuserust_amd/scan_csrc/gf_rp_core.h, the arithmetic the kernels of libgfreport.so run, as a
// stand-alone program for tests/test_report_core.py (g++ -fsanitize=address,undefined):
//
//     test_report_core <jobs> <answers>
//
// One job a line, strings in hex ("-" = empty); one line of answers per job:
//     ed <a> <b>                                                          -> distance
//     filter <seq> <break> <ld> <rd> <lp> <rp> <lcontig> <rcontig> <thr>  -> reason
//     adjust <seq> <break> <left ref> <right ref>                         -> shift left_distance right_distance status
// Every string lives in a heap block of exactly its length, so that the sanitizer sees a byte read next to it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../genefuserust_amd/scan_csrc/gf_rp_core.h"

namespace {

struct Bytes {
  uint8_t* p;
  int32_t n;
  explicit Bytes(const std::string& hex) : n(hex == "-" ? 0 : (int32_t)(hex.size() / 2)) {
    p = (uint8_t*)malloc(n ? n : 1);
    for (int32_t i = 0; i < n; i++) p[i] = (uint8_t)strtol(hex.substr(2 * (size_t)i, 2).c_str(), nullptr, 16);
  }
  ~Bytes() { free(p); }
  Bytes(const Bytes&) = delete;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s jobs answers\n", argv[0]);
    return 2;
  }
  std::ifstream jobs(argv[1]);
  std::ofstream answers(argv[2]);
  GfRpHostWave* w = (GfRpHostWave*)malloc(sizeof(GfRpHostWave));
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what, s1, s2, s3;
    in >> what;
    if (what == "ed") {
      in >> s1 >> s2;
      Bytes a(s1), b(s2);
      answers << gf_rp_edit_distance(*w, a.p, a.n, b.p, b.n) << "\n";
    } else if (what == "filter") {
      GfRpMatch m;
      int32_t thr;
      in >> s1 >> m.read_break >> m.left_distance >> m.right_distance >> m.left_position >> m.right_position >>
          m.left_contig >> m.right_contig >> thr;
      Bytes seq(s1);
      answers << gf_rp_filter_reason(*w, m, seq.p, seq.n, thr) << "\n";
    } else if (what == "adjust") {
      int32_t read_break;
      in >> s1 >> read_break >> s2 >> s3;
      Bytes seq(s1), lref(s2), rref(s3);
      GfRpAdjust a = {0, 0, 0, GF_RP_OUT_OF_DOMAIN};
      if (gf_rp_in_domain(read_break, seq.n)) {
        GfRpSide sides[2 * GF_RP_SHIFTS];
        for (int32_t k = 0; k < 2 * GF_RP_SHIFTS; k++) {
          const bool right = k & 1;
          const Bytes& ref = right ? rref : lref;
          sides[k] = gf_rp_calc_ed_side(*w, right, seq.p, seq.n, read_break + (k >> 1) - 3 + 1, ref.p, ref.n);
        }
        a = gf_rp_choose_shift(sides);
      }
      answers << a.shift << " " << a.left_distance << " " << a.right_distance << " " << a.status << "\n";
    } else {
      fprintf(stderr, "unknown job: %s\n", line.c_str());
      return 2;
    }
  }
  free(w);
  return jobs.bad() || !answers.flush() ? 2 : 0;
}
