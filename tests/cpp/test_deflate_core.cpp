// The host build of genefuserust_amd/scan_csrc/gf_df_core.h, the encoder the kernels of libgfdeflate.so run, as a
// stand-alone program for tests/test_deflate_core.py (g++ -fsanitize=address,undefined):
//
//     test_deflate_core <jobs> <answers>
//
// One job a line, one line of answers each:
//     member <text file> <member file>    the member of the file's text (1 .. 65280 bytes): "<size> <kind>"
//     plan <file of 316 counts>           gf_df_order on both alphabets (286 literal/length counts, then 30 distance
//                                         counts), then gf_df_plan, in a heap block of exactly one GfDfPlan:
//                                         "<lens[316]> <cl_lens[19]> <cl_freq[19]> <hlit> <hdist> <bits>"
//     len <length - 3>                    "<index> <extra bits> <value>" of the length symbol
//     dist <distance - 1>                 "<symbol> <extra bits> <value>" of the distance symbol
//     minlen <distance>                   from how many bytes on a match at this distance is taken
// The text is encoded from a heap copy of exactly its bytes into a heap block of exactly text + 31 bytes, so that the
// sanitizer sees a byte read or written next to either.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_df_core.h"

namespace {

std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
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
    std::string what;
    in >> what;
    if (what == "member") {
      std::string from, to;
      in >> from >> to;
      const std::vector<uint8_t> file = slurp(from);
      const uint32_t n = (uint32_t)file.size();
      if (n == 0 || n > GF_DF_TEXT) {
        fprintf(stderr, "a member holds 1 .. %u bytes of text, not %u\n", GF_DF_TEXT, n);
        return 2;
      }
      uint8_t* text = new uint8_t[n];
      memcpy(text, file.data(), n);
      uint8_t* out = new uint8_t[n + GF_DF_STORED_OVER];
      uint16_t* units = new uint16_t[n];
      uint32_t* table = new uint32_t[GF_DF_HASH_SIZE];
      int kind = 0;
      const uint32_t size = gf_df_member(text, n, out, units, table, kind);
      std::ofstream(to, std::ios::binary).write((const char*)out, size);
      answers << size << " " << kind << "\n";
      delete[] text;
      delete[] out;
      delete[] units;
      delete[] table;
    } else if (what == "plan") {
      std::string from;
      in >> from;
      std::ifstream counts(from);
      GfDfPlan* P = new GfDfPlan;
      uint32_t got = 0;
      while (got < GF_DF_NSYM && (counts >> P->freq[got])) got++;
      if (got != GF_DF_NSYM) {
        fprintf(stderr, "%s: %u counts, not %u\n", from.c_str(), got, GF_DF_NSYM);
        return 2;
      }
      gf_df_order(P->freq, GF_DF_NLIT, P->order);
      gf_df_order(P->freq + GF_DF_NLIT, GF_DF_NDIST, P->order + GF_DF_NLIT);
      gf_df_plan(*P);
      for (uint32_t s = 0; s < GF_DF_NSYM; s++) answers << (uint32_t)P->lens[s] << " ";
      for (uint32_t k = 0; k < GF_DF_NCL; k++) answers << (uint32_t)P->cl_lens[k] << " ";
      for (uint32_t k = 0; k < GF_DF_NCL; k++) answers << P->cl_freq[k] << " ";
      answers << P->hlit << " " << P->hdist << " " << P->bits << "\n";
      delete P;
    } else if (what == "len" || what == "dist") {
      uint32_t x, a, b, c;
      in >> x;
      if (what == "len") gf_df_len_symbol(x, a, b, c);
      else gf_df_dist_symbol(x, a, b, c);
      answers << a << " " << b << " " << c << "\n";
    } else if (what == "minlen") {
      uint32_t d;
      in >> d;
      answers << gf_df_min_len(d) << "\n";
    } else {
      fprintf(stderr, "unknown job: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
