// gf_um_core.h on the host, under the sanitizers: a stand-alone program that answers jobs, a line each.
//   cut SOURCE LENGTH SKIP SIDES A1 A2 JUNK HEX1 HEX2
//                              one record of the inline sources: its sides ("-": no bases; HEX2 is ignored with SIDES 1)
//                              placed A1 / A2 bytes into aligned buffers that end with the record's last byte, every
//                              other byte JUNK: "stays cut1 cut2 code has_n", the code in hex
//   name A JUNK HEX            U of the name line HEX placed A bytes into a buffer that ends with the line's last byte:
//                              "code has_n"
//   mix KHEX UHEX              gf_um_mix_key in hex
//   settings SOURCE LENGTH SKIP   gf_um_settings_ok
//   line TEXTBYTES I NL ..     gf_um_name_line over the newline positions NL ..: "exists start end"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_um_core.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

// The bytes at alignment a (malloc's blocks are 16-byte aligned) of a heap block that ends with their last byte, every
// other byte of it junk: the host walks load no byte outside the bounds they are given, so a load in front of the block
// or behind the last byte fails under ASan.
struct Placed {
  uint8_t* block = nullptr;
  const uint8_t* first = nullptr;
  Placed(const std::vector<uint8_t>& bytes, int a, int junk) {
    const size_t n = (size_t)a + bytes.size();
    block = (uint8_t*)std::malloc(n ? n : 1);
    if (((uintptr_t)block & 15) != 0) std::abort();
    std::memset(block, junk, n ? n : 1);
    if (!bytes.empty()) std::memcpy(block + a, bytes.data(), bytes.size());
    first = block + a;
  }
  ~Placed() { std::free(block); }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  std::ofstream out(argv[2]);
  std::string line;
  char buf[96];
  while (std::getline(in, line)) {
    std::istringstream job(line);
    std::string what;
    job >> what;
    if (what == "cut") {
      int source, length, skip, sides, a1, a2, junk;
      std::string hex1, hex2;
      job >> source >> length >> skip >> sides >> a1 >> a2 >> junk >> hex1 >> hex2;
      const std::vector<uint8_t> r1 = unhex(hex1), r2 = unhex(hex2);
      Placed p1(r1, a1, junk), p2(r2, a2, junk);
      const uint8_t* first[2] = {p1.first, p2.first};
      const int64_t L[2] = {(int64_t)r1.size(), (int64_t)r2.size()};
      int64_t cut[2] = {0, 0};
      uint64_t code = 0;
      bool has_n = false;
      const bool stays = gf_um_cut_host(source, length, skip, sides, first, L, cut, code, has_n);
      std::snprintf(buf, sizeof buf, "%d %lld %lld %016llx %d", stays ? 1 : 0, (long long)cut[0], (long long)cut[1],
                    (unsigned long long)code, has_n ? 1 : 0);
      out << buf << "\n";
    } else if (what == "name") {
      int a, junk;
      std::string hex;
      job >> a >> junk >> hex;
      const std::vector<uint8_t> text = unhex(hex);
      Placed p(text, a, junk);
      bool has_n = false;
      const uint64_t code = gf_um_name_code_host(p.first, 0, (int64_t)text.size(), has_n);
      std::snprintf(buf, sizeof buf, "%016llx %d", (unsigned long long)code, has_n ? 1 : 0);
      out << buf << "\n";
    } else if (what == "mix") {
      std::string k, u;
      job >> k >> u;
      std::snprintf(buf, sizeof buf, "%016llx",
                    (unsigned long long)gf_um_mix_key(std::stoull(k, nullptr, 16), std::stoull(u, nullptr, 16)));
      out << buf << "\n";
    } else if (what == "settings") {
      int source, length, skip;
      job >> source >> length >> skip;
      out << (gf_um_settings_ok(source, length, skip) ? 1 : 0) << "\n";
    } else if (what == "line") {
      long long text_bytes, i, p;
      job >> text_bytes >> i;
      std::vector<int64_t> nl;
      while (job >> p) nl.push_back(p);
      int64_t s = -1, e = -1;
      const bool exists = gf_um_name_line(nl.data(), (int64_t)nl.size(), text_bytes, i, s, e);
      out << (exists ? 1 : 0) << " " << (long long)s << " " << (long long)e << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
