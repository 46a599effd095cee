// genefuserust_amd/csrc/gf_host_batch.h on its own: jobs in, answers out, one line each (tests/test_host_batch.py).
//   check <have_reads 0|1> <n> null | <n+1 offsets>   ->  rc [b0 b1 maxlen]        (both halves of the pack check)
//   staged <reads> <bytes> <hits_cap> <compact_ws>    ->  the seven region offsets and the total
//   packed <b0> <b1>                                  ->  c0 nc iv_at bytes
//   zc <n> <bytes> <staged 0|1>                       ->  offsets matches counts bases bytes
// The offsets live in a vector of exactly n + 1 entries: a read past them is AddressSanitizer's to find.
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/csrc/gf_host_batch.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream jobs(argv[1]);
  std::ofstream out(argv[2]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "check") {
      int have = 0;
      long long n = 0;
      in >> have >> n;
      std::string tok;
      std::vector<int64_t> off;
      bool null = false;
      while (in >> tok) {
        if (tok == "null") null = true; else off.push_back(std::stoll(tok));
      }
      if (!null && n > 0 && (long long)off.size() != n + 1) return 3;
      gf_pack_span p;
      int rc = gf_pack_measure(null || off.empty() ? nullptr : off.data(), n, &p);
      if (rc == GF_OK) rc = gf_pack_reads_present(p, have != 0);
      out << rc;
      if (rc == GF_OK) out << " " << p.b0 << " " << p.b1 << " " << p.maxlen;
      out << "\n";
    } else if (what == "staged") {
      long long reads, bytes, cap, cws;
      in >> reads >> bytes >> cap >> cws;
      const gf_staged_layout a = gf_staged_layout_for(reads, bytes, cap, cws);
      out << a.bases << " " << a.offsets << " " << a.counts << " " << a.matches << " " << a.hits << " " << a.total << " "
          << a.compact_ws << " " << a.bytes << "\n";
    } else if (what == "packed") {
      long long b0, b1;
      in >> b0 >> b1;
      const gf_packed_stage k = gf_packed_stage_for(b0, b1);
      out << k.c0 << " " << k.nc << " " << k.iv_at << " " << k.bytes << "\n";
    } else if (what == "zc") {
      long long n, bytes;
      int staged;
      in >> n >> bytes >> staged;
      const gf_zc_layout z = gf_zc_layout_for(n, bytes, staged != 0);
      out << z.offsets << " " << z.matches << " " << z.counts << " " << z.bases << " " << z.bytes << "\n";
    } else {
      return 5;
    }
  }
  return 0;
}
