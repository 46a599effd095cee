// gf_dd_core.h on the host, under the sanitizers: a stand-alone program that answers jobs, a line each.
//   hash A JUNK HEX            H and K of the record HEX ("-": none) placed A bytes into an aligned buffer, every other
//                              byte of the buffer JUNK: "H K" in hex
//   pair A1 A2 JUNK HEX1 HEX2  K of the pair
//   mask L J                   gf_dd_byte_mask in hex
//   length START END           gf_dd_length
//   home KEYHEX SLOTS          gf_dd_home and gf_dd_next of it
//   level C                    gf_dd_level
//   slots N                    gf_dd_slots_ok
//   table SLOTS NEW COUNTED KEYHEX:INDEX ..   the single-thread walk of insert over an empty table of SLOTS, then with
//                              NEW > 0 of a rehash into NEW slots, then of the histogram: "failed=F K:FIRST:COUNT ..
//                              | h1 .. h31", the entries in slot order
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_dd_core.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

// the record at alignment a of a 16-byte aligned buffer that ends with the chunk of its last byte
struct Placed {
  void* raw = nullptr;
  const uint8_t* first = nullptr;
  Placed(const std::vector<uint8_t>& rec, int a, int junk) {
    const size_t bytes = ((size_t)a + rec.size() + 15) / 16 * 16;
    raw = std::aligned_alloc(16, bytes ? bytes : 16);
    std::memset(raw, junk, bytes ? bytes : 16);
    if (!rec.empty()) std::memcpy((uint8_t*)raw + a, rec.data(), rec.size());
    first = (uint8_t*)raw + a;
  }
  ~Placed() { std::free(raw); }
};

struct Table {
  std::vector<uint64_t> keys;
  std::vector<int64_t> first;
  std::vector<uint32_t> count;
  explicit Table(int64_t slots) : keys(slots, 0), first(slots, GF_DD_NO_INDEX), count(slots, 0) {}
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  std::ofstream out(argv[2]);
  std::string line;
  char buf[64];
  while (std::getline(in, line)) {
    std::istringstream job(line);
    std::string what;
    job >> what;
    if (what == "hash") {
      int a, junk;
      std::string hex;
      job >> a >> junk >> hex;
      const std::vector<uint8_t> rec = unhex(hex);
      Placed p(rec, a, junk);
      const uint64_t h = gf_dd_hash_record(p.first, (int64_t)rec.size());
      std::snprintf(buf, sizeof buf, "%016llx %016llx", (unsigned long long)h,
                    (unsigned long long)gf_dd_key_single((int64_t)rec.size(), h));
      out << buf << "\n";
    } else if (what == "pair") {
      int a1, a2, junk;
      std::string hex1, hex2;
      job >> a1 >> a2 >> junk >> hex1 >> hex2;
      const std::vector<uint8_t> r1 = unhex(hex1), r2 = unhex(hex2);
      Placed p1(r1, a1, junk), p2(r2, a2, junk);
      const uint64_t k = gf_dd_key_pair((int64_t)r1.size(), gf_dd_hash_record(p1.first, (int64_t)r1.size()),
                                        (int64_t)r2.size(), gf_dd_hash_record(p2.first, (int64_t)r2.size()));
      std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)k);
      out << buf << "\n";
    } else if (what == "mask") {
      long long L, j;
      job >> L >> j;
      std::snprintf(buf, sizeof buf, "%016llx", (unsigned long long)gf_dd_byte_mask(L, j));
      out << buf << "\n";
    } else if (what == "length") {
      long long s, e;
      job >> s >> e;
      out << (long long)gf_dd_length(s, e) << "\n";
    } else if (what == "home") {
      std::string key;
      long long slots;
      job >> key >> slots;
      const int64_t h = gf_dd_home(std::stoull(key, nullptr, 16), slots);
      out << (long long)h << " " << (long long)gf_dd_next(h, slots) << "\n";
    } else if (what == "level") {
      unsigned long c;
      job >> c;
      out << gf_dd_level((uint32_t)c) << "\n";
    } else if (what == "slots") {
      long long n;
      job >> n;
      out << (gf_dd_slots_ok(n) ? 1 : 0) << "\n";
    } else if (what == "table") {
      long long slots, grown;
      int counted;
      job >> slots >> grown >> counted;
      Table t(slots);
      long long failed = 0;
      std::string item;
      while (job >> item) {
        const size_t colon = item.find(':');
        const uint64_t key = std::stoull(item.substr(0, colon), nullptr, 16);
        const int64_t index = std::stoll(item.substr(colon + 1));
        bool is_new;
        const int64_t s = gf_dd_place_host(t.keys.data(), slots, key, is_new);
        if (s < 0) {
          ++failed;
          continue;
        }
        if (index < t.first[s]) t.first[s] = index;
        if (counted) ++t.count[s];
      }
      if (grown > 0) {
        Table u(grown);
        for (long long o = 0; o < slots; ++o) {
          if (!t.keys[o]) continue;
          bool is_new;
          const int64_t s = gf_dd_place_host(u.keys.data(), grown, t.keys[o], is_new);
          if (s < 0) return 3;
          if (t.first[o] < u.first[s]) u.first[s] = t.first[o];
          u.count[s] += t.count[o];
        }
        t = u;
        slots = grown;
      }
      long long hist[GF_DD_LEVELS] = {0};
      out << "failed=" << failed;
      for (long long s = 0; s < slots; ++s) {
        if (!t.keys[s]) continue;
        std::snprintf(buf, sizeof buf, " %016llx:%lld:%u", (unsigned long long)t.keys[s], (long long)t.first[s],
                      t.count[s]);
        out << buf;
        if (gf_dd_level(t.count[s]) > 0) ++hist[gf_dd_level(t.count[s])];
      }
      out << " |";
      for (int c = 1; c < GF_DD_LEVELS; ++c) out << " " << hist[c];
      out << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
