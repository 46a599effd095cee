// genefuserust_amd/scan_csrc/gf_oc_core.h on the host, for tests/test_overlap_correct_core.py: a stand-alone program
// that is compiled with -fsanitize=address,undefined.  It reads jobs, one per line, and writes one answer line per job:
//
//   pair G al ar junk <a hex> <qa hex> <b hex> <qb hex> <the settings>
//       ->  "<I*> <fixed a> <fixed b> <left> <words> <a hex> <qa hex> <b hex> <qb hex> <neighbours>"
//       the pair by gf_oc_correct_pair<G>, in place.  Each of the four records lies in a heap block of its own that is
//       exactly its chunks 0 .. (at + L - 1) / 16, its first byte al (a, qa) or ar (b, qb) bytes into chunk 0; the
//       bytes of the block that are not the record's are junk, as a neighbouring record's would be.  <words>: 1 when
//       the popcounts of gf_oc_diff_word over the words of [lo, hi) at I* sum to fixed + left (gf_at_try_insert's
//       count); <neighbours>: 1 when every junk byte is as it was.
//   settings <the settings>  ->  "ok", or what is wrong, in one word
//
// The settings: min_overlap max_diff diff_percent good_phred bad_phred.  "-" stands for an empty hex string.  Chunks
// outside a record's block are never asked for: the loader aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_oc_core.h"

namespace {

std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

std::string hex(const uint8_t* p, size_t n) {
  static const char* digits = "0123456789abcdef";
  if (n == 0) return "-";
  std::string out;
  for (size_t i = 0; i < n; ++i) {
    out.push_back(digits[p[i] >> 4]);
    out.push_back(digits[p[i] & 15]);
  }
  return out;
}

// a record inside a heap block of whole chunks, junk around it
struct Block {
  std::unique_ptr<uint8_t[]> bytes;
  int at = 0, len = 0, chunks = 0;
  uint8_t junk = 0;
  Block(const std::vector<uint8_t>& rec, int at_, uint8_t junk_) : at(at_), len((int)rec.size()), junk(junk_) {
    chunks = len ? (at + len - 1) / 16 + 1 : 0;
    bytes.reset(new uint8_t[(size_t)chunks * 16]);
    for (int k = 0; k < chunks * 16; ++k) bytes[(size_t)k] = junk;
    for (int k = 0; k < len; ++k) bytes[(size_t)(at + k)] = rec[(size_t)k];
  }
  uint8_t* first() const { return bytes.get() + (len ? at : 0); }
  bool neighbours_kept() const {
    for (int k = 0; k < chunks * 16; ++k)
      if ((k < at || k >= at + len) && bytes[(size_t)k] != junk) return false;
    return true;
  }
};

struct Loader {
  const Block& b;
  gf_pp_chunk operator()(int c) const {
    if (c < 0 || c >= b.chunks) {
      std::fprintf(stderr, "chunk %d of a read of %d bytes at %d was asked for\n", c, b.len, b.at);
      std::abort();
    }
    gf_pp_chunk ch;
    std::memcpy(ch.w, b.bytes.get() + 16 * c, 16);
    return ch;
  }
};

gf_oc_settings settings_from(std::istringstream& in) {
  gf_oc_settings s;
  in >> s.min_overlap >> s.max_diff >> s.diff_percent >> s.good_phred >> s.bad_phred;
  return s;
}

// the differences of the pair at I, by gf_oc_diff_word over planes packed from the blocks as they are now
int32_t word_sum(const Block& a, const Block& b, int32_t I) {
  uint32_t A[GF_AT_READ_WORDS], R[GF_AT_READ_WORDS];
  gf_at_pack_read(Loader{a}, a.at, a.len, false, A);
  gf_at_pack_read(Loader{b}, b.at, b.len, true, R);
  const int32_t lo = I > b.len ? I - b.len : 0, hi = I < a.len ? I : a.len;
  int32_t d = 0;
  for (int32_t w = lo >> 5; w <= (hi - 1) >> 5; ++w) d += gf_pp_popcount(gf_oc_diff_word(A, R, a.len, b.len, I, w));
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(gf_oc_settings) == 20, "gf_oc_settings is 20 bytes");
  static_assert(GF_OC_TOTALS == 6, "six totals");
  if (argc != 3) return 2;
  std::ifstream jobs(argv[1]);
  std::ofstream answers(argv[2]);
  std::string line;
  while (std::getline(jobs, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "pair") {
      int G, al, ar, junk;
      std::string ha, hqa, hb, hqb;
      in >> G >> al >> ar >> junk >> ha >> hqa >> hb >> hqb;
      const gf_oc_settings s = settings_from(in);
      if (!in || gf_oc_settings_error(s)) return 3;
      Block a(unhex(ha), al, (uint8_t)junk), qa(unhex(hqa), al, (uint8_t)junk);
      Block b(unhex(hb), ar, (uint8_t)junk), qb(unhex(hqb), ar, (uint8_t)junk);
      if (a.len != qa.len || b.len != qb.len) return 3;
      gf_oc_counts c;
      int32_t insert;
      // (the differences as the search sees them, before a byte changes)
      const gf_at_settings t = gf_oc_search_settings(s);
      int32_t before = -1;
      {
        uint32_t A[GF_AT_READ_WORDS], R[GF_AT_READ_WORDS];
        if (!gf_at_passes(a.len) && !gf_at_passes(b.len)) {
          gf_at_pack_read(Loader{a}, a.at, a.len, false, A);
          gf_at_pack_read(Loader{b}, b.at, b.len, true, R);
          const int32_t I = gf_at_find_insert<16>(A, R, a.len, b.len, t);
          if (I >= 0) before = word_sum(a, b, I);
          if (I >= 0 && (before > t.max_diff || !gf_at_try_insert(A, R, a.len, b.len, I, t))) return 4;
        }
      }
      if (G == 16)
        insert = gf_oc_correct_pair<16>(Loader{a}, al, a.len, Loader{b}, ar, b.len, a.first(), qa.first(), b.first(),
                                        qb.first(), s, c);
      else if (G == 64)
        insert = gf_oc_correct_pair<64>(Loader{a}, al, a.len, Loader{b}, ar, b.len, a.first(), qa.first(), b.first(),
                                        qb.first(), s, c);
      else
        return 3;
      const bool words = insert < 0 ? before == -1 : before == c.fixed[0] + c.fixed[1] + c.left;
      const bool kept = a.neighbours_kept() && qa.neighbours_kept() && b.neighbours_kept() && qb.neighbours_kept();
      answers << insert << " " << c.fixed[0] << " " << c.fixed[1] << " " << c.left << " " << (words ? 1 : 0) << " "
              << hex(a.first(), (size_t)a.len) << " " << hex(qa.first(), (size_t)qa.len) << " "
              << hex(b.first(), (size_t)b.len) << " " << hex(qb.first(), (size_t)qb.len) << " " << (kept ? 1 : 0) << "\n";
    } else if (what == "settings") {
      const gf_oc_settings s = settings_from(in);
      if (!in) return 3;
      const char* wrong = gf_oc_settings_error(s);
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
