// gf_rw_core.h on the host, under the sanitizers: a stand-alone program that answers jobs, a line each.
//   format SOURCE LENGTH GATHER SIDES N JUNK  then per side:
//          A_TEXT HEXTEXT A_REC HEXBASES HEXQUALS OFFS A_PRE HEXPRE PREOFFS A_OUT
//                              one gf_rw_format_host call.  Every input is placed A_* bytes into an aligned heap block
//                              that ends with its last byte, every other byte JUNK ("-": no bytes; OFFS / PREOFFS:
//                              n + 1 offsets with commas, from the first byte; HEXPRE "-" and PREOFFS "-" without a
//                              tag); the newline index is that of the text.  The output block has the capacity and
//                              ends with it.  Answers per side "HEXOUT OFFS", then "TOTALS CLEAN": CLEAN is 1 when
//                              every output byte behind the text is still JUNK.
//   span TEXTBYTES I NL ..     gf_rw_name_span over the newline positions NL ..: "start end"
//   record NS NE TOK TAGLEN FROM LEN   gf_rw_make_record: "start[0] .. start[7]", and the segment of its positions
//                              0, every start[s] - 1 and start[s], and size - 1
//   size NAMELEN TAGLEN LEN    gf_rw_size
//   cap TEXTBYTES N            gf_rw_capacity
//   token A HEX                gf_rw_token_end of the line HEX placed A bytes into a block that ends with it
//   pieces A SIZE              per piece "p:full:k_lo:k_hi"
//   settings SOURCE LENGTH GATHER   gf_rw_settings_ok
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../genefuserust_amd/scan_csrc/gf_rw_core.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char* digits = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(digits[p[i] >> 4]);
    s.push_back(digits[p[i] & 15]);
  }
  return s.empty() ? "-" : s;
}

static std::vector<int64_t> numbers(const std::string& s) {
  std::vector<int64_t> out;
  if (s == "-") return out;
  std::istringstream in(s);
  std::string item;
  while (std::getline(in, item, ',')) out.push_back(std::stoll(item));
  return out;
}

// The bytes at alignment a (malloc's blocks are 16-byte aligned) of a heap block that ends with their last byte, every
// other byte of it junk: the host walks load no byte outside the bounds they are given, so a load in front of the block
// or behind the last byte fails under ASan, and so does a store.
struct Placed {
  uint8_t* block = nullptr;
  uint8_t* first = nullptr;
  Placed(const std::vector<uint8_t>& bytes, int a, int junk) {
    const size_t n = (size_t)a + bytes.size();
    block = (uint8_t*)std::malloc(n ? n : 1);
    if (((uintptr_t)block & 15) != 0) std::abort();
    std::memset(block, junk, n ? n : 1);
    if (!bytes.empty()) std::memcpy(block + a, bytes.data(), bytes.size());
    first = block + a;
  }
  Placed(const Placed&) = delete;
  ~Placed() { std::free(block); }
};

struct Side {
  Placed *text = nullptr, *bases = nullptr, *quals = nullptr, *pre = nullptr, *out = nullptr;
  std::vector<int64_t> nl, off, pre_off, out_off;
  int64_t text_bytes = 0, cap = 0;
  ~Side() {
    delete text;
    delete bases;
    delete quals;
    delete pre;
    delete out;
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  std::ofstream out(argv[2]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream job(line);
    std::string what;
    job >> what;
    if (what == "format") {
      int source, length, gather, sides, junk;
      long long n;
      job >> source >> length >> gather >> sides >> n >> junk;
      Side side[2];
      gf_rw_in input[2] = {};
      uint8_t* out_text[2] = {nullptr, nullptr};
      int64_t out_cap[2] = {0, 0};
      int64_t* out_off[2] = {nullptr, nullptr};
      for (int s = 0; s < sides; ++s) {
        int a_text, a_rec, a_pre, a_out;
        std::string h_text, h_bases, h_quals, offs, h_pre, pre_offs;
        job >> a_text >> h_text >> a_rec >> h_bases >> h_quals >> offs >> a_pre >> h_pre >> pre_offs >> a_out;
        const std::vector<uint8_t> text = unhex(h_text);
        Side& x = side[s];
        x.text = new Placed(text, a_text, junk);
        x.bases = new Placed(unhex(h_bases), a_rec, junk);
        x.quals = new Placed(unhex(h_quals), (a_rec + 5) & 15, junk);
        x.pre = new Placed(unhex(h_pre), a_pre, junk);
        x.off = numbers(offs);
        x.pre_off = numbers(pre_offs);
        for (size_t k = 0; k < text.size(); ++k)
          if (text[k] == '\n') x.nl.push_back((int64_t)k);
        x.text_bytes = (int64_t)text.size();
        x.cap = gf_rw_capacity(x.text_bytes, n);
        x.out = new Placed(std::vector<uint8_t>((size_t)x.cap, (uint8_t)junk), a_out, junk);
        x.out_off.assign((size_t)n + 1, -1);
        input[s] = gf_rw_in{x.text->first, x.text_bytes, x.nl.data(), (int64_t)x.nl.size(), x.bases->first,
                            x.quals->first, x.off.data(), x.pre_off.empty() ? nullptr : x.pre->first,
                            x.pre_off.empty() ? nullptr : x.pre_off.data()};
        out_text[s] = x.out->first;
        out_cap[s] = x.cap;
        out_off[s] = x.out_off.data();
      }
      int64_t totals[GF_RW_TOTALS] = {0, 0, 0, 0, 0};
      gf_rw_format_host(source, length, gather, input, sides, n, out_text, out_cap, out_off, totals);
      bool clean = true;
      for (int s = 0; s < sides; ++s) {
        const Side& x = side[s];
        const int64_t total = x.out_off[(size_t)n];
        out << hex(x.out->first, (size_t)total) << " ";
        for (size_t k = 0; k < x.out_off.size(); ++k) out << (k ? "," : "") << (long long)x.out_off[k];
        out << " ";
        for (int64_t k = total; k < x.cap; ++k) clean = clean && x.out->first[k] == (uint8_t)junk;
        for (const uint8_t* p = x.out->block; p < x.out->first; ++p) clean = clean && *p == (uint8_t)junk;
      }
      for (int k = 0; k < GF_RW_TOTALS; ++k) out << (k ? "," : "") << (long long)totals[k];
      out << " " << (clean ? 1 : 0) << "\n";
    } else if (what == "span") {
      long long text_bytes, i, p;
      job >> text_bytes >> i;
      std::vector<int64_t> nl;
      while (job >> p) nl.push_back(p);
      int64_t s = -1, e = -1;
      gf_rw_name_span(nl.data(), (int64_t)nl.size(), text_bytes, i, s, e);
      out << (long long)s << " " << (long long)e << "\n";
    } else if (what == "record") {
      long long ns, ne, tok, tag_len, from, len;
      job >> ns >> ne >> tok >> tag_len >> from >> len;
      gf_rw_tag tag{(int32_t)tag_len, 0, 0, 0, 0, 0};
      const gf_rw_record r = gf_rw_make_record(ns, ne, tok, tag, from, len);
      for (int s = 0; s <= GF_RW_SEGS; ++s) out << (s ? "," : "") << (long long)r.start[s];
      out << " " << gf_rw_segment_of(r, 0);
      for (int s = 1; s <= GF_RW_SEGS; ++s) {
        if (r.start[s] > 0) out << "," << gf_rw_segment_of(r, r.start[s] - 1);
        if (s < GF_RW_SEGS) out << "," << gf_rw_segment_of(r, r.start[s]);
      }
      out << "\n";
    } else if (what == "size") {
      long long name_len, tag_len, len;
      job >> name_len >> tag_len >> len;
      out << (long long)gf_rw_size(name_len, tag_len, len) << "\n";
    } else if (what == "cap") {
      long long text_bytes, n;
      job >> text_bytes >> n;
      out << (long long)gf_rw_capacity(text_bytes, n) << "\n";
    } else if (what == "token") {
      int a;
      std::string h;
      job >> a >> h;
      const std::vector<uint8_t> text = unhex(h);
      Placed p(text, a, ' ');
      out << (long long)gf_rw_token_end(p.first, 0, (int64_t)text.size()) << "\n";
    } else if (what == "pieces") {
      int a;
      long long size;
      job >> a >> size;
      const int64_t pieces = gf_rw_pieces(a, size);
      out << (long long)pieces;
      for (int64_t q = 0; q < pieces; ++q) {
        const int64_t p = gf_rw_piece_pos(a, q);
        int k_lo = 0, k_hi = 16;
        const bool full = gf_rw_piece_full(p, size);
        if (!full) gf_rw_piece_part(p, size, k_lo, k_hi);
        out << " " << (long long)p << ":" << (full ? 1 : 0) << ":" << k_lo << ":" << k_hi;
      }
      out << "\n";
    } else if (what == "settings") {
      int source, length, gather;
      job >> source >> length >> gather;
      out << (gf_rw_settings_ok(source, length, gather) ? 1 : 0) << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
