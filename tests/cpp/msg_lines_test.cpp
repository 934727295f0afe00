// The two readers of JSON stream messages (msg_lines.hpp) against each other on the host: wherever
// the compact reader (the device's, here compiled for the host) does not answer "host", the generic
// reader gives the same status, bit-equal values, the same id span and the same hash; and the
// compact reader reads no byte outside [line start, line start + 256): every line is parsed from a
// heap block of exactly 256 bytes, so AddressSanitizer reports any byte read past it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "msg_lines.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static std::string num(std::mt19937_64& r, double lo, double hi, int kind) {
  char b[64];
  const double v = lo + (hi - lo) * (double)(r() % 1000000) / 1e6;
  switch (kind) {
    case 0: std::snprintf(b, sizeof b, "%.6f", v); break;
    case 1: std::snprintf(b, sizeof b, "%d", (int)v); break;
    case 2: std::snprintf(b, sizeof b, "%.9f", v); break;
    case 3: std::snprintf(b, sizeof b, "%.1f", v); break;
    case 4: std::snprintf(b, sizeof b, "%.17g", v); break;   // generic only
    case 5: std::snprintf(b, sizeof b, "%.5e", v); break;    // generic only
    default: std::snprintf(b, sizeof b, "\"%.4f\"", v); break;   // generic only: a number in a string
  }
  return b;
}

static msg::Format format(int k) {
  msg::Format f = msg::default_format();
  f.kind = 1;
  if (k & 1) f.line.time_format = 1;
  if (k & 2) { f.line.use_bbox = 1; f.line.bbox[0] = -45; f.line.bbox[1] = -90; f.line.bbox[2] = 45; f.line.bbox[3] = 90; }
  if (k & 4) f.line.accuracy_cap = 1000;
  if (k & 8) {
    std::strcpy(f.key[msg::kId], "i"); std::strcpy(f.key[msg::kLat], "la"); std::strcpy(f.key[msg::kLon], "lo");
    std::strcpy(f.key[msg::kTime], "t"); std::strcpy(f.key[msg::kAcc], (k & 16) ? "" : "a");
  }
  return f;
}

static std::string make_line(std::mt19937_64& r, const msg::Format& f, bool generic_only) {
  const int top = generic_only ? 7 : 4;
  std::vector<std::string> mem;
  std::string id = "veh" + std::to_string(r() % 500);
  if (r() % 50 == 0) id = std::string(1 + r() % 300, 'q');   // may pass 256 bytes
  const std::string q = "\"";
  const std::string sep = generic_only && r() % 2 ? " : " : ":";
  mem.push_back(q + f.key[msg::kId] + q + sep + q + id + q);
  char t[48];
  if (f.line.time_format == 1)
    std::snprintf(t, sizeof t, "\"%04d-%02d-%02d%c%02d:%02d:%02d\"", (int)(1970 + r() % 131), (int)(1 + r() % 12), (int)(1 + r() % 31),
                  r() % 2 ? ' ' : 'T', (int)(r() % 24), (int)(r() % 60), (int)(r() % 61));
  else
    std::snprintf(t, sizeof t, "%s%llu", r() % 20 == 0 ? "-" : "", (unsigned long long)(r() % 4102444800ull));
  mem.push_back(q + f.key[msg::kTime] + q + sep + t);
  mem.push_back(q + f.key[msg::kLat] + q + sep + num(r, -90, 90, (int)(r() % top)));
  mem.push_back(q + f.key[msg::kLon] + q + sep + num(r, -180, 180, (int)(r() % top)));
  if (f.key[msg::kAcc][0]) mem.push_back(q + f.key[msg::kAcc] + q + sep + num(r, 0, 3000, (int)(r() % top)));
  // extra members: scalars for every line, a nested one or a repeated key for generic-only lines
  static const char* extra[] = {"\"speed\":12.5", "\"ok\":true", "\"note\":\"a b, {c}\"", "\"gone\":null", "\"flag\":false",
                                "\"latitud\":1", "\"idx\":\"zz\""};
  for (int k = (int)(r() % 3); k > 0; --k) mem.push_back(extra[r() % 7]);
  if (generic_only && r() % 3 == 0) mem.push_back("\"nest\":{\"id\":[1,2,{\"x\":\"}\"}]}");
  for (size_t i = mem.size(); i > 1; --i) std::swap(mem[i - 1], mem[r() % i]);   // keys in every order
  // repeated keys, kept in front: the last of a repeated key wins
  if (generic_only && r() % 4 == 0) mem.insert(mem.begin(), q + f.key[msg::kLat] + q + ":\"first of two\"");
  if (generic_only && r() % 4 == 0) mem.insert(mem.begin(), q + f.key[msg::kLon] + q + ":null");
  std::string s = "{";
  for (size_t i = 0; i < mem.size(); ++i) { if (i) s += generic_only && r() % 2 ? " , " : ","; s += mem[i]; }
  s += "}";
  if (generic_only && r() % 3 == 0) s = " " + s + "\t";
  if (r() % 5 == 0) s += '\r';
  return s;
}

static void mutate(std::mt19937_64& r, std::string& s) {
  static const char pool[] = "0123456789.-+eE \t\r\nxX_:,|\"\"\\{}[]tfn";
  const int n = 1 + (int)(r() % 3);
  for (int k = 0; k < n; ++k) {
    const char c = r() % 40 == 0 ? (char)(r() % 256) : pool[r() % (sizeof pool - 1)];
    const size_t at = s.empty() ? 0 : r() % s.size();
    switch (r() % 3) {
      case 0: if (!s.empty()) s[at] = c; break;
      case 1: s.insert(s.begin() + (long)at, c); break;
      default: if (!s.empty()) s.erase(at, 1); break;
    }
  }
}

int main() {
  {   // formats
    msg::Format f = msg::default_format();
    f.kind = 1;
    CHECK(!*msg::format_error(f));
    std::strcpy(f.key[msg::kLat], "id");
    CHECK(*msg::format_error(f));
    std::strcpy(f.key[msg::kLat], "a\"b");
    CHECK(*msg::format_error(f));
    std::strcpy(f.key[msg::kLat], "");
    CHECK(*msg::format_error(f));
    std::memset(f.key[msg::kLat], 'k', msg::kKeyBytes);
    CHECK(*msg::format_error(f));
    f = msg::default_format();
    f.kind = 1;
    f.key[msg::kAcc][0] = 0;
    CHECK(!*msg::format_error(f));
    f.kind = 2;
    CHECK(*msg::format_error(f));
  }
  {   // named lines: -0 as a time, and the number spellings json.hpp takes but JSON does not
    msg::Format f = msg::default_format();
    f.kind = 1;
    const msg::Keys keys = msg::make_keys(f);
    auto both = [&](const std::string& line, sv::Line& c, sv::Line& g, uint32_t& cs, uint32_t& gs) {
      std::string text = line + "\n";
      text.resize(sv::kMaxLine, 'x');
      uint8_t* blk = (uint8_t*)std::malloc(sv::kMaxLine);
      std::memcpy(blk, text.data(), sv::kMaxLine);
      cs = msg::compact_json(blk, f.line, keys, c);
      std::free(blk);
      const char* why = nullptr;
      gs = msg::generic_message((const uint8_t*)line.data(), (const uint8_t*)line.data() + line.size(), f, g, &why);
    };
    const std::string head = "{\"id\":\"v\",\"latitude\":1.5,\"longitude\":2.5,\"accuracy\":3,\"timestamp\":";
    const double zero = 0.0;
    for (const char* t : {"-0", "0", "-0.0", "-0.4", "\"-0\"", "-0e0"}) {
      sv::Line c{}, g{};
      uint32_t cs = 0, gs = 0;
      both(head + t + "}", c, g, cs, gs);
      CHECK(gs == sv::kPoint && std::memcmp(&g.time, &zero, 8) == 0);   // +0.0, never -0.0
      CHECK(cs == sv::kHost || (cs == sv::kPoint && std::memcmp(&c.time, &g.time, 8) == 0));
      if (std::string(t) == "-0" || std::string(t) == "0") CHECK(cs == sv::kPoint);
    }
    for (const char* t : {"01", "007", "-01", "1.", "1.e5", "00"}) {
      for (int where = 0; where < 3; ++where) {
        sv::Line c{}, g{};
        uint32_t cs = 0, gs = 0;
        const std::string line = where == 0 ? head + t + "}"
                               : where == 1 ? std::string("{\"latitude\":") + t + ",\"id\":\"v\",\"longitude\":2.5,\"accuracy\":3,\"timestamp\":5}"
                                            : std::string("{\"extra\":[{\"n\":") + t + "}]," + head.substr(1) + "5}";
        both(line, c, g, cs, gs);
        CHECK(gs == sv::kBad);
        CHECK(cs == sv::kHost);
      }
    }
    sv::Line c{}, g{};
    uint32_t cs = 0, gs = 0;
    both(head + "10,\"note\":\"007 and 1. in a string\",\"n\":0,\"m\":-0.5e+07}", c, g, cs, gs);
    CHECK(gs == sv::kPoint && g.time == 10.0);
  }
  std::mt19937_64 r(20260112);
  const int kLines = 24000;
  long accepted = 0, points = 0, plain = 0, plain_taken = 0, hosts = 0, generic_bad = 0, generic_points = 0, outside = 0, blank = 0;
  for (int n = 0; n < kLines; ++n) {
    const msg::Format f = format((int)(r() % 32));
    const msg::Keys keys = msg::make_keys(f);
    const bool mutated = n % 2 == 1;
    const bool generic_only = !mutated && n % 10 == 0;
    std::string s = n % 400 == 2 ? std::string(r() % 2 ? "" : "\r") : make_line(r, f, generic_only);
    if (mutated) mutate(r, s);
    // the text as the device sees it: the line, its '\n', then whatever follows, in a block of
    // exactly sv::kMaxLine bytes
    std::string text = s + "\n";
    while (text.size() < sv::kMaxLine) text += make_line(r, f, false) + "\n";
    uint8_t* blk = (uint8_t*)std::malloc(sv::kMaxLine);
    std::memcpy(blk, text.data(), sv::kMaxLine);
    sv::Line c{};
    const uint32_t st = msg::compact_json(blk, f.line, keys, c);
    std::free(blk);
    // the generic reader over the first line of the untruncated text
    const uint8_t* b = (const uint8_t*)text.data();
    const uint8_t* e = (const uint8_t*)std::memchr(b, '\n', text.size());
    sv::Line g{};
    const char* why = nullptr;
    const uint32_t gs = msg::generic_message(b, e, f, g, &why);
    generic_bad += gs == sv::kBad;
    generic_points += gs == sv::kPoint;
    CHECK(gs != sv::kBad || why != nullptr);
    CHECK(gs != sv::kHost);
    if (generic_only && s.size() < 200) CHECK(gs == sv::kPoint || gs == sv::kOutside);
    const bool is_plain = !mutated && !generic_only && s.size() + 1 <= sv::kMaxLine;
    plain += is_plain;
    if (st == sv::kHost) {
      ++hosts;
      CHECK(!is_plain);   // a line in the compact layout is read by the compact reader
      continue;
    }
    plain_taken += is_plain;
    ++accepted;
    CHECK(st == gs);
    if ((size_t)(e - b) + 1 > sv::kMaxLine) CHECK(false);   // an accepted line fits 256 bytes
    outside += st == sv::kOutside;
    blank += st == sv::kBlank;
    if (st != sv::kPoint || gs != sv::kPoint) continue;
    ++points;
    CHECK(std::memcmp(&c.lat, &g.lat, 4) == 0 && std::memcmp(&c.lon, &g.lon, 4) == 0 && std::memcmp(&c.acc, &g.acc, 4) == 0);
    CHECK(std::memcmp(&c.time, &g.time, 8) == 0);
    CHECK(c.id_off == g.id_off && c.id_len == g.id_len && c.hash == g.hash);
    CHECK(c.hash == sv::id_hash(b + g.id_off, g.id_len));
  }
  std::printf("lines %d accepted %ld points %ld outside %ld blank %ld host %ld generic-bad %ld generic-points %ld\n", kLines, accepted,
              points, outside, blank, hosts, generic_bad, generic_points);
#if defined(__SANITIZE_ADDRESS__)
  std::printf("sanitizers: address, undefined\n");
#else
  std::printf("sanitizers: none (the 256-byte bound was not checked in this build)\n");
#endif
  std::printf("compact share of unmutated lines: %ld / %ld\n", plain_taken, plain);
  CHECK(plain > 8000 && points > 6000 && outside > 500 && blank > 20 && hosts > 3000 && generic_bad > 1000);
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("msg lines ok\n");
  return 0;
}
