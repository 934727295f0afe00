// The two readers of separated-value trace lines (sv_lines.hpp) against each other on the host:
// whatever the compact reader (the device's, here compiled for the host) accepts, the generic
// reader accepts with bit-equal values, the same id span and the same hash; and the compact reader
// reads no byte outside [line start, line start + 256): every line is parsed from a heap block of
// exactly 256 bytes, so AddressSanitizer reports any byte read past it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sv_lines.hpp"

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
    default: std::snprintf(b, sizeof b, "+%.4f", v < 0 ? -v : v); break;   // generic only
  }
  return b;
}

static sv::Format format(int k) {
  sv::Format f = sv::default_format();
  if (k & 1) f.time_format = 1;
  if (k & 2) { f.use_bbox = 1; f.bbox[0] = -45; f.bbox[1] = -90; f.bbox[2] = 45; f.bbox[3] = 90; }
  if (k & 4) f.accuracy_cap = 1000;
  if (k & 8) { f.sep = '|'; f.uuid_col = 1; f.time_col = 0; f.lat_col = 9; f.lon_col = 10; f.acc_col = (k & 16) ? -1 : 5; }
  return f;
}

static std::string make_line(std::mt19937_64& r, const sv::Format& f, bool generic_only) {
  const int ncol = 12;
  std::vector<std::string> col(ncol);
  const int top = generic_only ? 7 : 4;
  col[f.uuid_col] = "veh" + std::to_string(r() % 500);
  if (r() % 50 == 0) col[f.uuid_col] = std::string(1 + r() % 300, 'q');   // may pass 256 bytes
  char t[40];
  if (f.time_format == 1)
    std::snprintf(t, sizeof t, "%04d-%02d-%02d%c%02d:%02d:%02d", (int)(1970 + r() % 131), (int)(1 + r() % 12), (int)(1 + r() % 31),
                  r() % 2 ? ' ' : 'T', (int)(r() % 24), (int)(r() % 60), (int)(r() % 61));
  else
    std::snprintf(t, sizeof t, "%s%llu", r() % 20 == 0 ? "-" : "", (unsigned long long)(r() % 4102444800ull));
  col[f.time_col] = t;
  col[f.lat_col] = num(r, -90, 90, (int)(r() % top));
  col[f.lon_col] = num(r, -180, 180, (int)(r() % top));
  if (f.acc_col >= 0) col[f.acc_col] = num(r, 0, 3000, (int)(r() % top));
  int last = 0;
  for (int c = 0; c < ncol; ++c)
    if (!col[c].empty()) last = c;
  if (r() % 4 == 0 && last + 2 < ncol) { col[last + 2] = "more"; last += 2; }
  std::string s;
  for (int c = 0; c <= last; ++c) { if (c) s += (char)f.sep; s += col[c]; }
  if (generic_only && r() % 3 == 0) s = " " + s + "\t";
  if (r() % 5 == 0) s += '\r';
  return s;
}

static void mutate(std::mt19937_64& r, std::string& s, const sv::Format& f) {
  static const char pool[] = "0123456789.-+eE \t\r\nxX_:,|";
  const int n = 1 + (int)(r() % 3);
  for (int k = 0; k < n; ++k) {
    const char c = r() % 4 == 0 ? (char)f.sep : pool[r() % (sizeof pool - 1)];
    const size_t at = s.empty() ? 0 : r() % s.size();
    switch (r() % 3) {
      case 0: if (!s.empty()) s[at] = c; break;
      case 1: s.insert(s.begin() + (long)at, c); break;
      default: if (!s.empty()) s.erase(at, 1); break;
    }
  }
}

int main() {
  CHECK(sv::id_hash((const uint8_t*)"", 0) == 0xcbf29ce484222325ull);
  CHECK(sv::id_hash((const uint8_t*)"a", 1) == 0xaf63dc4c8601ec8cull);
  CHECK(sv::id_hash((const uint8_t*)"foobar", 6) == 0x85944171f73967e8ull);
  CHECK(sv::days_from_civil(1970, 1, 1) == 0 && sv::days_from_civil(2000, 3, 1) == 11017 && sv::days_from_civil(1969, 12, 31) == -1);
  double tv = 0;
  CHECK(sv::civil_time((const uint8_t*)"2017-01-01 06:05:40", tv) && tv == 1483250740.0);
  CHECK(!sv::civil_time((const uint8_t*)"2017-13-01 06:05:40", tv) && !sv::civil_time((const uint8_t*)"2017-01-01 24:05:40", tv));

  std::mt19937_64 r(20240607);
  const int kLines = 24000;
  long accepted = 0, points = 0, plain = 0, plain_points = 0, hosts = 0, generic_bad = 0, outside = 0, blank = 0;
  for (int n = 0; n < kLines; ++n) {
    const sv::Format f = format((int)(r() % 32));
    const bool mutated = n % 2 == 1;
    const bool generic_only = !mutated && n % 10 == 0;
    std::string s = n % 400 == 2 ? std::string(r() % 2 ? "" : "\r") : make_line(r, f, generic_only);
    if (mutated) mutate(r, s, f);
    // the text as the device sees it: the line, its '\n', then whatever follows, in a block of
    // exactly sv::kMaxLine bytes
    std::string text = s + "\n";
    while (text.size() < sv::kMaxLine) text += make_line(r, f, false) + "\n";
    uint8_t* blk = (uint8_t*)std::malloc(sv::kMaxLine);
    std::memcpy(blk, text.data(), sv::kMaxLine);
    sv::Line c{};
    const uint32_t st = sv::compact_line(blk, f, c);
    std::free(blk);
    // the generic reader over the first line of the untruncated text
    const uint8_t* b = (const uint8_t*)text.data();
    const uint8_t* e = (const uint8_t*)std::memchr(b, '\n', text.size());
    sv::Line g{};
    const char* why = nullptr;
    const uint32_t gs = sv::generic_line(b, e, f, g, &why);
    generic_bad += gs == sv::kBad;
    CHECK(gs != sv::kBad || why != nullptr);
    const bool is_plain = !mutated && !generic_only && s.size() + 1 <= sv::kMaxLine;
    plain += is_plain;
    if (st == sv::kHost) {
      ++hosts;
      CHECK(!is_plain);   // a line in the compact layout is read by the compact reader
      continue;
    }
    ++accepted;
    CHECK(st == gs);
    if ((size_t)(e - b) + 1 > sv::kMaxLine) CHECK(false);   // an accepted line fits 256 bytes
    outside += st == sv::kOutside;
    blank += st == sv::kBlank;
    if (st != sv::kPoint || gs != sv::kPoint) continue;
    ++points;
    plain_points += is_plain;
    CHECK(std::memcmp(&c.lat, &g.lat, 4) == 0 && std::memcmp(&c.lon, &g.lon, 4) == 0 && std::memcmp(&c.acc, &g.acc, 4) == 0);
    CHECK(std::memcmp(&c.time, &g.time, 8) == 0);
    CHECK(c.id_off == g.id_off && c.id_len == g.id_len && c.hash == g.hash);
    CHECK(c.hash == sv::id_hash(b + g.id_off, g.id_len));
  }
  std::printf("lines %d accepted %ld points %ld outside %ld blank %ld host %ld generic-bad %ld plain %ld\n", kLines, accepted, points,
              outside, blank, hosts, generic_bad, plain);
  CHECK(plain > 8000 && points > 6000 && outside > 500 && blank > 20 && hosts > 3000 && generic_bad > 1000);
  CHECK(plain_points + outside >= plain * 9 / 10);
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("sv lines ok\n");
  return 0;
}
