// Date patterns (time_pattern.hpp; DESIGN.md §3 rule 18) in the two readers of either kind of
// line, on the host: wherever the compact reader (the device's, here compiled for the host) does not
// answer "host", the generic reader gives the same status, bit-equal values, the same id span and
// hash; every unmutated line in the compact layout is taken by the compact reader and carries the
// instant that was written; and the compact reader reads no byte outside [line start, line start +
// 256): every line is parsed from a heap block of exactly 256 bytes, so AddressSanitizer reports
// any byte read past it.
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

static const char* kPatterns[8] = {
    "yyyy-MM-dd'T'HH:mm:ssZZ",      "yyyy-MM-dd'T'HH:mm:ss.SSSZZ", "yyyyMMddHHmmss",       "dd/MMM/yyyy HH:mm:ss",
    "M/d/yy h:mm:ss a",             "yyyy-DDD'T'kk:mm:ssZ",        "d MMMM yyyy HH:mm:ss.SSSSSS", "yyyy-MM-dd KK:mm a"};
static const char* kShort[12] = {"Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"};
static const char* kFull[12] = {"January", "February", "March",     "April",   "May",      "June",
                                "July",    "August",   "September", "October", "November", "December"};

struct Instant { int y, mo, d, doy, h, mi, s, ms, off; };   // off: minutes

static int month_len(int y, int m) {
  static const int len[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 29 : len[m - 1];
}

static Instant instant(std::mt19937_64& r, int pattern) {
  Instant t;
  t.y = pattern == 4 ? 1969 + (int)(r() % 100) : 1930 + (int)(r() % 171);
  t.mo = 1 + (int)(r() % 12);
  t.d = 1 + (int)(r() % (unsigned)month_len(t.y, t.mo));
  t.doy = t.d;
  for (int m = 1; m < t.mo; ++m) t.doy += month_len(t.y, m);
  t.h = (int)(r() % 24); t.mi = (int)(r() % 60); t.s = (int)(r() % 60);
  t.ms = r() % 3 ? (int)(r() % 1000) : 0;
  t.off = r() % 3 ? 0 : (int)(r() % 2879) - 1439;
  return t;
}

static std::string offset(const Instant& t, bool colon, bool zulu) {
  if (t.off == 0 && zulu) return "Z";
  char b[16];
  const int a = t.off < 0 ? -t.off : t.off;
  std::snprintf(b, sizeof b, colon ? "%c%02d:%02d" : "%c%02d%02d", t.off < 0 ? '-' : '+', a / 60, a % 60);
  return b;
}

// the text of t under pattern p, and the instant it states in *want
static std::string render(std::mt19937_64& r, int p, const Instant& t, double* want) {
  char b[96];
  const bool zulu = r() % 2;
  int64_t secs = sv::days_from_civil(t.y, t.mo, t.d) * 86400 + t.h * 3600 + t.mi * 60 + t.s;
  int ms = 0;
  switch (p) {
    case 0: std::snprintf(b, sizeof b, "%04d-%02d-%02dT%02d:%02d:%02d%s", t.y, t.mo, t.d, t.h, t.mi, t.s, offset(t, true, zulu).c_str()); secs -= t.off * 60; break;
    case 1: std::snprintf(b, sizeof b, "%04d-%02d-%02dT%02d:%02d:%02d.%03d%s", t.y, t.mo, t.d, t.h, t.mi, t.s, t.ms, offset(t, true, zulu).c_str()); secs -= t.off * 60; ms = t.ms; break;
    case 2: std::snprintf(b, sizeof b, "%04d%02d%02d%02d%02d%02d", t.y, t.mo, t.d, t.h, t.mi, t.s); break;
    case 3: std::snprintf(b, sizeof b, "%02d/%s/%04d %02d:%02d:%02d", t.d, kShort[t.mo - 1], t.y, t.h, t.mi, t.s); break;
    case 4: std::snprintf(b, sizeof b, "%d/%d/%02d %d:%02d:%02d %s", t.mo, t.d, t.y % 100, t.h % 12 ? t.h % 12 : 12, t.mi, t.s, t.h >= 12 ? "PM" : "AM"); break;
    case 5: std::snprintf(b, sizeof b, "%04d-%03dT%02d:%02d:%02d%s", t.y, t.doy, t.h ? t.h : 24, t.mi, t.s, offset(t, false, zulu).c_str()); secs -= t.off * 60; break;
    case 6: std::snprintf(b, sizeof b, "%d %s %04d %02d:%02d:%02d.%03d%03d", t.d, kFull[t.mo - 1], t.y, t.h, t.mi, t.s, t.ms, (int)(r() % 1000)); ms = t.ms; break;
    default: std::snprintf(b, sizeof b, "%04d-%02d-%02d %02d:%02d %s", t.y, t.mo, t.d, t.h % 12, t.mi, t.h >= 12 ? "pm" : "AM"); secs -= t.s; break;
  }
  if (secs < 0 && ms > 0) ++secs;
  *want = (double)secs;
  std::string s = b;
  if (r() % 4 == 0)   // names and half days in any case
    for (char& c : s) c = r() % 2 ? (char)std::toupper((unsigned char)c) : (char)std::tolower((unsigned char)c);
  if (p == 0 || p == 1 || p == 5)   // ... but the literal T and Z are bytes of the pattern
    for (char& c : s) if (c == 't' || c == 'z') c = (char)std::toupper((unsigned char)c);
  return s;
}

static std::string number(std::mt19937_64& r, double lo, double hi) {
  char b[32];
  std::snprintf(b, sizeof b, r() % 2 ? "%.6f" : "%.1f", lo + (hi - lo) * (double)(r() % 1000000) / 1e6);
  return b;
}

static std::string make_line(std::mt19937_64& r, const msg::Format& f, int p, double* want) {
  const Instant t = instant(r, p);
  const std::string tm = render(r, p, t, want), id = "veh" + std::to_string(r() % 500);
  const std::string la = number(r, -90, 90), lo = number(r, -180, 180), ac = number(r, 0, 3000);
  std::string s;
  if (f.kind == 1) {
    std::vector<std::string> mem = {"\"id\":\"" + id + "\"", "\"timestamp\":\"" + tm + "\"", "\"latitude\":" + la, "\"longitude\":" + lo,
                                    "\"accuracy\":" + ac};
    if (r() % 2) mem.push_back("\"speed\":12.5");
    for (size_t i = mem.size(); i > 1; --i) std::swap(mem[i - 1], mem[r() % i]);
    s = "{";
    for (size_t i = 0; i < mem.size(); ++i) s += (i ? "," : "") + mem[i];
    s += "}";
  } else {
    s = id + "|" + tm + "|" + la + "|" + lo + "|" + ac;
  }
  if (r() % 5 == 0) s += '\r';
  return s;
}

static void mutate(std::mt19937_64& r, std::string& s) {
  static const char pool[] = "0123456789.-+: \t\r\nZTxX_/,|\"\\{}aApPmM";
  const int n = 1 + (int)(r() % 2);
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
  tp::Pattern pat[8];
  for (int p = 0; p < 8; ++p) {
    std::string err;
    CHECK(tp::compile(kPatterns[p], pat[p], err));
    CHECK(!std::strcmp(pat[p].text, kPatterns[p]));
  }
  {   // formats: an id needs its program; a separator inside the pattern's literals
    sv::Format f = sv::default_format();
    f.sep = '|';
    f.time_format = 16;
    CHECK(*sv::format_error(f));
    CHECK(!*sv::format_error(f, &pat[0].prog));
    f.time_format = 2;
    CHECK(*sv::format_error(f, &pat[0].prog));
    f.time_format = 16;
    f.sep = '-';
    CHECK(*sv::format_error(f, &pat[0].prog));
    CHECK(!*sv::format_error(f, &pat[2].prog));
    msg::Format m = msg::default_format();
    m.kind = 1;
    m.line.time_format = 16;
    m.line.sep = '-';
    CHECK(*msg::format_error(m));
    CHECK(!*msg::format_error(m, &pat[0].prog));
  }
  std::mt19937_64 r(20261021);
  const int kLines = 20000;
  long accepted = 0, points = 0, plain = 0, hosts = 0, generic_bad = 0, bad_time = 0, outside = 0;
  for (int n = 0; n < kLines; ++n) {
    const int p = (n / 2) % 8;
    msg::Format f = msg::default_format();
    f.kind = (n / 16) % 2;
    f.line.sep = '|';
    f.line.time_format = tp::kFirstId + p;
    if (n % 3 == 0) { f.line.use_bbox = 1; f.line.bbox[0] = -45; f.line.bbox[1] = -90; f.line.bbox[2] = 45; f.line.bbox[3] = 90; }
    const msg::Keys keys = msg::make_keys(f);
    const bool mutated = n % 2 == 1;
    double want = 0.0;
    std::string s = make_line(r, f, p, &want);
    if (mutated) mutate(r, s);
    // the text as the device sees it: the line, its '\n', then whatever follows, in a block of
    // exactly sv::kMaxLine bytes
    std::string text = s + "\n";
    double other = 0.0;
    while (text.size() < sv::kMaxLine) text += make_line(r, f, p, &other) + "\n";
    uint8_t* blk = (uint8_t*)std::malloc(sv::kMaxLine);
    std::memcpy(blk, text.data(), sv::kMaxLine);
    sv::Line c{};
    const uint32_t st = f.kind == 1 ? msg::compact_json(blk, f.line, keys, c, &pat[p].prog) : sv::compact_line(blk, f.line, c, &pat[p].prog);
    std::free(blk);
    const uint8_t* b = (const uint8_t*)text.data();
    const uint8_t* e = (const uint8_t*)std::memchr(b, '\n', text.size());
    sv::Line g{};
    const char* why = nullptr;
    const uint32_t gs = msg::generic_message(b, e, f, g, &why, &pat[p]);
    generic_bad += gs == sv::kBad;
    CHECK(gs != sv::kBad || why != nullptr);
    if (gs == sv::kBad && why == pat[p].why) ++bad_time;
    CHECK(gs != sv::kHost);
    plain += !mutated;
    if (!mutated) {   // a line in the compact layout: read by the compact reader, to the instant written
      CHECK(st == sv::kPoint || st == sv::kOutside);
      if (st == sv::kPoint) CHECK(c.time == want);
    }
    if (st == sv::kHost) { ++hosts; continue; }
    ++accepted;
    CHECK(st == gs);
    CHECK((size_t)(e - b) + 1 <= sv::kMaxLine);
    outside += st == sv::kOutside;
    if (st != sv::kPoint || gs != sv::kPoint) continue;
    ++points;
    CHECK(std::memcmp(&c.lat, &g.lat, 4) == 0 && std::memcmp(&c.lon, &g.lon, 4) == 0 && std::memcmp(&c.acc, &g.acc, 4) == 0);
    CHECK(std::memcmp(&c.time, &g.time, 8) == 0);
    CHECK(c.id_off == g.id_off && c.id_len == g.id_len && c.hash == g.hash);
  }
  std::printf("lines %d accepted %ld points %ld outside %ld host %ld generic-bad %ld of them the time %ld\n", kLines, accepted, points,
              outside, hosts, generic_bad, bad_time);
#if defined(__SANITIZE_ADDRESS__)
  std::printf("sanitizers: address, undefined\n");
#else
  std::printf("sanitizers: none (the 256-byte bound was not checked in this build)\n");
#endif
  CHECK(plain == kLines / 2 && points > 8000 && outside > 1000 && hosts > 2000 && generic_bad > 2000 && bad_time > 1000);
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("time patterns ok\n");
  return 0;
}
