// sv_lines.hpp — the rules of separated-value trace lines (DESIGN.md §3 rule 11), as host/device
// functions shared by the device reader (lines.hip k_line_parse), the host reader and the host
// test (tests/cpp/sv_lines_test.cpp), the way json_points.hpp is for the JSON boundary.
//
// One point per line: fields split at a one-byte separator, the columns of the vehicle id, time,
// lat, lon and accuracy named by the format (reference py/simple_reporter.py:100-113 and :137-140,
// Formatter.java:97-109).  Two readers:
//   * generic_line (host): the rule that defines every value.  Whitespace stripped round the line
//     and round every used field, numbers in the grammar [+-](digits[.digits*]|.digits)[e[+-]digits]
//     converted correctly rounded (trace_json.hpp's reader), either time format.
//   * compact_line (host and device): the layout a writer of such files produces.  The line with
//     its '\n' is at most 256 bytes, no whitespace but one '\r' before the '\n' (and the five
//     separator bytes of a format-1 time, which no reader looks at), numbers in jp::number's form
//     (at most 15 digits, no exponent, no '+', digits on both sides of a '.'), an integer time of
//     at most 15 digits.  Everything else is "host": the generic reader reads that line, so what
//     a line yields or fails with never depends on the reader.
// A time_format from 16 up names a registered date pattern (rule 18, time_pattern.hpp): the caller
// resolves it and hands its program to the readers, which then give the stripped time column to
// tp::match; the compact reader takes a time text of at most 64 bytes with no whitespace at its ends.
// Order of the checks in both: enough fields, lat, lon, the bounding box (a point outside is
// dropped whatever its other fields hold, as the reference's `continue` at :105-106), then the
// id, the time and the accuracy.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "json_points.hpp"
#include "rm_common.hpp"
#include "time_pattern.hpp"
#include "trace_json.hpp"

namespace rm {
namespace sv {

// layout of rm_line_format (include/reporter_match.h)
struct Format {
  uint8_t sep;
  int32_t uuid_col, time_col, lat_col, lon_col, acc_col, time_format, accuracy_cap, use_bbox;
  double bbox[4];   // min_lat, min_lon, max_lat, max_lon
};

// what a line is
constexpr uint32_t kBlank = 0, kPoint = 1, kOutside = 2, kHost = 3, kBad = 4;
constexpr uint32_t kMaxLine = 256;   // bytes of a compact line, its '\n' included
constexpr uint32_t kMaxId = 4096;    // bytes of a vehicle id

struct Line {
  double time;
  uint64_t hash;
  float lat, lon, acc;
  uint32_t id_off, id_len;   // the stripped id, from the line's first byte
};

RM_HD bool space(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// 64-bit FNV-1a of the stripped vehicle id
RM_HD uint64_t id_hash(const uint8_t* s, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ (uint64_t)s[i]) * 0x100000001b3ull;
  return h;
}

// days since 1970-01-01 of a proleptic Gregorian date (m 1..12)
RM_HD int64_t days_from_civil(int64_t y, int64_t m, int64_t d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// "YYYY-MM-DD HH:MM:SS" at s[0, 19): digits at the fourteen digit positions, the five separator
// bytes not looked at (simple_reporter.py:108); calendar.timegm's value inside the ranges
RM_HD bool civil_time(const uint8_t* s, double& out) {
  const uint8_t p[14] = {0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18};
  uint32_t v[14];
  for (int k = 0; k < 14; ++k) {
    const uint8_t c = s[p[k]];
    if (!jp::digit(c)) return false;
    v[k] = (uint32_t)(c - '0');
  }
  const int64_t y = v[0] * 1000 + v[1] * 100 + v[2] * 10 + v[3];
  const int64_t mo = v[4] * 10 + v[5], d = v[6] * 10 + v[7], h = v[8] * 10 + v[9], mi = v[10] * 10 + v[11],
                sc = v[12] * 10 + v[13];
  if (mo < 1 || mo > 12 || d < 1 || d > 31 || h > 23 || mi > 59 || sc > 60) return false;
  out = (double)((days_from_civil(y, mo, 1) + d - 1) * 86400 + h * 3600 + mi * 60 + sc);
  return true;
}

RM_HD float accuracy_value(double v, int32_t cap) {
  double a = ::ceil(v);
  if (cap > 0 && a > (double)cap) a = (double)cap;
  return (float)a;
}

RM_HD bool outside(const Format& f, double la, double lo) {
  return f.use_bbox && (la < f.bbox[0] || la > f.bbox[2] || lo < f.bbox[1] || lo > f.bbox[3]);
}

// The compact reader.  s: the line's first byte; reads no byte outside s[0, kMaxLine).
RM_HD uint32_t compact_line(const uint8_t* s, const Format& f, Line& o, const tp::Program* prog = nullptr) {
  const bool t1 = f.time_format == 1;
  const bool tw = t1 || prog;   // whitespace may stand inside the time column
  if (space(f.sep)) return kHost;
  if (tw && (f.time_col == f.uuid_col || f.time_col == f.lat_col || f.time_col == f.lon_col || f.time_col == f.acc_col))
    return kHost;
  uint32_t ub = 0, ue = 0, tb = 0, te = 0, lab = 0, lae = 0, lob = 0, loe = 0, ab = 0, ae = 0;
  uint32_t field = 0, start = 0, end = kMaxLine;
  auto close = [&](uint32_t i) {
    if ((int32_t)field == f.uuid_col) { ub = start; ue = i; }
    if ((int32_t)field == f.time_col) { tb = start; te = i; }
    if ((int32_t)field == f.lat_col) { lab = start; lae = i; }
    if ((int32_t)field == f.lon_col) { lob = start; loe = i; }
    if ((int32_t)field == f.acc_col) { ab = start; ae = i; }
  };
  for (uint32_t i = 0; i < kMaxLine; ++i) {
    const uint8_t c = s[i];
    if (c == '\n') { end = i; break; }
    if (c == '\r' && i + 1 < kMaxLine && s[i + 1] == '\n') { end = i; break; }
    if (c == f.sep) { close(i); ++field; start = i + 1; continue; }
    if (space(c) && !(tw && (int32_t)field == f.time_col)) return kHost;
  }
  if (end == kMaxLine) return kHost;   // no '\n' within reach
  if (end == 0) return kBlank;
  close(end);
  int32_t need = f.uuid_col;
  need = f.time_col > need ? f.time_col : need;
  need = f.lat_col > need ? f.lat_col : need;
  need = f.lon_col > need ? f.lon_col : need;
  need = f.acc_col > need ? f.acc_col : need;
  if ((int32_t)field < need) return kHost;
  double la = 0.0, lo = 0.0;
  uint64_t q = lab;
  if (!jp::number(s, q, lae, la) || q != lae) return kHost;
  q = lob;
  if (!jp::number(s, q, loe, lo) || q != loe) return kHost;
  if (outside(f, la, lo)) return kOutside;
  if (ue == ub) return kHost;
  double tm = 0.0;
  if (prog) {
    const uint32_t nt = te - tb;
    if (nt == 0u || nt > tp::kMaxText || space(s[tb]) || space(s[te - 1u]) || !tp::match(*prog, s + tb, nt, tm)) return kHost;
  } else if (t1) {
    if (te - tb != 19u || !civil_time(s + tb, tm)) return kHost;
  } else {
    uint32_t i = tb;
    const bool neg = i < te && s[i] == '-';
    i += neg;
    const uint32_t nd = te - i;
    if (nd < 1u || nd > 15u) return kHost;
    int64_t v = 0;
    for (; i < te; ++i) {
      if (!jp::digit(s[i])) return kHost;
      v = v * 10 + (int64_t)(s[i] - '0');
    }
    tm = (double)(neg ? -v : v);
  }
  float ac = -1.0f;
  if (f.acc_col >= 0) {
    double a = 0.0;
    q = ab;
    if (!jp::number(s, q, ae, a) || q != ae) return kHost;
    ac = accuracy_value(a, f.accuracy_cap);
  }
  o.lat = (float)la;
  o.lon = (float)lo;
  o.time = tm;
  o.acc = ac;
  o.id_off = ub;
  o.id_len = ue - ub;
  o.hash = id_hash(s + ub, ue - ub);
  return kPoint;
}

// ---------------------------------------------------------------- host only: the generic rule
inline void strip(const uint8_t*& b, const uint8_t*& e) {
  while (b < e && space(*b)) ++b;
  while (e > b && space(e[-1])) --e;
}

// [+-](digits[.digits*] | .digits)[(e|E)[+-]digits] -> the correctly rounded double
inline bool generic_number(const uint8_t* b, const uint8_t* e, double& out) {
  const uint8_t* p = b;
  bool neg = false;
  if (p < e && (*p == '+' || *p == '-')) { neg = *p == '-'; ++p; }
  const uint8_t* i0 = p;
  while (p < e && jp::digit(*p)) ++p;
  const size_t ni = (size_t)(p - i0);
  size_t nf = 0;
  const uint8_t* f0 = p;
  if (p < e && *p == '.') {
    f0 = ++p;
    while (p < e && jp::digit(*p)) ++p;
    nf = (size_t)(p - f0);
  }
  if (ni == 0 && nf == 0) return false;
  const uint8_t* x0 = p;
  if (p < e && (*p == 'e' || *p == 'E')) {
    ++p;
    if (p < e && (*p == '+' || *p == '-')) ++p;
    const uint8_t* d0 = p;
    while (p < e && jp::digit(*p)) ++p;
    if (p == d0) return false;
  }
  if (p != e) return false;
  // the same value in JSON's grammar: no '+', a digit before the '.', digits after it
  std::string tok;
  tok.reserve((size_t)(e - b) + 4);
  if (neg) tok += '-';
  if (ni) tok.append((const char*)i0, ni);
  else tok += '0';
  if (nf) { tok += '.'; tok.append((const char*)f0, nf); }
  tok.append((const char*)x0, (size_t)(e - x0));
  out = tj::Reader::number_value(tok.c_str(), tok.size());
  return true;
}

// One line [b, e) (no '\n' inside) by the generic rule: kBlank, kPoint, kOutside, or kBad with
// the reason in *why.  o.id_off counts from b.
inline uint32_t generic_line(const uint8_t* b, const uint8_t* e, const Format& f, Line& o, const char** why,
                             const tp::Pattern* pat = nullptr) {
  const uint8_t* const line0 = b;
  strip(b, e);
  if (b == e) return kBlank;
  const int32_t cols[5] = {f.uuid_col, f.time_col, f.lat_col, f.lon_col, f.acc_col};
  const uint8_t* fb[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const uint8_t* fe[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int32_t need = 0;
  for (int k = 0; k < 5; ++k) need = cols[k] > need ? cols[k] : need;
  int32_t field = 0;
  const uint8_t* start = b;
  for (const uint8_t* p = b;; ++p) {
    if (p == e || *p == f.sep) {
      for (int k = 0; k < 5; ++k)
        if (cols[k] == field) { fb[k] = start; fe[k] = p; strip(fb[k], fe[k]); }
      if (p == e || field == need) break;   // further fields are ignored
      ++field;
      start = p + 1;
    }
  }
  if (field < need) { *why = "too few fields"; return kBad; }
  double la = 0.0, lo = 0.0;
  if (!generic_number(fb[2], fe[2], la)) { *why = "malformed latitude"; return kBad; }
  if (!generic_number(fb[3], fe[3], lo)) { *why = "malformed longitude"; return kBad; }
  if (outside(f, la, lo)) return kOutside;
  if (fb[0] == fe[0]) { *why = "empty vehicle id"; return kBad; }
  if ((size_t)(fe[0] - fb[0]) > kMaxId) { *why = "vehicle id longer than 4096 bytes"; return kBad; }
  double tm = 0.0;
  if (pat) {
    if (fe[1] - fb[1] > 0xffff || !tp::match(pat->prog, fb[1], (uint32_t)(fe[1] - fb[1]), tm)) { *why = pat->why; return kBad; }
  } else if (f.time_format == 1) {
    if (fe[1] - fb[1] != 19 || !civil_time(fb[1], tm)) { *why = "malformed time (YYYY-MM-DD HH:MM:SS)"; return kBad; }
  } else {
    const uint8_t* p = fb[1];
    bool neg = false;
    if (p < fe[1] && (*p == '+' || *p == '-')) { neg = *p == '-'; ++p; }
    const size_t nd = (size_t)(fe[1] - p);
    if (nd < 1 || nd > 18) { *why = "malformed time (an integer of at most 18 digits)"; return kBad; }
    int64_t v = 0;
    for (; p < fe[1]; ++p) {
      if (!jp::digit(*p)) { *why = "malformed time (an integer of at most 18 digits)"; return kBad; }
      v = v * 10 + (int64_t)(*p - '0');
    }
    tm = (double)(neg ? -v : v);
  }
  float ac = -1.0f;
  if (f.acc_col >= 0) {
    double a = 0.0;
    if (!generic_number(fb[4], fe[4], a)) { *why = "malformed accuracy"; return kBad; }
    ac = accuracy_value(a, f.accuracy_cap);
  }
  o.lat = (float)la;
  o.lon = (float)lo;
  o.time = tm;
  o.acc = ac;
  o.id_off = (uint32_t)(fb[0] - line0);
  o.id_len = (uint32_t)(fe[0] - fb[0]);
  o.hash = id_hash(fb[0], o.id_len);
  return kPoint;
}

inline const char* time_format_error(const Format& f, const tp::Program* prog) {
  if (f.time_format == 0 || f.time_format == 1 || (f.time_format >= tp::kFirstId && prog)) return "";
  return "time_format must be 0 (epoch seconds), 1 (YYYY-MM-DD HH:MM:SS) or an id that rm_time_pattern gave";
}

// "" when the format can be read, else what is wrong with it (prog: the pattern that
// f.time_format names, null when it names none)
inline const char* format_error(const Format& f, const tp::Program* prog = nullptr) {
  if (f.sep == '\n') return "the separator cannot be a newline";
  if (f.uuid_col < 0 || f.time_col < 0 || f.lat_col < 0 || f.lon_col < 0) return "uuid, time, lat and lon columns must be >= 0";
  if (f.acc_col < -1) return "the accuracy column must be >= 0, or -1 for none";
  if (const char* e = time_format_error(f, prog); *e) return e;
  if (prog && tp::has_literal(*prog, f.sep)) return "the time pattern's literals hold the separator";
  if (f.accuracy_cap < 0) return "accuracy_cap must be >= 0";
  return "";
}

inline Format default_format() {
  Format f;
  std::memset(&f, 0, sizeof f);
  f.sep = ',';
  f.uuid_col = 0; f.time_col = 1; f.lat_col = 2; f.lon_col = 3; f.acc_col = 4;
  return f;
}

}  // namespace sv
}  // namespace rm
