// msg_lines.hpp — the rules of stream messages (DESIGN.md §3 rule 14), beside sv_lines.hpp: one raw
// message per line becomes a vehicle key and a point (reference KeyedFormattingProcessor.java,
// Formatter.java:86-124).  A message format is a kind and rule 11's line format; kind 0 is rule 11
// unchanged (sv::generic_line / sv::compact_line), kind 1 is one JSON object per line with five
// named members; under a date pattern (rule 18) the time member is a string that tp::match reads.
// Two readers of kind 1, shared by the device reader (lines.hip k_line_parse<1>),
// the host reader and the host test (tests/cpp/msg_lines_test.cpp):
//   * generic_json (host): the rule that defines every value.  The stripped line is one JSON value
//     (json.hpp) that must be an object; of a repeated key the last wins; lat, lon and accuracy from
//     a number node or a string node holding a number, the time from either, the id from a string
//     node without an escape or an integer number token.
//   * compact_json (host and device): what a writer of such messages produces.  '{', members
//     "key":value with single commas, '}', at most one '\r', the '\n'; no whitespace outside
//     strings; strings without '"', '\' and bytes below 0x20; values are numbers in jp::number's
//     form, such strings, true, false or null; each used key exactly once.  Everything else is
//     "host": the generic reader reads that line, so what a line yields never depends on the reader.
// Order of the checks in both: the object, every used key present, lat, lon, the bounding box, then
// the id, the time and the accuracy (rule 11's order).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "json.hpp"
#include "sv_lines.hpp"

#if defined(__clang__)
#define RM_UNROLL _Pragma("unroll")
#else
#define RM_UNROLL
#endif

namespace rm {
namespace msg {

constexpr uint32_t kKeyBytes = 32;   // a key with its NUL
constexpr int kId = 0, kLat = 1, kLon = 2, kTime = 3, kAcc = 4;

// layout of rm_message_format (include/reporter_match.h)
struct Format {
  int32_t kind;   // 0 separated values, 1 JSON
  int32_t pad;
  sv::Format line;
  char key[5][kKeyBytes];   // id, lat, lon, time, accuracy ("" : none)
};

// the five keys as the compact reader compares them: length and FNV-1a first, bytes on a hit.
// Passed to the kernel by value (uniform: they sit in the kernel arguments, not in a table in HBM).
struct Keys {
  uint64_t hash[5];
  uint32_t len[5];
  uint8_t text[5][kKeyBytes];
};

inline Keys make_keys(const Format& f) {
  Keys k;
  std::memset(&k, 0, sizeof k);
  for (int i = 0; i < 5; ++i) {
    k.len[i] = (uint32_t)strnlen(f.key[i], kKeyBytes);
    std::memcpy(k.text[i], f.key[i], k.len[i] < kKeyBytes ? k.len[i] : kKeyBytes - 1);
    k.hash[i] = sv::id_hash(k.text[i], k.len[i] < kKeyBytes ? k.len[i] : kKeyBytes - 1);
  }
  return k;
}

// The compact reader.  s: the line's first byte; reads no byte outside s[0, sv::kMaxLine).
RM_HD uint32_t compact_json(const uint8_t* s, const sv::Format& f, const Keys& K, sv::Line& o, const tp::Program* prog = nullptr) {
  // a byte past the reach reads as NUL, which no state accepts
  auto at = [&](uint32_t i) -> uint8_t { return i < sv::kMaxLine ? s[i] : (uint8_t)0; };
  if (at(0) == '\n' || (at(0) == '\r' && at(1) == '\n')) return sv::kBlank;
  if (at(0) != '{') return sv::kHost;
  uint32_t i = 1, seen = 0;
  uint32_t vb[5] = {0, 0, 0, 0, 0}, ve[5] = {0, 0, 0, 0, 0};
  uint32_t str = 0;   // bit k: member k's value is a string (else a number token)
  if (at(i) == '}') {
    ++i;
  } else {
    for (;;) {
      if (at(i) != '"') return sv::kHost;
      const uint32_t kb = ++i;
      uint64_t h = 0xcbf29ce484222325ull;
      for (;; ++i) {
        const uint8_t c = at(i);
        if (c == '"') break;
        if (c < 0x20 || c == '\\') return sv::kHost;
        h = (h ^ (uint64_t)c) * 0x100000001b3ull;
      }
      const uint32_t kl = i - kb;
      ++i;
      if (at(i) != ':') return sv::kHost;
      ++i;
      int which = -1;
      RM_UNROLL
      for (int k = 0; k < 5; ++k) {
        if (K.len[k] != kl || K.hash[k] != h || kl == 0u) continue;
        bool same = true;   // (constant indices into the keys: scalar values, nothing in scratch)
        RM_UNROLL
        for (uint32_t b = 0; b < kKeyBytes - 1; ++b) same = same && (b >= kl || s[kb + b] == K.text[k][b]);
        if (same) which = k;
      }
      if (which >= 0) {
        if (seen & (1u << which)) return sv::kHost;
        seen |= 1u << which;
      }
      const uint8_t c = at(i);
      uint32_t b0 = i, e0 = i;
      bool is_str = false, scalar = true;
      if (c == '"') {
        b0 = ++i;
        for (;; ++i) {
          const uint8_t d = at(i);
          if (d == '"') break;
          if (d < 0x20 || d == '\\') return sv::kHost;
        }
        e0 = i++;
        is_str = true;
      } else if (c == '-' || jp::digit(c)) {
        const uint32_t d0 = i + (c == '-');
        if (at(d0) == '0' && jp::digit(at(d0 + 1))) return sv::kHost;   // a leading zero: not JSON (the host says so)
        uint64_t q = i;
        double x = 0.0;
        if (!jp::number(s, q, sv::kMaxLine, x)) return sv::kHost;
        i = (uint32_t)q;
        e0 = i;
      } else if (c == 't') {
        if (at(i + 1) != 'r' || at(i + 2) != 'u' || at(i + 3) != 'e') return sv::kHost;
        i += 4;
        scalar = false;
      } else if (c == 'f') {
        if (at(i + 1) != 'a' || at(i + 2) != 'l' || at(i + 3) != 's' || at(i + 4) != 'e') return sv::kHost;
        i += 5;
        scalar = false;
      } else if (c == 'n') {
        if (at(i + 1) != 'u' || at(i + 2) != 'l' || at(i + 3) != 'l') return sv::kHost;
        i += 4;
        scalar = false;
      } else {
        return sv::kHost;   // '{', '[' and everything that opens no value
      }
      if (which >= 0) {
        if (!scalar) return sv::kHost;
        RM_UNROLL
        for (int k = 0; k < 5; ++k) {   // (constant indices: the spans stay in registers on the device)
          const bool hit = which == k;
          vb[k] = hit ? b0 : vb[k];
          ve[k] = hit ? e0 : ve[k];
        }
        if (is_str) str |= 1u << which;
      }
      const uint8_t d = at(i);
      ++i;
      if (d == ',') continue;
      if (d == '}') break;
      return sv::kHost;
    }
  }
  if (at(i) == '\r') ++i;
  if (at(i) != '\n') return sv::kHost;
  const bool has_acc = K.len[kAcc] != 0u;
  const uint32_t need = has_acc ? 31u : 15u;
  if ((seen & need) != need) return sv::kHost;
  if (str & ((1u << kLat) | (1u << kLon) | (1u << kAcc))) return sv::kHost;
  double la = 0.0, lo = 0.0;
  uint64_t q = vb[kLat];
  if (!jp::number(s, q, ve[kLat], la) || q != ve[kLat]) return sv::kHost;
  q = vb[kLon];
  if (!jp::number(s, q, ve[kLon], lo) || q != ve[kLon]) return sv::kHost;
  if (sv::outside(f, la, lo)) return sv::kOutside;
  if (!(str & (1u << kId)) || ve[kId] == vb[kId]) return sv::kHost;
  double tm = 0.0;
  if (prog) {
    const uint32_t nt = ve[kTime] - vb[kTime];
    if (!(str & (1u << kTime)) || nt > tp::kMaxText || !tp::match(*prog, s + vb[kTime], nt, tm)) return sv::kHost;
  } else if (f.time_format == 1) {
    if (!(str & (1u << kTime)) || ve[kTime] - vb[kTime] != 19u || !sv::civil_time(s + vb[kTime], tm)) return sv::kHost;
  } else {
    if (str & (1u << kTime)) return sv::kHost;
    uint32_t p = vb[kTime];
    const uint32_t e = ve[kTime];
    const bool neg = p < e && s[p] == '-';
    p += neg;
    const uint32_t nd = e - p;
    if (nd < 1u || nd > 15u) return sv::kHost;
    int64_t v = 0;
    for (; p < e; ++p) {
      if (!jp::digit(s[p])) return sv::kHost;
      v = v * 10 + (int64_t)(s[p] - '0');
    }
    tm = (double)(neg ? -v : v);
  }
  float ac = -1.0f;
  if (has_acc) {
    double a = 0.0;
    q = vb[kAcc];
    if (!jp::number(s, q, ve[kAcc], a) || q != ve[kAcc]) return sv::kHost;
    ac = sv::accuracy_value(a, f.accuracy_cap);
  }
  o.lat = (float)la;
  o.lon = (float)lo;
  o.time = tm;
  o.acc = ac;
  o.id_off = vb[kId];
  o.id_len = ve[kId] - vb[kId];
  o.hash = sv::id_hash(s + vb[kId], o.id_len);
  return sv::kPoint;
}

// ---------------------------------------------------------------- host only: the generic rule
// the raw spans [vb, ve) of the top-level members' values of a line that json.hpp has accepted
// as an object, in member order
inline void member_spans(const uint8_t* b, const uint8_t* e, std::vector<std::pair<const uint8_t*, const uint8_t*>>& out) {
  auto ws = [&](const uint8_t*& p) { while (p < e && (*p == ' ' || *p == '\t' || *p == '\r')) ++p; };
  auto skip_string = [&](const uint8_t*& p) {   // p on the opening quote
    for (++p; p < e && *p != '"'; ++p)
      if (*p == '\\') ++p;
    ++p;
  };
  const uint8_t* p = b;
  ws(p);
  ++p;   // '{'
  for (;;) {
    ws(p);
    if (p >= e || *p != '"') return;   // '}' of an empty object
    skip_string(p);
    ws(p);
    ++p;   // ':'
    ws(p);
    const uint8_t* v0 = p;
    if (*p == '"') {
      skip_string(p);
    } else {
      int depth = 0;
      for (; p < e; ++p) {
        if (*p == '"') { skip_string(p); --p; continue; }
        if (*p == '{' || *p == '[') ++depth;
        else if (*p == '}' || *p == ']') { if (depth == 0) break; --depth; }
        else if (depth == 0 && (*p == ',' || *p == ' ' || *p == '\t' || *p == '\r')) break;
      }
    }
    out.emplace_back(v0, p);
    ws(p);
    if (p >= e || *p != ',') return;
    ++p;
  }
}

// json.hpp reads numbers leniently (`01`, `007`, `1.`, `1.e5`); a message holds JSON's own:
// -?(0|[1-9]digits)(.digits)?([eE][+-]?digits)?.  Every number token of a line that json.hpp has
// accepted, nested ones included, is checked against that here.
inline bool strict_numbers(const uint8_t* b, const uint8_t* e) {
  for (const uint8_t* p = b; p < e; ++p) {
    if (*p == '"') {   // a string: no token inside
      for (++p; p < e && *p != '"'; ++p)
        if (*p == '\\') ++p;
      continue;
    }
    if (*p != '-' && !jp::digit(*p)) continue;
    if (*p == '-') ++p;
    if (p >= e || !jp::digit(*p)) return false;
    if (*p == '0' && p + 1 < e && jp::digit(p[1])) return false;   // a leading zero
    while (p < e && jp::digit(*p)) ++p;
    if (p < e && *p == '.') {
      ++p;
      if (p >= e || !jp::digit(*p)) return false;   // a bare dot
      while (p < e && jp::digit(*p)) ++p;
    }
    if (p < e && (*p == 'e' || *p == 'E')) {
      ++p;
      if (p < e && (*p == '+' || *p == '-')) ++p;
      if (p >= e || !jp::digit(*p)) return false;
      while (p < e && jp::digit(*p)) ++p;
    }
    --p;   // (the loop steps past the token's last byte)
  }
  return true;
}

constexpr const char* kWhyTime0 = "malformed time (an integer of at most 18 digits)";
constexpr const char* kWhyTime1 = "malformed time (YYYY-MM-DD HH:MM:SS)";

// One line [b, e) (no '\n' inside) by the generic rule: kBlank, kPoint, kOutside, or kBad with the
// reason in *why.  o.id_off counts from b.
inline uint32_t generic_json(const uint8_t* b, const uint8_t* e, const Format& mf, sv::Line& o, const char** why,
                             const tp::Pattern* pat = nullptr) {
  const sv::Format& f = mf.line;
  const uint8_t* const line0 = b;
  sv::strip(b, e);
  if (b == e) return sv::kBlank;
  if (std::memchr(b, 0, (size_t)(e - b))) { *why = "invalid JSON"; return sv::kBad; }
  json::Value root;
  try {
    root = json::parse(std::string((const char*)b, (size_t)(e - b)).c_str());
  } catch (const std::exception&) {
    *why = "invalid JSON";
    return sv::kBad;
  }
  if (!strict_numbers(b, e)) { *why = "invalid JSON"; return sv::kBad; }
  if (root.type != json::Value::Object) { *why = "not a JSON object"; return sv::kBad; }
  std::vector<std::pair<const uint8_t*, const uint8_t*>> span;
  member_spans(b, e, span);
  if (span.size() != root.obj.size()) { *why = "invalid JSON"; return sv::kBad; }
  const bool has_acc = mf.key[kAcc][0] != 0;
  int at[5] = {-1, -1, -1, -1, -1};
  for (size_t m = 0; m < root.obj.size(); ++m)
    for (int k = 0; k < 5; ++k)
      if ((k != kAcc || has_acc) && root.obj[m].first == mf.key[k]) at[k] = (int)m;   // the last wins
  for (int k = 0; k < (has_acc ? 5 : 4); ++k)
    if (at[k] < 0) { *why = "missing key"; return sv::kBad; }
  auto number = [&](int k, double& out) {
    const json::Value& v = root.obj[(size_t)at[k]].second;
    if (v.type == json::Value::Number) { out = v.num; return true; }
    if (v.type != json::Value::String) return false;
    const uint8_t* sb = (const uint8_t*)v.str.data();
    const uint8_t* se = sb + v.str.size();
    sv::strip(sb, se);
    return sv::generic_number(sb, se, out);
  };
  double la = 0.0, lo = 0.0;
  if (!number(kLat, la)) { *why = "malformed latitude"; return sv::kBad; }
  if (!number(kLon, lo)) { *why = "malformed longitude"; return sv::kBad; }
  if (sv::outside(f, la, lo)) return sv::kOutside;
  // the id: the raw bytes between the quotes, or an integer token's text
  const json::Value& idv = root.obj[(size_t)at[kId]].second;
  const uint8_t* ib = span[(size_t)at[kId]].first;
  const uint8_t* ie = span[(size_t)at[kId]].second;
  if (idv.type == json::Value::String) {
    ++ib; --ie;
    if (std::memchr(ib, '\\', (size_t)(ie - ib))) { *why = "malformed vehicle id"; return sv::kBad; }
  } else if (idv.type == json::Value::Number) {
    const uint8_t* p = ib + (ib < ie && *ib == '-');
    if (p == ie) { *why = "malformed vehicle id"; return sv::kBad; }
    for (; p < ie; ++p)
      if (!jp::digit(*p)) { *why = "malformed vehicle id"; return sv::kBad; }
  } else {
    *why = "malformed vehicle id";
    return sv::kBad;
  }
  if (ib == ie) { *why = "empty vehicle id"; return sv::kBad; }
  if ((size_t)(ie - ib) > sv::kMaxId) { *why = "vehicle id longer than 4096 bytes"; return sv::kBad; }
  const json::Value& tv = root.obj[(size_t)at[kTime]].second;
  double tm = 0.0;
  if (pat) {   // a number node is malformed under a pattern
    if (tv.type != json::Value::String || tv.str.size() > 0xffff ||
        !tp::match(pat->prog, (const uint8_t*)tv.str.data(), (uint32_t)tv.str.size(), tm)) {
      *why = pat->why;
      return sv::kBad;
    }
  } else if (f.time_format == 1) {
    if (tv.type != json::Value::String || tv.str.size() != 19 || !sv::civil_time((const uint8_t*)tv.str.data(), tm)) {
      *why = kWhyTime1;
      return sv::kBad;
    }
  } else if (tv.type == json::Value::Number) {
    const double v = std::trunc(tv.num);
    if (!(std::fabs(v) < 9007199254740992.0)) { *why = kWhyTime0; return sv::kBad; }
    tm = v + 0.0;   // (-0 and -0.4 give +0, as a long does)
  } else if (tv.type == json::Value::String) {
    const uint8_t* p = (const uint8_t*)tv.str.data();
    const uint8_t* pe = p + tv.str.size();
    sv::strip(p, pe);
    bool neg = false;
    if (p < pe && (*p == '+' || *p == '-')) { neg = *p == '-'; ++p; }
    const size_t nd = (size_t)(pe - p);
    if (nd < 1 || nd > 18) { *why = kWhyTime0; return sv::kBad; }
    int64_t v = 0;
    for (; p < pe; ++p) {
      if (!jp::digit(*p)) { *why = kWhyTime0; return sv::kBad; }
      v = v * 10 + (int64_t)(*p - '0');
    }
    tm = (double)(neg ? -v : v);
  } else {
    *why = kWhyTime0;
    return sv::kBad;
  }
  float ac = -1.0f;
  if (has_acc) {
    double a = 0.0;
    if (!number(kAcc, a)) { *why = "malformed accuracy"; return sv::kBad; }
    ac = sv::accuracy_value(a, f.accuracy_cap);
  }
  o.lat = (float)la;
  o.lon = (float)lo;
  o.time = tm;
  o.acc = ac;
  o.id_off = (uint32_t)(ib - line0);
  o.id_len = (uint32_t)(ie - ib);
  o.hash = sv::id_hash(ib, o.id_len);
  return sv::kPoint;
}

// either kind by the generic rule
inline uint32_t generic_message(const uint8_t* b, const uint8_t* e, const Format& mf, sv::Line& o, const char** why,
                                const tp::Pattern* pat = nullptr) {
  return mf.kind == 1 ? generic_json(b, e, mf, o, why, pat) : sv::generic_line(b, e, mf.line, o, why, pat);
}

// "" when the format can be read, else what is wrong with it
inline const char* format_error(const Format& f, const tp::Program* prog = nullptr) {
  if (f.kind != 0 && f.kind != 1) return "kind must be 0 (separated values) or 1 (JSON)";
  if (f.kind == 0) return sv::format_error(f.line, prog);
  if (const char* e = sv::time_format_error(f.line, prog); *e) return e;
  if (f.line.accuracy_cap < 0) return "accuracy_cap must be >= 0";
  for (int k = 0; k < 5; ++k) {
    const size_t n = strnlen(f.key[k], kKeyBytes);
    if (n >= kKeyBytes) return "a key is longer than 31 bytes";
    if (n == 0 && k != kAcc) return "the id, lat, lon and time keys cannot be empty";
    for (size_t i = 0; i < n; ++i) {
      const uint8_t c = (uint8_t)f.key[k][i];
      if (c == '"' || c == '\\' || c < 0x20) return "a key holds a quote, a backslash or a control byte";
    }
    for (int j = 0; j < k; ++j)
      if (n && !std::strncmp(f.key[k], f.key[j], kKeyBytes)) return "two keys are equal";
  }
  return "";
}

inline Format default_format() {
  Format f;
  std::memset(&f, 0, sizeof f);
  f.line = sv::default_format();
  std::strcpy(f.key[kId], "id");
  std::strcpy(f.key[kLat], "latitude");
  std::strcpy(f.key[kLon], "longitude");
  std::strcpy(f.key[kTime], "timestamp");
  std::strcpy(f.key[kAcc], "accuracy");
  return f;
}

}  // namespace msg
}  // namespace rm

#undef RM_UNROLL
