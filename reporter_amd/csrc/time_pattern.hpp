// time_pattern.hpp — date patterns of the formatter string (DESIGN.md §3 rule 18; reference
// Formatter.java:65,80,104,119 hands the string to Joda's DateTimeFormat).  A pattern compiles once,
// on the host, into a Program of at most 32 steps; match() runs the program over one time text and
// is the only reader of such texts: the host generic readers and the compact readers inside
// k_line_parse (sv_lines.hpp, msg_lines.hpp) both call it, so the value of a text never depends on
// the reader.
//
// A Program is 72 bytes and travels to the kernel by value, like msg::Keys.  Its steps are packed
// 16 bits each, four to a word; step() picks the word with selects over constant indices, so neither
// the program nor anything match() keeps per lane is an array indexed at run time (DESIGN.md §5:
// such arrays go to scratch).  The program is wave-uniform: the step loop and the branch on the
// step's kind are scalar, lanes diverge on their text alone.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "json_points.hpp"
#include "rm_common.hpp"

#if defined(__clang__)
#define RM_TP_UNROLL _Pragma("unroll")
#else
#define RM_TP_UNROLL
#endif

namespace rm {
namespace sv {
RM_HD int64_t days_from_civil(int64_t y, int64_t m, int64_t d);   // sv_lines.hpp
}
namespace tp {

constexpr uint32_t kMaxSteps = 32;     // steps of a program
constexpr uint32_t kMaxPattern = 63;   // bytes of a pattern's text
constexpr uint32_t kMaxText = 64;      // bytes of a time text the compact readers take
constexpr int32_t kFirstId = 16;       // rm_line_format.time_format of the first registered pattern
constexpr int32_t kMaxPatterns = 240;  // patterns of one process

// step kinds: a literal byte, the numeric fields (digits), then the text fields
enum : uint32_t {
  kLit = 0,
  kYear, kYear2, kMonth, kDay, kDoy, kHour, kHour24, kHour12, kHour11, kMinute, kSecond, kFrac,
  kMonthShort, kMonthFull, kHalf, kOffset, kOffsetColon
};
constexpr uint32_t kFirstNumeric = kYear, kLastNumeric = kFrac;
constexpr uint32_t kUsesDoy = 1u, kUsesHalf = 2u;   // Program::flags

// step k: bits 0-4 the kind; a literal's byte in bits 8-15; a numeric field's least and most
// digits in bits 8-11 and 12-15
struct Program {
  uint32_t n;
  uint32_t flags;
  uint64_t w[kMaxSteps / 4];
};
static_assert(sizeof(Program) == 72, "the program is a kernel argument");

RM_HD uint32_t step(const Program& P, uint32_t k) {
  uint64_t w = 0;
  RM_TP_UNROLL
  for (uint32_t j = 0; j < kMaxSteps / 4; ++j) w = (k >> 2) == j ? P.w[j] : w;
  return (uint32_t)(w >> (16u * (k & 3u))) & 0xffffu;
}

// the English month names, lower case: the first three bytes, then the rest of the full name
// (bytes from the low end) and its length.  m is a constant where these are called.
RM_HD uint32_t month_head(uint32_t m) {
  static constexpr uint32_t h[12] = {0x6a616e, 0x666562, 0x6d6172, 0x617072, 0x6d6179, 0x6a756e,
                              0x6a756c, 0x617567, 0x736570, 0x6f6374, 0x6e6f76, 0x646563};
  return h[m];
}
RM_HD uint64_t month_rest(uint32_t m) {
  static constexpr uint64_t r[12] = {0x79726175ull /* uary */, 0x7972617572ull /* ruary */, 0x6863ull /* ch */, 0x6c69ull /* il */,
                              0ull, 0x65ull /* e */, 0x79ull /* y */, 0x747375ull /* ust */,
                              0x7265626d6574ull /* tember */, 0x7265626full /* ober */, 0x7265626d65ull /* ember */,
                              0x7265626d65ull /* ember */};
  return r[m];
}
RM_HD uint32_t month_rest_len(uint32_t m) {
  static constexpr uint32_t l[12] = {4, 5, 2, 2, 0, 1, 1, 3, 6, 4, 5, 5};
  return l[m];
}

RM_HD bool leap(int64_t y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }

// The text t[0, n) under P: consumed exactly, every field in its range -> the instant in whole
// seconds.  Reads no byte outside t[0, n).
RM_HD bool match(const Program& P, const uint8_t* t, uint32_t n, double& out) {
  uint32_t i = 0;
  int64_t year = 0;
  int32_t month = 1, day = 1, doy = 1, hour = 0, minute = 0, sec = 0, ms = 0, pm = 0, off = 0;
  for (uint32_t k = 0; k < P.n; ++k) {
    const uint32_t st = step(P, k), kind = st & 31u;
    if (kind == kLit) {
      if (i >= n || t[i] != (uint8_t)(st >> 8)) return false;
      ++i;
    } else if (kind <= kLastNumeric) {
      const uint32_t least = (st >> 8) & 15u, most = st >> 12;
      uint32_t nd = 0;
      int32_t v = 0, v3 = 0;   // the digits' value; that of the first three, as if three were given
      while (nd < most && i < n && jp::digit(t[i])) {
        const int32_t d = (int32_t)(t[i] - '0');
        v = v * 10 + d;
        if (nd < 3u) v3 = v3 * 10 + d;
        ++i;
        ++nd;
      }
      if (nd < least) return false;
      if (nd < 3u) v3 *= nd == 1u ? 100 : 10;
      if (kind == kYear) {
        year = v;
      } else if (kind == kYear2) {
        year = v + (v >= 69 ? 1900 : 2000);
      } else if (kind == kMonth) {
        if (v < 1 || v > 12) return false;
        month = v;
      } else if (kind == kDay) {
        if (v < 1 || v > 31) return false;
        day = v;
      } else if (kind == kDoy) {
        if (v < 1 || v > 366) return false;
        doy = v;
      } else if (kind == kHour) {
        if (v > 23) return false;
        hour = v;
      } else if (kind == kHour24) {
        if (v < 1 || v > 24) return false;
        hour = v == 24 ? 0 : v;
      } else if (kind == kHour12) {
        if (v < 1 || v > 12) return false;
        hour = v == 12 ? 0 : v;
      } else if (kind == kHour11) {
        if (v > 11) return false;
        hour = v;
      } else if (kind == kMinute) {
        if (v > 59) return false;
        minute = v;
      } else if (kind == kSecond) {
        if (v > 59) return false;
        sec = v;
      } else {
        ms = v3;
      }
    } else if (kind == kMonthShort || kind == kMonthFull) {
      if (i + 3u > n) return false;
      const uint32_t c = ((uint32_t)(t[i] | 0x20u) << 16) | ((uint32_t)(t[i + 1] | 0x20u) << 8) | (uint32_t)(t[i + 2] | 0x20u);
      int32_t m = 0;
      uint64_t rest = 0;
      uint32_t nr = 0;
      RM_TP_UNROLL
      for (uint32_t j = 0; j < 12; ++j) {
        const bool hit = c == month_head(j);
        m = hit ? (int32_t)j + 1 : m;
        rest = hit ? month_rest(j) : rest;
        nr = hit ? month_rest_len(j) : nr;
      }
      if (m == 0) return false;
      i += 3u;
      if (kind == kMonthFull) {
        if (i + nr > n) return false;
        for (uint32_t j = 0; j < nr; ++j, rest >>= 8)
          if ((uint8_t)(t[i + j] | 0x20u) != (uint8_t)rest) return false;
        i += nr;
      }
      month = m;
    } else if (kind == kHalf) {
      if (i + 2u > n || (t[i + 1] | 0x20u) != 'm') return false;
      const uint8_t c = t[i] | 0x20u;
      if (c != 'a' && c != 'p') return false;
      pm = c == 'p';
      i += 2u;
    } else {   // kOffset, kOffsetColon
      if (i < n && t[i] == 'Z') {
        ++i;
        off = 0;
      } else {
        const uint32_t colon = kind == kOffsetColon ? 1u : 0u;
        if (i + 5u + colon > n || (t[i] != '+' && t[i] != '-')) return false;
        const uint32_t q = i + 3u + colon;
        if (!jp::digit(t[i + 1]) || !jp::digit(t[i + 2]) || !jp::digit(t[q]) || !jp::digit(t[q + 1])) return false;
        if (colon && t[i + 3] != ':') return false;
        const int32_t oh = (t[i + 1] - '0') * 10 + (t[i + 2] - '0'), om = (t[q] - '0') * 10 + (t[q + 1] - '0');
        if (oh > 23 || om > 59) return false;
        off = (oh * 3600 + om * 60) * (t[i] == '-' ? -1 : 1);
        i = q + 2u;
      }
    }
  }
  if (i != n) return false;
  const int32_t lp = leap(year) ? 1 : 0;
  int64_t days;
  if (P.flags & kUsesDoy) {
    if (doy > 365 + lp) return false;
    days = sv::days_from_civil(year, 1, 1) + doy - 1;
  } else {
    const int32_t len = month == 2 ? 28 + lp : 30 + ((month + (month >> 3)) & 1);
    if (day > len) return false;
    days = sv::days_from_civil(year, month, day);
  }
  if (P.flags & kUsesHalf) hour += 12 * pm;
  int64_t T = days * 86400 + hour * 3600 + minute * 60 + sec - off;
  if (T < 0 && ms > 0) ++T;   // the milliseconds divided by 1000 as Java's long division: toward zero
  out = (double)T;
  return true;
}

// ---------------------------------------------------------------- host only: the compiler
// a compiled pattern as the registry keeps it
struct Pattern {
  Program prog;
  char text[kMaxPattern + 1];
  char why[kMaxPattern + 24];   // "malformed time (<pattern>)"
};

inline bool has_literal(const Program& P, uint8_t c) {
  for (uint32_t k = 0; k < P.n; ++k) {
    const uint32_t st = step(P, k);
    if ((st & 31u) == kLit && (uint8_t)(st >> 8) == c) return true;
  }
  return false;
}

// pattern -> out; false with the reason in err
inline bool compile(const char* pattern, Pattern& out, std::string& err) {
  const size_t len = std::strlen(pattern);
  if (len > kMaxPattern) { err = "the pattern is longer than 63 bytes"; return false; }
  struct Step { uint32_t kind, lit, letters, natural; };
  Step steps[kMaxSteps];
  uint32_t ns = 0;
  auto push = [&](uint32_t kind, uint32_t lit, uint32_t letters, uint32_t natural) {
    if (ns == kMaxSteps) { err = "the pattern has more than 32 steps"; return false; }
    steps[ns++] = Step{kind, lit, letters, natural};
    return true;
  };
  auto literal = [&](uint8_t c) {
    if (c == '"' || c == '\\' || c < 0x20) { err = "a literal cannot be a double quote, a backslash or a control byte"; return false; }
    return push(kLit, c, 0, 0);
  };
  bool seen[128] = {false};   // by class letter: y M d D H (any hour) a m s S Z
  auto field = [&](char cls, char letter) {
    if (seen[(int)cls]) {
      err = cls == 'H' ? std::string("two hour fields") : std::string("field '") + letter + "' is given twice";
      return false;
    }
    seen[(int)cls] = true;
    return true;
  };
  auto too_long = [&](char letter, uint32_t most) {
    err = std::string("field '") + letter + "' takes at most " + std::to_string(most) + " letters";
    return false;
  };
  for (size_t i = 0; i < len;) {
    const uint8_t c = (uint8_t)pattern[i];
    if (c == '\'') {
      if (pattern[i + 1] == '\'') { if (!literal('\'')) return false; i += 2; continue; }
      size_t j = i + 1;
      for (;; ++j) {
        if (j >= len) { err = "a quote is not closed"; return false; }
        if (pattern[j] == '\'') {
          if (pattern[j + 1] != '\'') break;
          ++j;   // '' inside quoted text: one quote
        }
        if (!literal((uint8_t)pattern[j])) return false;
      }
      i = j + 1;
      continue;
    }
    if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) { if (!literal(c)) return false; ++i; continue; }
    uint32_t r = 1;
    while (pattern[i + r] == (char)c) ++r;
    i += r;
    bool ok = true;
    switch (c) {
      case 'y': if (r > 9) return too_long('y', 9); ok = field('y', 'y') && push(r == 2 ? kYear2 : kYear, 0, r, r == 2 ? 2 : 4); break;
      case 'M':
        if (r > 4) return too_long('M', 4);
        ok = field('M', 'M') && push(r == 3 ? kMonthShort : r == 4 ? kMonthFull : kMonth, 0, r, 2);
        break;
      case 'd': if (r > 2) return too_long('d', 2); ok = field('d', 'd') && push(kDay, 0, r, 2); break;
      case 'D': if (r > 3) return too_long('D', 3); ok = field('D', 'D') && push(kDoy, 0, r, 3); break;
      case 'H': if (r > 2) return too_long('H', 2); ok = field('H', 'H') && push(kHour, 0, r, 2); break;
      case 'k': if (r > 2) return too_long('k', 2); ok = field('H', 'k') && push(kHour24, 0, r, 2); break;
      case 'h': if (r > 2) return too_long('h', 2); ok = field('H', 'h') && push(kHour12, 0, r, 2); seen[(int)'h'] = true; break;
      case 'K': if (r > 2) return too_long('K', 2); ok = field('H', 'K') && push(kHour11, 0, r, 2); seen[(int)'h'] = true; break;
      case 'a': if (r > 1) return too_long('a', 1); ok = field('a', 'a') && push(kHalf, 0, r, 0); break;
      case 'm': if (r > 2) return too_long('m', 2); ok = field('m', 'm') && push(kMinute, 0, r, 2); break;
      case 's': if (r > 2) return too_long('s', 2); ok = field('s', 's') && push(kSecond, 0, r, 2); break;
      case 'S': if (r > 9) return too_long('S', 9); ok = field('S', 'S') && push(kFrac, 0, r, r); break;
      case 'Z':
        if (r > 2) { err = "'ZZZ' (a zone id) is not read"; return false; }
        ok = field('Z', 'Z') && push(r == 2 ? kOffsetColon : kOffset, 0, r, 0);
        break;
      case 'z': case 'E': case 'e': case 'w': case 'x': case 'Y': case 'C': case 'G':
        err = std::string("field '") + (char)c + "' is not read";
        return false;
      default:
        err = std::string("unknown pattern letter '") + (char)c + "'";
        return false;
    }
    if (!ok) return false;
  }
  auto numeric = [](const Step& s) { return s.kind >= kFirstNumeric && s.kind <= kLastNumeric; };
  if (seen[(int)'h'] && !seen[(int)'a']) { err = "'h' and 'K' need 'a'"; return false; }
  if (seen[(int)'a'] && !seen[(int)'h']) { err = "'a' needs 'h' or 'K'"; return false; }
  if (seen[(int)'D'] && (seen[(int)'M'] || seen[(int)'d'])) { err = "'D' cannot stand with 'M' or 'd'"; return false; }
  if (!seen[(int)'y']) { err = "the pattern has no year"; return false; }
  if (!seen[(int)'D'] && !(seen[(int)'M'] && seen[(int)'d'])) { err = "the pattern needs 'D', or both 'M' and 'd'"; return false; }
  if (steps[0].kind == kLit && steps[0].lit == ' ') { err = "the pattern begins with a space"; return false; }
  if (steps[ns - 1].kind == kLit && steps[ns - 1].lit == ' ') { err = "the pattern ends with a space"; return false; }
  std::memset(&out, 0, sizeof out);
  for (uint32_t k = 0; k < ns; ++k) {
    const Step& s = steps[k];
    uint32_t word = s.kind;
    if (s.kind == kLit) {
      word |= s.lit << 8;
    } else if (numeric(s)) {
      const bool adjacent = k + 1 < ns && numeric(steps[k + 1]);
      if (s.kind == kFrac && adjacent) { err = "'S' is directly followed by a numeric field"; return false; }
      uint32_t least = 1, most = s.letters > s.natural ? s.letters : s.natural;
      if (adjacent || s.kind == kYear2) least = most = s.letters;
      word |= (least << 8) | (most << 12);
    }
    out.prog.w[k >> 2] |= (uint64_t)word << (16u * (k & 3u));
  }
  out.prog.n = ns;
  out.prog.flags = (seen[(int)'D'] ? kUsesDoy : 0u) | (seen[(int)'a'] ? kUsesHalf : 0u);
  std::memcpy(out.text, pattern, len);
  std::snprintf(out.why, sizeof out.why, "malformed time (%s)", pattern);
  return true;
}

}  // namespace tp
}  // namespace rm

#undef RM_TP_UNROLL
