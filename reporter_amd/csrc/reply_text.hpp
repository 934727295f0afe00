// reply_text.hpp — the text of a /report reply (DESIGN.md §3 rule 19; reference
// py/reporter_service.py:79-179, 240-243): the time routine, and one emitter per piece of a reply
// -- head (stats up to "segments":[), segment, middle, report, tail -- written once against a sink.
// The counting sink gives a piece's length and the writing sink its bytes, so the two cannot
// differ; a host sink that appends to a string (reply.hip) gives the same reply with the times
// std::to_chars writes.  Everything is __host__ __device__ and free of HIP types, so the host
// program tests/cpp/reply_text_test.cpp runs exactly the code the kernels of reply.hip run.
#pragma once
#include <stdint.h>

#include "rm_common.hpp"
#include "tile_text.hpp"

namespace rm {

// ---- times: start_time, end_time, t0, t1 ----
// -1 is "-1" and 0 is "0".  A finite 1 <= x < 2^53 is its integer part and the fewest fractional
// digits with which the text parses back to x (never more than 17 significant digits).  Any other
// value is kRtTimeOther: its trace is flagged and written on the host.
enum RtTimeKind : uint32_t { kRtTimeMinusOne = 0, kRtTimeZero = 1, kRtTimeDigits = 2, kRtTimeOther = 3 };
TT_HD uint32_t rt_time_kind(double x) {
  if (x == -1.0) return kRtTimeMinusOne;
  if (x == 0.0) return kRtTimeZero;
  if (x >= 1.0 && x < 9007199254740992.0) return kRtTimeDigits;
  return kRtTimeOther;   // (NaN fails every comparison above)
}

struct RtTime {
  uint64_t ip;     // the integer part
  uint64_t frac;   // the d fractional digits as a number (< 10^d)
  uint32_t d;
};

// x = M / 2^k with M the 53-bit significand (k = 52 - exponent, 0..52), F = M mod 2^k the
// fraction's numerator.  With d digits the nearest decimal is N = round(F 10^d / 2^k); it parses
// back to x when it lies strictly inside x's rounding interval, |N / 10^d - F / 2^k| < 2^-(k+1),
// that is 2 |N 2^k - F 10^d| < 10^d.  (At a power of two the interval below x is half as wide, but
// there F = 0 and d = 0.)  All of it in integers: F 10^d < 2^52 10^17 < 2^109 needs the 128 bits;
// N 2^k - F 10^d is what the rounding shift drops, taken from the sum's low k bits.  d = 17 less
// the integer part's digits always passes (10^17 > 2^54 decimals per binade against 2^52 doubles).
TT_HD RtTime rt_time_digits(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  const uint32_t k = 52u - (uint32_t)(((b >> 52) & 0x7ffull) - 1023ull);
  const uint64_t m = (b & 0xfffffffffffffull) | 0x10000000000000ull;
  RtTime t;
  t.ip = m >> k;
  t.frac = 0;
  t.d = 0;
  const uint64_t mask = (1ull << k) - 1ull;
  const uint64_t f = m & mask;
  if (f == 0ull) return t;
  const uint64_t half = 1ull << (k - 1u);   // (f != 0, so k >= 1)
  uint64_t p10 = 1;
  for (uint32_t d = 1; d <= 17u; ++d) {
    p10 *= 10ull;
    const unsigned __int128 q = (unsigned __int128)f * p10 + half;
    const uint64_t n = (uint64_t)(q >> k);
    const uint64_t r = (uint64_t)q & mask;
    const uint64_t err = r > half ? r - half : half - r;
    t.frac = n;
    t.d = d;
    if (2ull * err < p10 && n < p10) break;
  }
  return t;
}

TT_HD uint32_t rt_time_len(double x, bool& other) {
  const uint32_t kind = rt_time_kind(x);
  if (kind == kRtTimeMinusOne) return 2u;
  if (kind == kRtTimeZero) return 1u;
  if (kind == kRtTimeOther) { other = true; return 1u; }   // a "0" holds the place in a flagged trace
  const RtTime t = rt_time_digits(x);
  return tt_digits(t.ip) + (t.d ? 1u + t.d : 0u);
}
TT_HD uint32_t rt_put_time(char* p, double x, bool& other) {
  const uint32_t kind = rt_time_kind(x);
  if (kind == kRtTimeMinusOne) { p[0] = '-'; p[1] = '1'; return 2u; }
  if (kind == kRtTimeZero) { p[0] = '0'; return 1u; }
  if (kind == kRtTimeOther) { other = true; p[0] = '0'; return 1u; }
  const RtTime t = rt_time_digits(x);
  uint32_t n = tt_put_u64(p, t.ip);
  if (t.d) {
    p[n++] = '.';
    uint64_t v = t.frac;
    for (uint32_t i = t.d; i-- > 0u;) {
      p[n + i] = (char)('0' + (uint32_t)(v % 10ull));
      v /= 10ull;
    }
    n += t.d;
  }
  return n;
}

// ---- stats.*.length: 0 when never assigned (< 0), else the metres as kilometres with exactly
// three decimals (1234 -> 1.234), which parses to Python's round(m * 0.001, 3)
TT_HD uint32_t rt_km_len(int32_t m) { return m < 0 ? 1u : tt_digits((uint64_t)m / 1000ull) + 4u; }
TT_HD uint32_t rt_put_km(char* p, int32_t m) {
  if (m < 0) { p[0] = '0'; return 1u; }
  const uint32_t n = tt_put_u64(p, (uint64_t)m / 1000ull);
  const uint32_t f = (uint32_t)m % 1000u;
  p[n] = '.';
  p[n + 1] = (char)('0' + f / 100u);
  p[n + 2] = (char)('0' + f / 10u % 10u);
  p[n + 3] = (char)('0' + f % 10u);
  return n + 4u;
}

// ---- the two sinks every piece is written against ----
#if defined(__HIP__) || defined(__HIPCC__)
#define RT_M __host__ __device__ __forceinline__
#define RT_HD template <class Sink> __host__ __device__ __forceinline__
#else
#define RT_M inline
#define RT_HD template <class Sink> static inline
#endif
struct RtCount {
  uint32_t n = 0;
  bool other = false;   // a time outside the routine's range was met
  template <uint32_t N> RT_M void lit(const char (&)[N]) { n += N - 1u; }
  RT_M void u64(uint64_t v) { n += tt_digits(v); }
  RT_M void i64(int64_t v) { n += tt_len_i64(v); }
  RT_M void km(int32_t m) { n += rt_km_len(m); }
  RT_M void time(double x) { n += rt_time_len(x, other); }
};
struct RtWrite {
  char* p;
  bool other = false;
  template <uint32_t N> RT_M void lit(const char (&s)[N]) {
    for (uint32_t i = 0; i + 1u < N; ++i) p[i] = s[i];
    p += N - 1u;
  }
  RT_M void u64(uint64_t v) { p += tt_put_u64(p, v); }
  RT_M void i64(int64_t v) { p += tt_put_i64(p, v); }
  RT_M void km(int32_t m) { p += rt_put_km(p, m); }
  RT_M void time(double x) { p += rt_put_time(p, x, other); }
};

// ---- the pieces ----
// {"stats":{...}[,"shape_used":S],"segment_matcher":{"segments":[
RT_HD void rt_head(Sink& s, const ReportStats& st) {
  s.lit("{\"stats\":{\"successful_matches\":{\"count\":"); s.i64(st.successful_count);
  s.lit(",\"length\":"); s.km(st.successful_length_m);
  s.lit("},\"unreported_matches\":{\"count\":"); s.i64(st.unreported_count);
  s.lit(",\"length\":"); s.km(st.unreported_length_m);
  s.lit("},\"match_errors\":{\"discontinuities\":"); s.i64(st.discontinuities);
  s.lit(",\"invalid_speeds\":"); s.i64(st.invalid_speeds);
  s.lit(",\"invalid_times\":"); s.i64(st.invalid_times);
  s.lit("},\"unassociated_segments\":"); s.i64(st.unassociated);
  s.lit("}");
  if (st.shape_used > 0) { s.lit(",\"shape_used\":"); s.i64(st.shape_used); }
  s.lit(",\"segment_matcher\":{\"segments\":[");
}
// the object tj::format_segments writes (same keys, same order), after a comma unless first
RT_HD void rt_segment(Sink& s, const SegmentRec& r, bool first) {
  if (!first) s.lit(",");
  s.lit("{");
  if (r.flags & 2u) { s.lit("\"segment_id\":"); s.u64(r.segment_id); s.lit(","); }
  s.lit("\"way_ids\":["); s.u64(r.way_first);
  if (r.way_last != r.way_first) { s.lit(","); s.u64(r.way_last); }
  s.lit("],\"start_time\":"); s.time(r.start_time);
  s.lit(",\"end_time\":"); s.time(r.end_time);
  s.lit(",\"queue_length\":"); s.i64(r.queue_length);
  s.lit(",\"length\":"); s.i64(r.length);
  if (r.flags & 1u) s.lit(",\"internal\":true"); else s.lit(",\"internal\":false");
  s.lit(",\"begin_shape_index\":"); s.u64(r.begin_shape_index);
  s.lit(",\"end_shape_index\":"); s.u64(r.end_shape_index);
  s.lit("}");
}
// "mode" is the hard-coded auto of reporter_service.py:96,101
RT_HD void rt_middle(Sink& s) { s.lit("],\"mode\":\"auto\"},\"datastore\":{\"mode\":\"auto\",\"reports\":["); }
RT_HD void rt_report(Sink& s, const ReportRec& r, bool first) {
  if (!first) s.lit(",");
  s.lit("{\"id\":"); s.u64(r.id);
  s.lit(",\"t0\":"); s.time(r.t0);
  s.lit(",\"t1\":"); s.time(r.t1);
  s.lit(",\"length\":"); s.i64(r.length);
  s.lit(",\"queue_length\":"); s.i64(r.queue_length);
  if (r.next_id != kInvalidSegmentId) { s.lit(",\"next_id\":"); s.u64(r.next_id); }
  s.lit("}");
}
RT_HD void rt_tail(Sink& s) { s.lit("]}}"); }

// One trace's reply is S + R + 3 items: the head, its S segments, the middle, its R reports, the
// tail.  Item j of the trace against a sink:
RT_HD void rt_item(Sink& s, uint32_t j, const SegmentRec* segs, uint32_t S, const ReportRec* reps, uint32_t R,
                   const ReportStats& st) {
  if (j == 0u) rt_head(s, st);
  else if (j <= S) rt_segment(s, segs[j - 1u], j == 1u);
  else if (j == S + 1u) rt_middle(s);
  else if (j <= S + 1u + R) rt_report(s, reps[j - S - 2u], j == S + 2u);
  else rt_tail(s);
}

// the longest piece: the head with every number at its longest (the i32 minimum, 2147483.647)
constexpr uint32_t kRtMaxTime = 18;   // 17 significant digits and the point
constexpr uint32_t kRtMaxHead = 236 + 6 * 11 + 2 * 11 + 10;
constexpr uint32_t kRtMaxSegment = 139 + 20 + 2 * 10 + 2 * kRtMaxTime + 2 * 11 + 2 * 10;
constexpr uint32_t kRtMaxReport = 57 + 2 * 20 + 2 * kRtMaxTime + 2 * 11;
constexpr uint32_t kRtMaxPiece = kRtMaxHead;
static_assert(kRtMaxSegment <= kRtMaxPiece && kRtMaxReport <= kRtMaxPiece, "the head is the longest piece");

}  // namespace rm
