// The text routines of a /report reply (reporter_amd/csrc/reply_text.hpp) on the host: the same
// code the kernels of reply.hip run.  The time routine over powers of two and their neighbours,
// every digit count, epoch-sized values with 0..7 fractional digits and 200,000 seeded log-uniform
// values of [1, 2^53): the length function equals the bytes written, the text parses back to the
// value, has at most 17 significant digits, and does not parse back with one fractional digit
// fewer; nothing is written outside a guarded buffer.  Every piece writer against an
// snprintf-built expectation at the field extremes.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "reply_text.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);             \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

constexpr size_t kGuard = 64, kBuf = 1024;
constexpr unsigned char kFill = 0xA5;

// run `put` at offsets of a guarded buffer; the bytes written must be `want` and every other byte
// must keep the fill
template <class F>
static void guarded(const std::string& want, uint32_t said_len, F put, size_t offsets = 17) {
  CHECK(said_len == want.size());
  for (size_t off = 0; off < offsets; ++off) {
    std::vector<unsigned char> b(kGuard + kBuf + kGuard, kFill);
    char* p = (char*)b.data() + kGuard + off;
    const uint32_t n = put(p);
    CHECK(n == want.size());
    CHECK(std::memcmp(p, want.data(), want.size()) == 0);
    for (size_t i = 0; i < b.size(); ++i) {
      const bool inside = i >= kGuard + off && i < kGuard + off + want.size();
      if (!inside) CHECK(b[i] == kFill);
    }
  }
}

static uint64_t g_times = 0;
static uint32_t g_max_sig = 0, g_max_len = 0;

// one value of the routine's range
static void check_time(double x, size_t offsets = 1) {
  CHECK(rt_time_kind(x) == kRtTimeDigits);
  bool other = false;
  const uint32_t len = rt_time_len(x, other);
  CHECK(!other && len >= 1 && len <= kRtMaxTime);
  unsigned char b[kGuard + 32 + kGuard];
  for (size_t off = 0; off < offsets; ++off) {
    std::memset(b, kFill, sizeof b);
    char* p = (char*)b + kGuard + off;
    const uint32_t n = rt_put_time(p, x, other);
    CHECK(n == len && !other);
    for (size_t i = 0; i < sizeof b; ++i)
      if (i < kGuard + off || i >= kGuard + off + len) CHECK(b[i] == kFill);
    if (off) continue;
    const std::string text(p, n);
    CHECK(std::strtod(text.c_str(), nullptr) == x);
    const size_t dot = text.find('.');
    const uint32_t sig = (uint32_t)(dot == std::string::npos ? text.size() : text.size() - 1);
    CHECK(sig <= 17);
    CHECK(text[0] != '0' && text.find_first_not_of("0123456789.") == std::string::npos);
    if (sig > g_max_sig) g_max_sig = sig;
    if (len > g_max_len) g_max_len = len;
    if (dot != std::string::npos) {   // the correctly rounded text with one digit fewer is another double
      const int d = (int)(text.size() - dot - 1);
      CHECK(d >= 1 && text.back() != '0');
      char fewer[400];
      std::snprintf(fewer, sizeof fewer, "%.*f", d - 1, x);
      CHECK(std::strtod(fewer, nullptr) != x);
    } else {
      CHECK(x == std::floor(x));
    }
  }
  ++g_times;
}

// the shortest "%.*f" that parses back: libc's answer for values without a rounding tie
static std::string time_want(double x) {
  if (x == -1.0) return "-1";
  if (x == 0.0) return "0";
  char buf[400];
  for (int d = 0; d <= 17; ++d) {
    std::snprintf(buf, sizeof buf, "%.*f", d, x);
    if (std::strtod(buf, nullptr) == x) return buf;
  }
  CHECK(false);
  return buf;
}

static std::string km_want(int32_t m) {
  if (m < 0) return "0";
  char buf[32];
  std::snprintf(buf, sizeof buf, "%d.%03d", m / 1000, m % 1000);
  return buf;
}

static std::string head_want(const ReportStats& s) {
  char buf[1024], shape[64] = "";
  if (s.shape_used > 0) std::snprintf(shape, sizeof shape, ",\"shape_used\":%d", s.shape_used);
  std::snprintf(buf, sizeof buf,
                "{\"stats\":{\"successful_matches\":{\"count\":%d,\"length\":%s},\"unreported_matches\":{\"count\":%d,"
                "\"length\":%s},\"match_errors\":{\"discontinuities\":%d,\"invalid_speeds\":%d,\"invalid_times\":%d},"
                "\"unassociated_segments\":%d}%s,\"segment_matcher\":{\"segments\":[",
                s.successful_count, km_want(s.successful_length_m).c_str(), s.unreported_count,
                km_want(s.unreported_length_m).c_str(), s.discontinuities, s.invalid_speeds, s.invalid_times, s.unassociated, shape);
  return buf;
}

static std::string segment_want(const SegmentRec& r, bool first) {
  char buf[1024], id[64] = "", way2[32] = "";
  if (r.flags & 2u) std::snprintf(id, sizeof id, "\"segment_id\":%" PRIu64 ",", r.segment_id);
  if (r.way_last != r.way_first) std::snprintf(way2, sizeof way2, ",%u", r.way_last);
  std::snprintf(buf, sizeof buf,
                "%s{%s\"way_ids\":[%u%s],\"start_time\":%s,\"end_time\":%s,\"queue_length\":%d,\"length\":%d,\"internal\":%s,"
                "\"begin_shape_index\":%u,\"end_shape_index\":%u}",
                first ? "" : ",", id, r.way_first, way2, time_want(r.start_time).c_str(), time_want(r.end_time).c_str(),
                r.queue_length, r.length, (r.flags & 1u) ? "true" : "false", r.begin_shape_index, r.end_shape_index);
  return buf;
}

static std::string report_want(const ReportRec& r, bool first) {
  char buf[1024], nxt[64] = "";
  if (r.next_id != kInvalidSegmentId) std::snprintf(nxt, sizeof nxt, ",\"next_id\":%" PRIu64, r.next_id);
  std::snprintf(buf, sizeof buf, "%s{\"id\":%" PRIu64 ",\"t0\":%s,\"t1\":%s,\"length\":%d,\"queue_length\":%d%s}", first ? "" : ",",
                r.id, time_want(r.t0).c_str(), time_want(r.t1).c_str(), r.length, r.queue_length, nxt);
  return buf;
}

template <class F>
static void piece(const std::string& want, uint32_t max_len, F emit) {
  CHECK(want.size() <= max_len && want.size() <= kRtMaxPiece);
  RtCount c;
  emit(c);
  CHECK(!c.other);
  guarded(want, c.n, [&](char* q) {
    RtWrite w{q};
    emit(w);
    CHECK(!w.other);
    return (uint32_t)(w.p - q);
  });
}

int main() {
  // ---- the time routine
  for (int e = 0; e <= 52; ++e) {
    const double p = std::ldexp(1.0, e);
    check_time(p, 17);
    check_time(std::nextafter(p, 1e300), 17);
    if (e) check_time(std::nextafter(p, 0.0), 17);
  }
  check_time(9007199254740991.0, 17);                    // 2^53 - 1
  check_time(std::nextafter(9007199254740992.0, 0.0));   // the largest double below 2^53
  {
    double p = 1.0;
    for (int k = 1; k <= 16; ++k) {   // one integer of every digit count, and both edges
      check_time(p);
      check_time(p * 7.0 < 9007199254740992.0 ? p * 7.0 : p * 9.0);
      if (k > 1) check_time(p - 1.0);
      p *= 10.0;
    }
  }
  {
    const char* epoch[] = {"1500000000", "1483228960.1", "1483228960.13", "1483228960.135", "1483228960.1354",
                           "1483228960.13549", "1483228960.135494", "1483228960.1354945"};
    for (int d = 0; d <= 7; ++d) {
      const double x = std::strtod(epoch[d], nullptr);
      check_time(x, 17);
      bool other = false;
      char buf[32];
      const uint32_t n = rt_put_time(buf, x, other);
      CHECK(std::string(buf, n) == epoch[d]);   // the digits it was written with
    }
  }
  {
    uint64_t s = 0x9E3779B97F4A7C15ull;   // splitmix64
    auto next = [&] {
      uint64_t z = (s += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      return z ^ (z >> 31);
    };
    for (int i = 0; i < 200000; ++i) {   // log-uniform: a uniform exponent 0..52 and a uniform significand
      const uint64_t r = next();
      const uint64_t bits = ((1023ull + (r >> 52) % 53ull) << 52) | (next() & 0xfffffffffffffull);
      double x;
      std::memcpy(&x, &bits, 8);
      check_time(x);
    }
  }
  CHECK(g_max_sig == 17 && g_max_len == kRtMaxTime);
  // ---- what the routine does not take, and the two fixed texts
  {
    const double outside[] = {-2.0, -1.5, 0.5, 0.999999, 9007199254740992.0, 1e300, HUGE_VAL, -HUGE_VAL, std::nan(""), 5e-324};
    for (double x : outside) {
      CHECK(rt_time_kind(x) == kRtTimeOther);
      bool o1 = false, o2 = false;
      char buf[8];
      CHECK(rt_time_len(x, o1) == 1 && o1);
      CHECK(rt_put_time(buf, x, o2) == 1 && o2 && buf[0] == '0');
    }
    bool other = false;
    guarded("-1", rt_time_len(-1.0, other), [&](char* q) { return rt_put_time(q, -1.0, other); });
    guarded("0", rt_time_len(0.0, other), [&](char* q) { return rt_put_time(q, 0.0, other); });
    CHECK(!other);
  }
  // ---- kilometres with three decimals
  for (int32_t m : {-1, -2147483647 - 1, 0, 1, 9, 10, 99, 100, 999, 1000, 1234, 500, 10000, 999999, 1000000, 2147483647})
    guarded(km_want(m), rt_km_len(m), [&](char* q) { return rt_put_km(q, m); });
  // ---- the pieces at the field extremes
  const int32_t i32s[] = {0, 1, 7, 1234, 999999, 2147483647, (int32_t)(-2147483647 - 1), -1};
  uint64_t pieces = 0;
  for (int32_t a : i32s)
    for (int32_t b : {0, -1, 15, 2147483647}) {
      ReportStats st;
      st.successful_count = a; st.unreported_count = a ^ 1; st.successful_length_m = b; st.unreported_length_m = a;
      st.discontinuities = a; st.invalid_speeds = b; st.invalid_times = a; st.unassociated = a; st.shape_used = b;
      st.n_reports = 0;
      piece(head_want(st), kRtMaxHead, [&](auto& s) { rt_head(s, st); });
      ++pieces;
    }
  {
    ReportStats st;   // every number at its longest
    st.successful_count = st.unreported_count = st.discontinuities = st.invalid_speeds = st.invalid_times = st.unassociated =
        (int32_t)(-2147483647 - 1);
    st.successful_length_m = st.unreported_length_m = st.shape_used = 2147483647;
    st.n_reports = 0;
    CHECK(head_want(st).size() == kRtMaxHead);
    piece(head_want(st), kRtMaxHead, [&](auto& s) { rt_head(s, st); });
  }
  const double times[] = {-1.0, 0.0, 1.0, 1500000000.0, 1483228960.135494, 1483228960.1354945, 9007199254740991.0,
                          1.0000000000000002};
  const uint64_t ids[] = {0ull, 7ull, kInvalidSegmentId, kInvalidSegmentId - 1, 0xffffffffffffffffull};
  const uint32_t ways[] = {0u, 1u, 0xffffffffu, 4000000000u};
  for (uint64_t id : ids)
    for (uint32_t w : ways)
      for (int t = 0; t < 8; ++t)
        for (uint32_t flags = 0; flags < 4; ++flags) {
          SegmentRec r;
          std::memset(&r, 0, sizeof r);
          r.segment_id = id; r.flags = flags;
          r.way_first = w; r.way_last = (t & 1) ? w : ways[(t + 1) % 4];   // one way id, or two
          r.start_time = times[t]; r.end_time = times[(t + 3) % 8];
          r.length = i32s[t]; r.queue_length = i32s[(t + 5) % 8];
          r.begin_shape_index = w; r.end_shape_index = ~w;
          for (int first = 0; first < 2; ++first)
            piece(segment_want(r, first), kRtMaxSegment, [&](auto& s) { rt_segment(s, r, first); });
          ReportRec q;
          std::memset(&q, 0, sizeof q);
          q.id = id; q.next_id = ids[(t + flags) % 5];
          q.t0 = times[t]; q.t1 = times[(t + 1) % 8];
          q.length = i32s[(t + 2) % 8]; q.queue_length = i32s[t];
          for (int first = 0; first < 2; ++first)
            piece(report_want(q, first), kRtMaxReport, [&](auto& s) { rt_report(s, q, first); });
          pieces += 4;
        }
  {
    SegmentRec r;   // the longest segment and report
    std::memset(&r, 0, sizeof r);
    r.segment_id = 0xffffffffffffffffull; r.flags = 2u; r.way_first = 0xffffffffu; r.way_last = 0xfffffffeu;
    r.start_time = r.end_time = 1483228960.1354945;   // 17 significant digits
    r.length = r.queue_length = (int32_t)(-2147483647 - 1);
    r.begin_shape_index = r.end_shape_index = 0xffffffffu;
    CHECK(segment_want(r, false).size() == kRtMaxSegment);
    ReportRec q;
    std::memset(&q, 0, sizeof q);
    q.id = q.next_id = 0xffffffffffffffffull; q.t0 = q.t1 = 1483228960.1354945;
    q.length = q.queue_length = (int32_t)(-2147483647 - 1);
    CHECK(report_want(q, false).size() == kRtMaxReport);
  }
  piece("],\"mode\":\"auto\"},\"datastore\":{\"mode\":\"auto\",\"reports\":[", kRtMaxPiece, [&](auto& s) { rt_middle(s); });
  piece("]}}", kRtMaxPiece, [&](auto& s) { rt_tail(s); });
  // ---- the items of one trace in order are its reply
  {
    SegmentRec segs[2];
    std::memset(segs, 0, sizeof segs);
    segs[0].segment_id = 234881064; segs[0].flags = 2; segs[0].way_first = segs[0].way_last = 1;
    segs[0].start_time = 1500000000.5; segs[0].end_time = 1500000030.0; segs[0].length = 500; segs[0].end_shape_index = 5;
    segs[1] = segs[0];
    segs[1].segment_id = 268435496; segs[1].start_time = 1500000030.0; segs[1].end_time = -1; segs[1].length = -1;
    ReportRec rep;
    std::memset(&rep, 0, sizeof rep);
    rep.id = 234881064; rep.next_id = 268435496; rep.t0 = 1500000000.5; rep.t1 = 1500000030.0; rep.length = 500;
    ReportStats st;
    std::memset(&st, 0, sizeof st);
    st.successful_count = 1; st.successful_length_m = 500; st.unreported_length_m = -1; st.shape_used = -1; st.n_reports = 1;
    std::string want = head_want(st) + segment_want(segs[0], true) + segment_want(segs[1], false) +
                       "],\"mode\":\"auto\"},\"datastore\":{\"mode\":\"auto\",\"reports\":[" + report_want(rep, true) + "]}}";
    std::string got;
    for (uint32_t j = 0; j < 2 + 1 + 3; ++j) {
      RtCount c;
      rt_item(c, j, segs, 2, &rep, 1, st);
      std::string part(c.n, '?');
      RtWrite w{&part[0]};
      rt_item(w, j, segs, 2, &rep, 1, st);
      CHECK((size_t)(w.p - part.data()) == part.size());
      got += part;
    }
    CHECK(got == want);
    CHECK(got.find("\"length\":0.500}") != std::string::npos && got.find("\"shape_used\"") == std::string::npos);
  }
  if (g_fail) return 1;
  std::printf("reply text ok (%" PRIu64 " times, %" PRIu64 " pieces)\n", g_times, pieces);
  return 0;
}
