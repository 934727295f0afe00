// Host test of edges_json.hpp: the polyline encoder against the published vector and a decoder
// written here, and the edge-entry formatter with every optional key absent and present.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "edges_json.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

static void check_eq(const std::string& got, const std::string& want, int line) {
  if (got != want) {
    std::printf("FAILED line %d:\n got  %s\n want %s\n", line, got.c_str(), want.c_str());
    ++g_fail;
  }
}
#define CHECK_EQ(a, b) check_eq((a), (b), __LINE__)

// the inverse, written for this test: (lat, lon) integers at the encoder's factor
static bool decode(const std::string& s, std::vector<long long>& out) {
  out.clear();
  long long prev[2] = {0, 0};
  size_t i = 0;
  int which = 0;
  while (i < s.size()) {
    unsigned long long u = 0;
    int shift = 0;
    for (;;) {
      if (i == s.size()) return false;   // a value cut short
      const int c = (unsigned char)s[i++] - 63;
      if (c < 0 || c > 63) return false;
      u |= (unsigned long long)(c & 0x1f) << shift;
      shift += 5;
      if (c < 0x20) break;
    }
    const long long d = (u & 1ull) ? ~(long long)(u >> 1) : (long long)(u >> 1);
    prev[which] += d;
    out.push_back(prev[which]);
    which ^= 1;
  }
  return which == 0;
}

static MatchedEdge visit() {
  MatchedEdge r{};
  r.edge = 7; r.way = 4242; r.b_cm = 2500; r.e_cm = 10000; r.t_enter = 100.0; r.t_exit = 3700.0;
  r.begin_point = 3; r.end_point = 5; r.shape_begin = 9; r.shape_end = 12;
  r.seg_dense = kNone; r.seg_off_cm = 0; r.flags = 0; r.len_cm = 10000;
  return r;
}

int main() {
  // the published example: (38.5, -120.2), (40.7, -120.95), (43.252, -126.453) at precision 5
  {
    const float pts[] = {-120.2f, 38.5f, -120.95f, 40.7f, -126.453f, 43.252f};   // (lon, lat) pairs
    std::string enc;
    tj::polyline_encode(pts, 3, 1e5, enc);
    CHECK_EQ(enc, "_p~iF~ps|U_ulLnnqC_mqNvxq`@");
    std::vector<long long> v;
    CHECK(decode(enc, v));
    CHECK((v == std::vector<long long>{3850000, -12020000, 4070000, -12095000, 4325200, -12645300}));
  }
  // an empty shape, single values, zero and negative differences
  {
    std::string enc;
    tj::polyline_encode(nullptr, 0, 1e6, enc);
    CHECK_EQ(enc, "");
    std::string z;
    tj::polyline_put(z, 0);
    CHECK_EQ(z, "?");
    z.clear();
    tj::polyline_put(z, -1);
    CHECK_EQ(z, "@");
    z.clear();
    tj::polyline_put(z, 16);      // zig-zag 32: the first value of two groups
    CHECK_EQ(z, "_@");
    const float pts[] = {8.5f, 47.25f, 8.5f, 47.25f, 8.25f, 47.25f, 8.25f, 47.0f, -0.5f, -0.25f, 0.0f, 0.0f};
    tj::polyline_encode(pts, 6, 1e6, enc);
    std::vector<long long> v;
    CHECK(decode(enc, v));
    CHECK((v == std::vector<long long>{47250000, 8500000, 47250000, 8500000, 47250000, 8250000, 47000000, 8250000,
                                       -250000, -500000, 0, 0}));
    std::string one, two;
    tj::polyline_encode(pts, 1, 1e6, one);
    tj::polyline_encode(pts, 2, 1e6, two);
    CHECK_EQ(two, one + "??");   // the repeated vertex: two zero differences
  }
  // round trip at 1e6 over generated vertices (a fixed LCG), llround((double)v * 1e6) of each float
  {
    std::vector<float> pts;
    unsigned long long s = 12345;
    for (int i = 0; i < 4000; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const double u = (double)(s >> 11) / 9007199254740992.0;
      const bool lat = (i & 1) != 0;
      // long jumps, short steps, and repeats of the vertex before
      float x = (float)((u - 0.5) * (lat ? 180.0 : 360.0));
      if (i >= 2 && (i / 2) % 3 == 1) x = pts[i - 2] + (float)((u - 0.5) * 1e-3);
      if (i >= 2 && (i / 2) % 7 == 3) x = pts[i - 2];
      pts.push_back(x);
    }
    std::string enc;
    tj::polyline_encode(pts.data(), pts.size() / 2, 1e6, enc);
    std::vector<long long> v;
    CHECK(decode(enc, v));
    CHECK(v.size() == pts.size());
    for (size_t i = 0; i + 1 < pts.size() && i + 1 < v.size(); i += 2) {
      CHECK(v[i] == std::llround((double)pts[i + 1] * 1e6));
      CHECK(v[i + 1] == std::llround((double)pts[i] * 1e6));
    }
    for (const char c : enc) CHECK(c >= 63 && c <= 126);
  }
  // a polyline in a JSON string: only the backslash needs an escape
  {
    std::string o;
    tj::put_polyline_string(o, "a\\b?`~");
    CHECK_EQ(o, "\"a\\\\b?`~\"");
  }
  // an entry with every optional key absent ...
  {
    MatchedEdge r = visit();
    r.t_exit = r.t_enter;   // no time passed: no speed
    std::string o;
    tj::format_matched_edge(r, 0, true, o);
    CHECK_EQ(o, "{\"edge_id\":7,\"way_id\":4242,\"begin_shape_index\":9,\"end_shape_index\":12,\"begin_trace_index\":3,"
                "\"end_trace_index\":5,\"length\":0.075,\"start_time\":100,\"end_time\":100,"
                "\"source_percent_along\":0.25,\"target_percent_along\":1}");
    // a chain's first visit that is also the trace's first is no discontinuity
    r.flags = kEdgeChainFirst;
    std::string o2;
    tj::format_matched_edge(r, 0, true, o2);
    CHECK_EQ(o2, o);
  }
  // ... and present: 0.075 km in one hour
  {
    MatchedEdge r = visit();
    r.seg_dense = 2; r.seg_off_cm = 500;
    r.flags = kEdgeInternal | kEdgeHasSegment | kEdgeChainFirst;
    std::string o;
    tj::format_matched_edge(r, 123456789012345ull, false, o);
    CHECK_EQ(o, "{\"edge_id\":7,\"way_id\":4242,\"segment_id\":123456789012345,\"begin_shape_index\":9,"
                "\"end_shape_index\":12,\"begin_trace_index\":3,\"end_trace_index\":5,\"length\":0.075,\"speed\":0.075,"
                "\"start_time\":100,\"end_time\":3700,\"source_percent_along\":0.25,\"target_percent_along\":1,"
                "\"internal\":true,\"discontinuity\":true}");
  }
  // the whole reply: segments kept, edges and shape appended; no visits gives empty lists
  {
    std::string js = "{\"segments\":[]}";
    tj::append_matched_edges(nullptr, 0, nullptr, 0, [](uint32_t) { return 0ull; }, js);
    CHECK_EQ(js, "{\"segments\":[],\"edges\":[],\"shape\":\"\"}");
    MatchedEdge two[2] = {visit(), visit()};
    two[0].flags = kEdgeChainFirst;
    two[1].flags = kEdgeChainFirst | kEdgeHasSegment;
    two[1].seg_dense = 1;
    const float pts[] = {-120.2f, 38.5f, -120.95f, 40.7f};
    js = "{\"segments\":[{\"x\":1}]}";
    tj::append_matched_edges(two, 2, pts, 2, [](uint32_t sd) { return 1000ull + sd; }, js);
    CHECK(js.rfind("{\"segments\":[{\"x\":1}],\"edges\":[{\"edge_id\":7,", 0) == 0);
    CHECK(js.find("\"segment_id\":1001") != std::string::npos);
    size_t n_disc = 0;
    for (size_t at = js.find("\"discontinuity\":true"); at != std::string::npos; at = js.find("\"discontinuity\":true", at + 1)) ++n_disc;
    CHECK(n_disc == 1);   // the second chain's first visit only
    std::string enc;
    tj::polyline_encode(pts, 2, 1e6, enc);
    std::string tail = "],\"shape\":";
    tj::put_polyline_string(tail, enc);
    tail += '}';
    CHECK(js.size() > tail.size() && js.compare(js.size() - tail.size(), tail.size(), tail) == 0);
  }
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("edges json ok\n");
  return 0;
}
