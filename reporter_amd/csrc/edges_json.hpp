// edges_json.hpp — the reply side of rm_match_edges (DESIGN.md §3 rule 10): the encoded polyline
// and the per-edge entries Valhalla's trace_attributes gives ("edges", "shape").  Host only, no
// HIP: tests/cpp/edges_json_test.cpp compiles it alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "rm_common.hpp"
#include "trace_json.hpp"

namespace rm {
namespace tj {

// one signed value of an encoded polyline: zig-zag, then 5-bit groups, low group first, + 63
inline void polyline_put(std::string& o, int64_t d) {
  uint64_t u = d < 0 ? ~((uint64_t)d << 1) : (uint64_t)d << 1;
  while (u >= 0x20u) {
    o += (char)((0x20u | (u & 0x1fu)) + 63u);
    u >>= 5;
  }
  o += (char)(u + 63u);
}

// The encoded polyline of n (lon, lat) pairs: per vertex lat then lon, each llround(v * factor)
// (1e5: the published format, 1e6: Valhalla's shapes), as the difference to the vertex before.
inline void polyline_encode(const float* lonlat, size_t n, double factor, std::string& o) {
  int64_t plat = 0, plon = 0;
  for (size_t i = 0; i < n; ++i) {
    const int64_t lat = std::llround((double)lonlat[2 * i + 1] * factor);
    const int64_t lon = std::llround((double)lonlat[2 * i] * factor);
    polyline_put(o, lat - plat);
    polyline_put(o, lon - plon);
    plat = lat;
    plon = lon;
  }
}

// a polyline as a JSON string: its alphabet (63..126) holds the backslash and no quote
inline void put_polyline_string(std::string& o, const std::string& enc) {
  o += '"';
  for (const char c : enc) {
    if (c == '\\') o += '\\';
    o += c;
  }
  o += '"';
}

// One entry of "edges".  segment_id: the OSMLR id of r.seg_dense (read only when the edge has
// one); trace_first: the visit is its trace's first (a later chain-first visit is a discontinuity)
inline void format_matched_edge(const MatchedEdge& r, uint64_t segment_id, bool trace_first, std::string& o) {
  const double km = (double)(r.e_cm - r.b_cm) / 1e5;
  o += "{\"edge_id\":"; put_u64(o, r.edge);
  o += ",\"way_id\":"; put_u64(o, r.way);
  if (r.flags & kEdgeHasSegment) { o += ",\"segment_id\":"; put_u64(o, segment_id); }
  o += ",\"begin_shape_index\":"; put_u64(o, r.shape_begin);
  o += ",\"end_shape_index\":"; put_u64(o, r.shape_end);
  o += ",\"begin_trace_index\":"; put_u64(o, r.begin_point);
  o += ",\"end_trace_index\":"; put_u64(o, r.end_point);
  o += ",\"length\":"; put_num(o, km);
  if (r.t_exit > r.t_enter) { o += ",\"speed\":"; put_num(o, km / ((r.t_exit - r.t_enter) / 3600.0)); }
  o += ",\"start_time\":"; put_num(o, r.t_enter);
  o += ",\"end_time\":"; put_num(o, r.t_exit);
  o += ",\"source_percent_along\":"; put_num(o, r.len_cm ? (double)r.b_cm / (double)r.len_cm : 0.0);
  o += ",\"target_percent_along\":"; put_num(o, r.len_cm ? (double)r.e_cm / (double)r.len_cm : 0.0);
  if (r.flags & kEdgeInternal) o += ",\"internal\":true";
  if ((r.flags & kEdgeChainFirst) && !trace_first) o += ",\"discontinuity\":true";
  o += '}';
}

// Extends a {"segments":[...]} reply to {"segments":[...],"edges":[...],"shape":"..."}: the n
// visits of one trace and its nv shape vertices ((lon, lat) pairs), the shape at precision 6.
// seg_id(dense) gives a dense segment's OSMLR id.
template <class SegId>
inline void append_matched_edges(const MatchedEdge* ed, uint32_t n, const float* shape, uint32_t nv, SegId&& seg_id,
                                 std::string& o) {
  o.pop_back();   // the closing brace of {"segments":[...]}
  o.reserve(o.size() + 32 + (size_t)n * 320 + (size_t)nv * 8);
  o += ",\"edges\":[";
  for (uint32_t k = 0; k < n; ++k) {
    if (k) o += ',';
    format_matched_edge(ed[k], (ed[k].flags & kEdgeHasSegment) ? (uint64_t)seg_id(ed[k].seg_dense) : 0ull, k == 0, o);
  }
  o += "],\"shape\":";
  std::string enc;
  enc.reserve((size_t)nv * 8);
  polyline_encode(shape, nv, 1e6, enc);
  put_polyline_string(o, enc);
  o += '}';
}

}  // namespace tj
}  // namespace rm
