// points.hip — matched points (DESIGN.md §3 rule 9): the snapped road position of every input
// point of the last run, states and the points the interpolation rule dropped alike.
//
// k_matched_points works over state slots, one 16-lane group per slot (four slots per wave, as
// the group search tiers): the group writes the record of its own state (type 1) and then walks
// the gap of non-state points behind it in time order (type 2), carrying the lower bound xmin so
// that snapped positions never run backwards on the route.  The gap's polyline is the chosen path
// of the transition into the next state, clipped at both candidates, or the rest of the state's
// own edge when the chain ends there.  A lane takes whole pieces (path edges) of a polyline of
// several and walks their shape segments; the segments of a polyline of one piece (a stopped
// vehicle's gap of a hundred points lies on one edge) are dealt out over the lanes.  Every
// candidate position is keyed `sq bits << 32 | route cm`; the keys are min-reduced across the
// group with __shfl_xor (no LDS, no atomics) and the lane that owns the minimum writes the record
// as two 16-byte stores.
//
// The stage runs only on request (Matcher::matched_points) over what the last run left in HBM:
// nothing here is launched by run() / run_small() / rerun().
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace rm {

namespace {

constexpr int kPtW = 16;          // lanes per state slot
constexpr int kPtThreads = 256;   // 16 slots per block
constexpr uint32_t kPtUnmatched = 0u, kPtMatched = 1u, kPtInterpolated = 2u;

struct PointsArgs {
  uint32_t T;
  uint64_t P;
  const uint32_t* trace_off; const float* lon; const float* lat;
  const MatchOptions* opts; const uint32_t* trace_opt;
  const uint32_t* slot_trace; const uint32_t* n_states; const uint32_t* state_orig;
  const uint4* cand_desc; const int8_t* choice; const uint8_t* chain_start;
  const uint32_t* path_off; const uint32_t* path_cnt; const uint32_t* path_inline; const uint32_t* path_pool;
  const uint2* path_sab;
  const uint32_t* trace_err;
  const uint32_t* road_vert_off;   // per road: its first shape vertex (R + 1)
  uint4* out;                      // two per point: {lon, lat, sq, edge}, {off_cm, way, type, route_cm}
};

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int d) {
  return ((unsigned long long)(uint32_t)__shfl_xor((int)(v >> 32), d, kPtW) << 32) |
         (uint32_t)__shfl_xor((int)(uint32_t)v, d, kPtW);
}

__device__ __forceinline__ void store_point(const PointsArgs& a, uint64_t pt, float lon, float lat, float sq, uint32_t edge,
                                            uint32_t off_cm, uint32_t way, uint32_t type, uint32_t route_cm) {
  a.out[2 * pt] = make_uint4(__float_as_uint(lon), __float_as_uint(lat), __float_as_uint(sq), edge);
  a.out[2 * pt + 1] = make_uint4(off_cm, way, type, route_cm);
}

// rule 9 road_point from shape segment i, which holds s (cum_i <= s <= cum_{i+1}): the first
// segment of the road with s <= cum[i+1] is i itself unless s lies on its first vertex
__device__ __forceinline__ void road_point_from(const DevGraph& g, uint32_t va, uint32_t i, uint4 A, uint4 B, uint32_t s,
                                                float& lon, float& lat) {
  while (i > va && s <= A.z) {
    --i;
    B = A;
    A = g.verts[i];
  }
  const uint32_t d = B.z - A.z;
  float t = 0.0f;
  if (d > 0u) t = (float)(s - A.z) / (float)d;
  const float alon = __uint_as_float(A.x), alat = __uint_as_float(A.y);
  lon = alon + t * (__uint_as_float(B.x) - alon);
  lat = alat + t * (__uint_as_float(B.y) - alat);
}

// sq_to of rule 9: the squared distance in the measurement's local frame (K1's, rule 2)
__device__ __forceinline__ float sq_to(float plon, float plat, float mlon, float mlat, float qlon, float qlat) {
  const float dx = (qlon - plon) * mlon, dy = (qlat - plat) * mlat;
  return dx * dx + dy * dy;
}

struct Piece {      // one path edge of the polyline, clipped to [c0, c1] in edge coordinates
  uint32_t e, va, vb;   // directed edge, first and last shape vertex of its road
  uint32_t L, rev, c0, c1;
  uint32_t x0;          // route coordinate of c0
};

struct Best {
  unsigned long long key, tag;   // sq bits << 32 | route cm; piece << 32 | shape segment
  float lon, lat;
  uint32_t e, c;
};

__device__ __forceinline__ Piece make_piece(const DevGraph& g, const PointsArgs& a, uint32_t e, bool first, bool last,
                                            uint32_t sa, uint32_t sb) {
  Piece pc;
  const uint4 er = g.edges[e];
  const uint32_t road = er.w >> 1;
  pc.e = e;
  pc.L = er.y;
  pc.rev = er.w & 1u;
  pc.va = a.road_vert_off[road];
  pc.vb = a.road_vert_off[road + 1] - 1u;
  pc.c0 = first ? (pc.rev ? pc.L - sa : sa) : 0u;
  pc.c1 = last ? (pc.rev ? pc.L - sb : sb) : pc.L;
  pc.x0 = 0u;
  return pc;
}

// candidates of one piece from route coordinate xmin on: shape segments i0, i0 + step, ...
__device__ __forceinline__ void scan_piece(const DevGraph& g, const Piece& pc, uint32_t piece, uint32_t xmin, float plon,
                                           float plat, float mlon, float mlat, uint32_t i0, uint32_t step, Best& b) {
  if (pc.x0 + (pc.c1 - pc.c0) < xmin) return;   // wholly behind the previous point
  const uint32_t clo = xmin > pc.x0 ? pc.c0 + (xmin - pc.x0) : pc.c0;
  const uint32_t slo = pc.rev ? pc.L - pc.c1 : clo, shi = pc.rev ? pc.L - clo : pc.c1;
  for (uint32_t i = i0; i < pc.vb; i += step) {
    const uint4 A = g.verts[i], B = g.verts[i + 1];
    if (B.z < slo || A.z > shi) continue;
    // K1's projection (rule 2): clamped t, s = rint(along) clamped to the segment
    const float ax = (__uint_as_float(A.x) - plon) * mlon, ay = (__uint_as_float(A.y) - plat) * mlat;
    const float bx = (__uint_as_float(B.x) - plon) * mlon, by = (__uint_as_float(B.y) - plat) * mlat;
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    float t = 0.0f;
    if (l2 > 0.0f) {
      t = -(ax * dx + ay * dy) / l2;
      if (t < 0.0f) t = 0.0f;
      if (t > 1.0f) t = 1.0f;
    }
    const float along = (float)A.z + t * (float)(B.z - A.z);
    uint32_t s = (uint32_t)rintf(along);
    if (s < A.z) s = A.z;
    if (s > B.z) s = B.z;
    if (s < slo) s = slo;
    if (s > shi) s = shi;
    float qlon, qlat;
    road_point_from(g, pc.va, i, A, B, s, qlon, qlat);
    const float sq = sq_to(plon, plat, mlon, mlat, qlon, qlat);
    const uint32_t c = pc.rev ? pc.L - s : s;
    const unsigned long long key = ((unsigned long long)__float_as_uint(sq) << 32) | (pc.x0 + (c - pc.c0));
    const unsigned long long tag = ((unsigned long long)piece << 32) | i;
    if (key < b.key || (key == b.key && tag < b.tag)) {
      b.key = key; b.tag = tag; b.lon = qlon; b.lat = qlat; b.e = pc.e; b.c = c;
    }
  }
}

// the pieces q0 + lane of a transition's path (edges pe[0 .. ns)), a lane each, with their route
// coordinates: xbase is the route coordinate at piece q0 and moves on to piece q0 + 16
__device__ __forceinline__ Piece load_pieces(const DevGraph& g, const PointsArgs& a, const uint32_t* pe, uint32_t ns,
                                             uint32_t q0, int lane, uint32_t sa, uint32_t sb, uint32_t& xbase, bool& valid) {
  const uint32_t q = q0 + (uint32_t)lane;
  valid = q < ns;
  Piece pc{};
  if (valid) pc = make_piece(g, a, pe[q], q == 0u, q + 1u == ns, sa, sb);
  const uint32_t ln = pc.c1 - pc.c0;
  uint32_t incl = ln;
#pragma unroll
  for (int d = 1; d < kPtW; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, kPtW);
    if (lane >= d) incl += o;
  }
  pc.x0 = xbase + incl - ln;
  xbase += (uint32_t)__shfl((int)incl, kPtW - 1, kPtW);
  return pc;
}

__global__ void __launch_bounds__(kPtThreads) k_matched_points(DevGraph g, PointsArgs a) {
  const uint64_t p = ((uint64_t)blockIdx.x * kPtThreads + threadIdx.x) / kPtW;   // state slot of the group
  const int lane = threadIdx.x & (kPtW - 1);
  if (p >= a.P) return;
  const uint32_t k = a.slot_trace[p];
  const uint32_t o = a.trace_off[k], n = a.trace_off[k + 1] - o, S = a.n_states[k];
  const uint32_t s = (uint32_t)(p - o);
  if (s >= S) return;                                   // no state at this slot
  const uint32_t q0 = a.state_orig[p];
  const uint32_t q1 = s + 1u < S ? a.state_orig[p + 1] : n;
  const int ch = a.choice[p];
  if (a.trace_err[k] != 0u || ch < 0) {                 // unmatched: the state and its followers
    for (uint32_t q = q0 + (uint32_t)lane; q < q1; q += kPtW) store_point(a, (uint64_t)o + q, 0.f, 0.f, 0.f, kNone, 0u, 0u, kPtUnmatched, 0u);
    return;
  }
  const uint4 cd = a.cand_desc[(p * kMaxCand + (uint32_t)ch) * 2];   // {road, s, L, speeds}
  const uint32_t road = cd.x, sa = cd.y, L = cd.z;
  // a slot continues a chain when it holds the path of the transition into it
  const auto path_of = [&](uint64_t l, uint32_t& ns) -> const uint32_t* {
    ns = a.path_cnt[l];
    if (ns <= (uint32_t)kInlinePath) return a.path_inline + l * kInlinePath;
    const uint32_t at = a.path_off[l];
    if (at == kNone) ns = 0u;
    return a.path_pool + at;
  };
  uint32_t ns_p = 0u, ns_n = 0u;
  const uint32_t* pe_p = nullptr;
  const uint32_t* pe_n = nullptr;
  if (s >= 1u && !a.chain_start[p]) pe_p = path_of(p, ns_p);
  if (s + 1u < S && !a.chain_start[p + 1] && a.choice[p + 1] >= 0) pe_n = path_of(p + 1, ns_n);
  uint32_t e_a;
  if (ns_p) {
    e_a = pe_p[ns_p - 1u];
  } else if (ns_n) {
    e_a = pe_n[0];
  } else {
    const uint4 r0 = g.road_rec[2 * (uint64_t)road], r1 = g.road_rec[2 * (uint64_t)road + 1];   // {.., fwd}, {rev, info fwd, ..}
    const uint32_t acc = mode_access(a.opts[a.trace_opt[k]].mode);
    e_a = (r0.w != kNone && (edge_access(r1.y) & acc) != 0u) ? r0.w : r1.x;
  }
  if (e_a == kNone) {   // (K1 keeps only roads with an edge the mode can use: not reached)
    for (uint32_t q = q0 + (uint32_t)lane; q < q1; q += kPtW) store_point(a, (uint64_t)o + q, 0.f, 0.f, 0.f, kNone, 0u, 0u, kPtUnmatched, 0u);
    return;
  }
  const uint32_t rev_a = g.edges[e_a].w & 1u;
  const uint32_t off_a = rev_a ? L - sa : sa;
  const uint32_t va = a.road_vert_off[road], vb = a.road_vert_off[road + 1] - 1u;
  const float mlat = (float)kMetersPerDegLat;
  {
    // type 1: road_point(road, sa) -- the first shape segment with sa <= cum[i+1], or the last
    uint32_t fi = vb - 1u;
    for (uint32_t i0 = va; i0 < vb; i0 += kPtW) {
      const uint32_t i = i0 + (uint32_t)lane;
      uint32_t hit = (i < vb && sa <= g.verts[i + 1].z) ? i : kNone;
#pragma unroll
      for (int d = 1; d < kPtW; d <<= 1) hit = min(hit, (uint32_t)__shfl_xor((int)hit, d, kPtW));
      if (hit != kNone) { fi = hit; break; }
    }
    if (lane == 0) {
      const uint4 A = g.verts[fi], B = g.verts[fi + 1];
      const uint32_t d = B.z - A.z;
      float t = 0.0f;
      if (d > 0u) t = (float)(sa - A.z) / (float)d;
      const float alon = __uint_as_float(A.x), alat = __uint_as_float(A.y);
      const float qlon = alon + t * (__uint_as_float(B.x) - alon), qlat = alat + t * (__uint_as_float(B.y) - alat);
      const uint64_t pt = (uint64_t)o + q0;
      const float plon = a.lon[pt], plat = a.lat[pt];
      store_point(a, pt, qlon, qlat, sq_to(plon, plat, meters_per_lon(plat), mlat, qlon, qlat), e_a, off_a, g.edge_way[e_a],
                  kPtMatched, 0u);
    }
  }
  if (q0 + 1u >= q1) return;
  // type 2: the gap's polyline
  const bool single = ns_n <= 1u;      // one piece: its shape segments are dealt out over the lanes
  Piece pc{};
  bool valid = true;
  uint32_t sb = 0u;
  if (ns_n) sb = a.path_sab[p + 1].y;
  if (!ns_n) {
    pc.e = e_a; pc.va = va; pc.vb = vb; pc.L = L; pc.rev = rev_a; pc.c0 = off_a; pc.c1 = L; pc.x0 = 0u;
  } else if (single) {
    pc = make_piece(g, a, pe_n[0], true, true, sa, sb);
  } else {
    uint32_t xb = 0u;
    pc = load_pieces(g, a, pe_n, ns_n, 0u, lane, sa, sb, xb, valid);   // pieces 0..15 stay in registers
  }
  uint32_t xmin = 0u;
  for (uint32_t q = q0 + 1u; q < q1; ++q) {
    const uint64_t pt = (uint64_t)o + q;
    const float plon = a.lon[pt], plat = a.lat[pt];
    const float mlon = meters_per_lon(plat);
    Best b;
    b.key = ~0ull; b.tag = ~0ull; b.lon = 0.f; b.lat = 0.f; b.e = kNone; b.c = 0u;
    if (single) {
      scan_piece(g, pc, 0u, xmin, plon, plat, mlon, mlat, pc.va + (uint32_t)lane, kPtW, b);
    } else {
      if (valid) scan_piece(g, pc, (uint32_t)lane, xmin, plon, plat, mlon, mlat, pc.va, 1u, b);
      uint32_t xb = pc.x0 + (pc.c1 - pc.c0);
      xb = (uint32_t)__shfl((int)xb, kPtW - 1, kPtW);    // route coordinate behind piece 15
      for (uint32_t c0 = kPtW; c0 < ns_n; c0 += kPtW) {
        bool v2;
        const Piece p2 = load_pieces(g, a, pe_n, ns_n, c0, lane, sa, sb, xb, v2);
        if (v2) scan_piece(g, p2, c0 + (uint32_t)lane, xmin, plon, plat, mlon, mlat, p2.va, 1u, b);
      }
    }
    unsigned long long wk = b.key, wt = b.tag;
#pragma unroll
    for (int d = 1; d < kPtW; d <<= 1) {
      const unsigned long long ok = shfl_xor_u64(wk, d), ot = shfl_xor_u64(wt, d);
      if (ok < wk || (ok == wk && ot < wt)) { wk = ok; wt = ot; }
    }
    if (wk == ~0ull) {   // (a piece always remains eligible: not reached on a valid graph)
      if (lane == 0) store_point(a, pt, 0.f, 0.f, 0.f, kNone, 0u, 0u, kPtUnmatched, 0u);
      continue;
    }
    xmin = (uint32_t)wk;
    if (b.key == wk && b.tag == wt)   // the one lane that owns the minimum
      store_point(a, pt, b.lon, b.lat, __uint_as_float((uint32_t)(wk >> 32)), b.e, b.c, g.edge_way[b.e], kPtInterpolated, xmin);
  }
}

}  // namespace

const uint32_t* Engine::road_vert_off_dev() {
  std::lock_guard<std::mutex> lk(ball_mu_);
  if (!road_vert_off_) {
    RM_HIP(hipSetDevice(device_));
    const std::vector<uint32_t>& v = host_.road_vert_off;
    road_vert_off_.reserve(v.size());
    RM_HIP(hipMemcpy(road_vert_off_, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return road_vert_off_;
}

void Matcher::matched_points(MatchedPoint* out) {
  RM_HIP(hipSetDevice(eng_->device()));
  sync();
  const uint64_t P = n_points_;
  if (!n_traces_ || !P) return;
  const uint32_t* rvo = eng_->road_vert_off_dev();
  if (P > mp_dev_.cap()) {   // grow-only, by half again (a service's batch sizes creep upwards)
    const uint64_t c = std::max<uint64_t>(P + P / 2, 4096);
    mp_dev_.reserve(c, ("matched-point buffer of " + std::to_string(c * sizeof(MatchedPoint)) + " bytes does not fit in HBM").c_str());
  }
  const Workspace& w = ws_;
  PointsArgs a;
  a.T = n_traces_; a.P = P;
  a.trace_off = in_.trace_off; a.lon = in_.lon; a.lat = in_.lat; a.opts = in_.opts; a.trace_opt = in_.trace_opt;
  a.slot_trace = w.slot_trace; a.n_states = w.n_states; a.state_orig = w.state_orig;
  a.cand_desc = w.cand_desc; a.choice = w.choice; a.chain_start = w.chain_start;
  a.path_off = w.path_off; a.path_cnt = w.path_cnt; a.path_inline = w.path_inline; a.path_pool = w.path_pool;
  a.path_sab = w.path_sab;
  a.trace_err = w.trace_err;
  a.road_vert_off = rvo;
  a.out = (uint4*)mp_dev_.get();
  const uint32_t grid = (uint32_t)((P * kPtW + kPtThreads - 1) / kPtThreads);
  tic(kKPoints);
  hipLaunchKernelGGL(k_matched_points, dim3(grid), dim3(kPtThreads), 0, stream_, eng_->dev_snapshot(), a);
  toc(kKPoints);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(out, mp_dev_, P * sizeof(MatchedPoint), hipMemcpyDeviceToHost, stream_));
  sync();
}

}  // namespace rm
