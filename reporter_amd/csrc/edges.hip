// edges.hip — matched edges (DESIGN.md §3 rule 10): every directed edge a matched chain drove,
// with its entry and exit times, and the trace's matched polyline.
//
// K4 builds one traversal record per path edge in registers and keeps only the OSMLR runs it
// folds them into.  This stage builds the same records again (the same slots, the same wave scan
// for the distance into the transition's route, the same fp64 time interpolation) and keeps what
// the oracle's add_trav keeps: one visit per run of records on one edge that join end to begin.
//
//   k_edge_visits   one wave per trace, 64 traversal records per window, one per lane.  Ballots
//                   give the kept records, the chain breaks and the records that open a visit;
//                   the lane that closes a visit writes its 64-byte record at the trace's first
//                   record + the visit's index and counts the shape vertices the visit adds (two
//                   binary searches over its road's cum); a wave scan with a running carry turns
//                   the counts into shape_begin / shape_end.  The visit still open at a window's
//                   end is carried in wave-uniform registers.  Per trace: visits, vertices.
//   k_edge_scan     exclusive scan of the two per-trace counts (edge_off, shape_off; T + 1 each)
//   k_edge_fill     one lane per visit (its trace by binary search over edge_off; a visit
//                   adds 1.25 vertices on average, too few to share among lanes): the staged
//                   record goes to its compacted place and its vertices (road_point of either
//                   end, the road's stored vertices between them in travel order) into the
//                   trace's shape
//
// Every output position comes from a scan: no atomics, the same bytes on every call.  The stage
// runs only on request (Matcher::matched_edges) over what the last run left in HBM: nothing here
// is launched by run() / run_small() / rerun(), and no kernel id is added (its device time is
// measured by its own events, Matcher::matched_edges_ms).
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "wave_util.hpp"

namespace rm {

namespace {

constexpr int kFillThreads = 256;
constexpr int kScanThreads = 1024;

struct EdgeArgs {
  uint32_t T, total;               // traces; traversal records of the run
  uint64_t P, visits;              // points; visits of the batch (k_edge_fill)
  const uint32_t* trace_off; const uint32_t* state_orig; const double* state_time;
  const uint32_t* path_off; const uint32_t* path_cnt; const uint32_t* path_inline; const uint32_t* path_pool;
  const uint2* path_sab; const uint32_t* route_dist; const uint32_t* trav_off; const uint32_t* rec_slot;
  const uint32_t* trace_err;
  const uint32_t* road_vert_off;   // per road: its first shape vertex (R + 1)
  uint4* stage;                    // four per traversal record: the visits of trace k from its first record on
  uint32_t* cnt;                   // per trace: visits [0, T), shape vertices [T, 2T)
  uint32_t* off;                   // edge_off [0, T], shape_off [T + 1, 2T + 1]
  unsigned long long* tot;         // visits, shape vertices
  uint4* edges; float2* shape;     // the compacted records and the shapes
};

// the road's stored vertices strictly inside (lo, hi): the first one and how many
__device__ __forceinline__ uint32_t interior(const DevGraph& g, uint32_t va, uint32_t vb, uint32_t lo, uint32_t hi,
                                             uint32_t& first) {
  uint32_t a = va, b = vb + 1u;          // first vertex with cum > lo
  while (a < b) {
    const uint32_t m = a + (b - a) / 2u;
    if (g.verts[m].z > lo) b = m; else a = m + 1u;
  }
  first = a;
  uint32_t c = a, d = vb + 1u;           // first vertex with cum >= hi
  while (c < d) {
    const uint32_t m = c + (d - c) / 2u;
    if (g.verts[m].z >= hi) d = m; else c = m + 1u;
  }
  return c > a ? c - a : 0u;
}

// shape vertices a visit adds: the interior vertices of [b_cm, e_cm] and its end, and its begin
// when it opens a chain
__device__ __forceinline__ uint32_t visit_verts(const DevGraph& g, const EdgeArgs& a, uint32_t e, uint32_t b_cm,
                                                uint32_t e_cm, bool first) {
  const uint4 er = g.edges[e];
  const uint32_t road = er.w >> 1, L = er.y;
  const bool rev = (er.w & 1u) != 0u;
  const uint32_t s_b = rev ? L - b_cm : b_cm, s_e = rev ? L - e_cm : e_cm;
  uint32_t f;
  return interior(g, a.road_vert_off[road], a.road_vert_off[road + 1] - 1u, min(s_b, s_e), max(s_b, s_e), f) +
         (first ? 2u : 1u);
}

__device__ __forceinline__ void store_visit(const DevGraph& g, uint4* at, uint32_t e, uint32_t b_cm, uint32_t e_cm,
                                            double t_enter, double t_exit, uint32_t p_b, uint32_t p_e, uint32_t sh_b,
                                            uint32_t sh_e, bool first) {
  const uint4 sr = g.seg_rec[e];   // {len_cm | reversed << 31 | internal << 30, segment, offset, way}
  const unsigned long long tb = (unsigned long long)__double_as_longlong(t_enter);
  const unsigned long long te = (unsigned long long)__double_as_longlong(t_exit);
  const uint32_t flags = (((sr.x >> 30) & 1u) ? kEdgeInternal : 0u) | (sr.y != kNone ? kEdgeHasSegment : 0u) |
                         (first ? kEdgeChainFirst : 0u);
  at[0] = make_uint4(e, sr.w, b_cm, e_cm);
  at[1] = make_uint4((uint32_t)tb, (uint32_t)(tb >> 32), (uint32_t)te, (uint32_t)(te >> 32));
  at[2] = make_uint4(p_b, p_e, sh_b, sh_e);
  at[3] = make_uint4(sr.y, sr.z, flags, sr.x & 0x3fffffffu);
}

__global__ void __launch_bounds__(64) k_edge_visits(DevGraph g, EdgeArgs a) {
  const uint32_t k = blockIdx.x;
  if (k >= a.T) return;
  const int lane = threadIdx.x;
  const uint32_t o = a.trace_off[k], o1 = a.trace_off[k + 1];
  const uint32_t Rb = o < a.P ? a.trav_off[o] : a.total;
  uint32_t Re = o1 < a.P ? a.trav_off[o1] : a.total;
  if (Re > a.total) Re = a.total;
  if (a.trace_err[k] != 0u || Rb >= Re) {   // a failed trace has no visits
    if (lane == 0) { a.cnt[k] = 0u; a.cnt[a.T + k] = 0u; }
    return;
  }
  uint4* const out = a.stage + 4ull * Rb;
  const uint32_t rl = Re - 1u;
  // carried between windows: the slot of the record before the window and whether the last kept
  // record is chain-continuous up to it; the route distance of the transition that straddles the
  // window start; the visit still open (its begin fields, and its end so far = the last kept record)
  uint32_t c_slot = kNone;
  bool c_has = false;
  unsigned long long carry_x = 0;
  bool v_open = false, v_first = false;
  uint32_t v_e = 0, v_b = 0, v_en = 0, v_pb = 0, v_pe = 0;
  double v_tb = 0.0, v_te = 0.0;
  uint32_t visits = 0, nvert = 0;
  for (uint32_t c0 = Rb; c0 < Re; c0 += 64) {
    const uint32_t n = min(64u, Re - c0);
    const bool last = c0 + n == Re;
    const bool act = (uint32_t)lane < n;
    // ---- one traversal record per lane (rule 6; every load at a clamped record index)
    const uint32_t l = a.rec_slot[min(c0 + (uint32_t)lane, rl)];   // a transition's target slot: l >= 1
    const uint32_t ns = a.path_cnt[l];
    const uint32_t q = min(c0 + (uint32_t)lane, rl) - a.trav_off[l];
    const uint32_t* pe = ns <= (uint32_t)kInlinePath ? a.path_inline + (uint64_t)l * kInlinePath : a.path_pool + a.path_off[l];
    const uint32_t e = pe[q];
    const uint4 sr = g.seg_rec[e];
    const uint2 sab = a.path_sab[l];
    const uint32_t D = a.route_dist[l];
    const double ta = a.state_time[l - 1], tbs = a.state_time[l];
    const uint32_t L = sr.x & 0x3fffffffu;
    const bool rev = (sr.x >> 31) != 0u;
    uint32_t b0 = 0u, b1 = L;
    if (q == 0u) b0 = rev ? L - sab.x : sab.x;
    if (q + 1u == ns) b1 = rev ? L - sab.y : sab.y;
    if (!act) b0 = b1 = 0u;
    const uint32_t p_b = a.state_orig[l - 1];
    const uint32_t p_e = q + 1u == ns ? a.state_orig[l] : p_b;
    const unsigned long long w = (unsigned long long)(b1 - b0);
    const unsigned long long S = wave_incl_sum(w, lane);
    const int st = act ? lane - (int)q : lane;              // lane of the transition's first record
    const unsigned long long S_st = at_lane(S, st - 1);
    unsigned long long xb = S - w - (st > 0 ? S_st : 0ull);
    if (st < 0) xb += carry_x;
    const double tbr = interp_time(ta, tbs, xb, D);
    const double ter = interp_time(ta, tbs, xb + w, D);
    // ---- the previous kept record of the chain; a kept record either extends its visit or opens one
    const bool kept = act && b1 != b0;
    const unsigned long long K = __ballot(kept);
    const uint32_t lp = __shfl_up(l, 1, 64);
    const bool brk = act && (lane == 0 ? !(c_slot != kNone && same_chain(c_slot, l)) : !same_chain(lp, l));
    const unsigned long long BR = __ballot(brk);
    const int j = hi_le(K, lane - 1), pb = hi_le(BR, lane);
    const bool has = j >= 0 ? pb <= j : (pb < 0 && c_has);
    uint32_t u_e = at_lane(e, j), u_en = at_lane(b1, j);
    if (j < 0) { u_e = v_e; u_en = v_en; }
    const bool opens = kept && !(has && u_e == e && u_en == b0);
    const unsigned long long NW = __ballot(opens);
    const unsigned long long FC = __ballot(opens && !has);
    // ---- the visit carried in closes before this window's first kept record when that opens a
    // visit (or, at the trace's end, when the window keeps nothing)
    if (v_open && ((K != 0ull && ((NW >> __builtin_ctzll(K)) & 1ull)) || (K == 0ull && last))) {
      const uint32_t c = visit_verts(g, a, v_e, v_b, v_en, v_first);   // wave-uniform
      if (lane == 0)
        store_visit(g, out + 4ull * (visits - 1u), v_e, v_b, v_en, v_tb, v_te, v_pb, v_pe,
                    v_first ? nvert : nvert - 1u, nvert + c - 1u, v_first);
      nvert += c;
      v_open = false;
    }
    // ---- visits that close in this window: begin fields from the lane that opened them
    const int ps = hi_le(NW, lane);
    const uint32_t h_b = at_lane(b0, ps), h_pb = at_lane(p_b, ps);
    const double h_tb = at_lane(tbr, ps);
    const uint32_t f_b = ps >= 0 ? h_b : v_b, f_pb = ps >= 0 ? h_pb : v_pb;
    const double f_tb = ps >= 0 ? h_tb : v_tb;
    const bool f_first = ps >= 0 ? ((FC >> ps) & 1ull) != 0ull : v_first;
    const int nx = lo_gt(K, lane);
    const bool closes = kept && (nx < 64 ? ((NW >> nx) & 1ull) != 0ull : last);
    uint32_t c = 0u;
    if (closes) c = visit_verts(g, a, e, f_b, b1, f_first);
    const uint32_t C = (uint32_t)wave_incl_sum((unsigned long long)c, lane);
    if (closes) {
      const uint32_t idx = ps >= 0 ? visits + (uint32_t)__popcll(NW & ((2ull << lane) - 1ull)) - 1u : visits - 1u;
      const uint32_t sh_e = nvert + C - 1u;
      store_visit(g, out + 4ull * idx, e, f_b, b1, f_tb, ter, f_pb, p_e, f_first ? sh_e + 1u - c : sh_e - c, sh_e, f_first);
    }
    nvert += __shfl(C, 63, 64);
    visits += (uint32_t)__popcll(NW);
    if (last) break;
    // ---- carry into the next window
    if (K != 0ull) {
      const int jl = 63 - __builtin_clzll(K);           // its visit stays open (nx == 64, not last)
      const uint32_t t_b = __shfl(f_b, jl, 64), t_pb = __shfl(f_pb, jl, 64);
      const double t_tb = __shfl(f_tb, jl, 64);
      const int t_first = __shfl((int)f_first, jl, 64);
      v_b = t_b; v_pb = t_pb; v_tb = t_tb; v_first = t_first != 0;
      v_e = __shfl(e, jl, 64); v_en = __shfl(b1, jl, 64); v_pe = __shfl(p_e, jl, 64);
      v_te = __shfl(ter, jl, 64);
      v_open = true;
      c_has = jl == 63 ? true : (BR >> (jl + 1)) == 0ull;
    } else {
      c_has = c_has && BR == 0ull;
    }
    c_slot = __shfl(l, (int)n - 1, 64);
    carry_x = __shfl(xb + w, (int)n - 1, 64);
  }
  if (lane == 0) { a.cnt[k] = visits; a.cnt[a.T + k] = nvert; }
}

// exclusive scans of the per-trace visit and vertex counts by one block; totals to tot[0..1]
__global__ void __launch_bounds__(kScanThreads) k_edge_scan(EdgeArgs a) {
  __shared__ unsigned long long part[2][kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long base0 = 0, base1 = 0;
  for (uint32_t t0 = 0; t0 < a.T; t0 += kScanThreads) {
    const uint32_t k = t0 + (uint32_t)tid;
    const unsigned long long c0 = k < a.T ? a.cnt[k] : 0u, c1 = k < a.T ? a.cnt[a.T + k] : 0u;
    const unsigned long long s0 = wave_incl_sum(c0, lane), s1 = wave_incl_sum(c1, lane);
    if (lane == 63) { part[0][wv] = s0; part[1][wv] = s1; }
    __syncthreads();
    unsigned long long p0 = 0, p1 = 0, t0s = 0, t1s = 0;
    for (int i = 0; i < kScanThreads / 64; ++i) {
      if (i < wv) { p0 += part[0][i]; p1 += part[1][i]; }
      t0s += part[0][i]; t1s += part[1][i];
    }
    if (k < a.T) {
      a.off[k] = (uint32_t)(base0 + p0 + s0 - c0);
      a.off[a.T + 1 + k] = (uint32_t)(base1 + p1 + s1 - c1);
    }
    base0 += t0s; base1 += t1s;
    __syncthreads();
  }
  if (tid == 0) {
    a.off[a.T] = (uint32_t)base0;
    a.off[2 * a.T + 1] = (uint32_t)base1;
    a.tot[0] = base0;
    a.tot[1] = base1;
  }
}

// rule 9's road_point: the first shape segment with s <= cum[i+1], or the last (fp32, no FMA)
__device__ __forceinline__ float2 road_point(const DevGraph& g, uint32_t va, uint32_t vb, uint32_t s) {
  uint32_t lo = va + 1u, hi = vb;        // first vertex in (va, vb] with cum >= s, or vb
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2u;
    if (g.verts[m].z >= s) hi = m; else lo = m + 1u;
  }
  const uint4 A = g.verts[lo - 1u], B = g.verts[lo];
  const uint32_t d = B.z - A.z;
  float t = 0.0f;
  if (d > 0u) t = (float)(s - A.z) / (float)d;
  const float alon = __uint_as_float(A.x), alat = __uint_as_float(A.y);
  return make_float2(alon + t * (__uint_as_float(B.x) - alon), alat + t * (__uint_as_float(B.y) - alat));
}

__global__ void __launch_bounds__(kFillThreads) k_edge_fill(DevGraph g, EdgeArgs a) {
  const uint64_t v = (uint64_t)blockIdx.x * kFillThreads + threadIdx.x;   // visit of the lane
  if (v >= a.visits) return;
  uint32_t lo = 0u, hi = a.T;            // its trace: the first k with edge_off[k + 1] > v (edge_off[T] = visits)
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2u;
    if (a.off[m + 1u] > v) hi = m; else lo = m + 1u;
  }
  const uint32_t k = lo;
  const uint32_t idx = (uint32_t)v - a.off[k];
  const uint4* src = a.stage + 4ull * (a.trav_off[a.trace_off[k]] + idx);
  const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
  uint4* dst = a.edges + 4ull * v;
  dst[0] = q0; dst[1] = q1; dst[2] = q2; dst[3] = q3;
  float2* sh = a.shape + a.off[a.T + 1 + k];
  const uint4 er = g.edges[q0.x];
  const uint32_t road = er.w >> 1, L = er.y;
  const bool rev = (er.w & 1u) != 0u;
  const uint32_t va = a.road_vert_off[road], vb = a.road_vert_off[road + 1] - 1u;
  const uint32_t s_b = rev ? L - q0.z : q0.z, s_e = rev ? L - q0.w : q0.w;
  if (q3.z & kEdgeChainFirst) sh[q2.z] = road_point(g, va, vb, s_b);
  sh[q2.w] = road_point(g, va, vb, s_e);
  const uint32_t nint = q2.w - q2.z - 1u;
  if (nint) {
    uint32_t first;
    (void)interior(g, va, vb, min(s_b, s_e), max(s_b, s_e), first);
    for (uint32_t i = 0; i < nint; ++i) {   // travel order: descending on a reverse edge
      const uint4 vt = g.verts[rev ? first + nint - 1u - i : first + i];
      sh[q2.z + 1u + i] = make_float2(__uint_as_float(vt.x), __uint_as_float(vt.y));
    }
  }
}

// grow-only device buffer of n bytes (by half again)
void grow(DevBuf<char>& p, uint64_t need, const char* what) {
  if (need <= p.cap()) return;
  const uint64_t c = std::max<uint64_t>(need + need / 2, 4096);
  p.reserve(c, (std::string("matched-edge ") + what + " buffer of " + std::to_string(c) + " bytes does not fit in HBM").c_str());
}

}  // namespace

void Matcher::matched_edges(uint64_t out[2]) {
  RM_HIP(hipSetDevice(eng_->device()));
  sync();
  const uint32_t T = n_traces_;
  const uint64_t R = n_path_;   // one traversal record per chosen path edge
  me_traces_ = T; me_n_ = 0; me_v_ = 0; me_ms_ = 0.0; me_ran_ = true;
  me_timer_.harvest(nullptr);   // (a pair a call that threw left behind)
  out[0] = out[1] = 0;
  if (!T) return;
  if (R >= 0xffffffffull) throw BatchTooLarge("batch too large (traversal records >= 2^32)");
  const uint32_t* rvo = eng_->road_vert_off_dev();
  // per trace 2 counts, 2 (T + 1) offsets, then the two totals (8-byte aligned)
  const uint64_t words = 4ull * T + 2;
  grow(me_small_, (words + (words & 1)) * 4 + 16, "offset");
  grow(me_stage_, std::max<uint64_t>(R, 1) * sizeof(MatchedEdge), "staging");
  const Workspace& w = ws_;
  EdgeArgs a;
  a.T = T; a.total = (uint32_t)R; a.P = n_points_; a.visits = 0;
  a.trace_off = in_.trace_off; a.state_orig = w.state_orig; a.state_time = w.state_time;
  a.path_off = w.path_off; a.path_cnt = w.path_cnt; a.path_inline = w.path_inline; a.path_pool = w.path_pool;
  a.path_sab = w.path_sab; a.route_dist = w.route_dist; a.trav_off = w.trav_off; a.rec_slot = w.rec_slot;
  a.trace_err = w.trace_err;
  a.road_vert_off = rvo;
  a.stage = (uint4*)me_stage_.get();
  a.cnt = (uint32_t*)me_small_.get();
  a.off = a.cnt + 2ull * T;
  a.tot = (unsigned long long*)(me_small_ + (words + (words & 1)) * 4);
  a.edges = nullptr; a.shape = nullptr;
  const DevGraph g = eng_->dev_snapshot();
  // every run path leaves rec_slot filled (k_rec_slot, or the path scan's fused apply pass)
  me_timer_.tic(0, stream_);
  hipLaunchKernelGGL(k_edge_visits, dim3(T), dim3(64), 0, stream_, g, a);
  hipLaunchKernelGGL(k_edge_scan, dim3(1), dim3(kScanThreads), 0, stream_, a);
  me_timer_.toc(stream_);
  RM_HIP(hipGetLastError());
  unsigned long long tot[2] = {0, 0};
  RM_HIP(hipMemcpyAsync(tot, a.tot, sizeof tot, hipMemcpyDeviceToHost, stream_));
  sync();
  if (tot[0] > R || tot[1] >= 0xffffffffull) throw BatchTooLarge("batch too large (shape vertices >= 2^32)");
  me_timer_.harvest(&me_ms_);
  if (tot[0]) {
    grow(me_edges_, tot[0] * sizeof(MatchedEdge), "record");
    grow(me_shape_, tot[1] * sizeof(float2), "shape");
    a.edges = (uint4*)me_edges_.get();
    a.shape = (float2*)me_shape_.get();
    a.visits = tot[0];
    const uint32_t grid = (uint32_t)((tot[0] + kFillThreads - 1) / kFillThreads);
    me_timer_.tic(0, stream_);
    hipLaunchKernelGGL(k_edge_fill, dim3(grid), dim3(kFillThreads), 0, stream_, g, a);
    me_timer_.toc(stream_);
    RM_HIP(hipGetLastError());
    sync();
    me_timer_.harvest(&me_ms_);
  }
  me_n_ = tot[0]; me_v_ = tot[1];
  out[0] = me_n_; out[1] = me_v_;
}

void Matcher::get_matched_edges(uint32_t* edge_off, MatchedEdge* edges, uint32_t* shape_off, float* shape) {
  RM_HIP(hipSetDevice(eng_->device()));
  sync();
  if (!me_ran_) throw std::runtime_error("matched_edges has not run");
  const uint32_t T = me_traces_;
  if (!T) { edge_off[0] = 0; shape_off[0] = 0; return; }
  const uint32_t* off = (const uint32_t*)me_small_.get() + 2ull * T;
  RM_HIP(hipMemcpyAsync(edge_off, off, (T + 1ull) * 4, hipMemcpyDeviceToHost, stream_));
  RM_HIP(hipMemcpyAsync(shape_off, off + T + 1, (T + 1ull) * 4, hipMemcpyDeviceToHost, stream_));
  if (me_n_) {
    RM_HIP(hipMemcpyAsync(edges, me_edges_, me_n_ * sizeof(MatchedEdge), hipMemcpyDeviceToHost, stream_));
    RM_HIP(hipMemcpyAsync(shape, me_shape_, me_v_ * sizeof(float2), hipMemcpyDeviceToHost, stream_));
  }
  sync();
}

}  // namespace rm
