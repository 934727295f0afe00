// sessions.hip — vehicle sessions (DESIGN.md §3 rule 12): the reference's streaming batcher
// (BatchingProcessor.java:57-106, Batch.java:35-90) kept and triggered in HBM beside a matcher.
//
//   store     the points of every vehicle, packed SoA grouped by vehicle, in one of two buffers;
//             per vehicle {off, cnt, scan_from, try_from, max_sep, last_update}
//   append    a micro-batch is grouped by a stable radix sort on vehicle << 32 | arrival, a scan of
//             kept + new counts lays the other buffer out, and one thread per point copies the kept
//             old points and the new ones there (which is also what reclaims trimmed prefixes)
//   trigger   k_sess_trigger: 16 lanes per vehicle, 16 arrivals a step -- the fp64 distance to
//             point 0 per lane, an inclusive prefix maximum of the f32 values across the group seeded
//             with the carried max_sep, the three-part condition per lane, a ballot restricted to
//             the group for the first triggering arrival.  max_sep covers the points before
//             scan_from and no arrival before try_from may trigger, so the kernel that searches
//             on after a trim is also the one that recomputes max_sep over the kept points
//   rounds    the triggered vehicles' lists are gathered into the matcher's workspace inputs,
//             run_device matches and reports them (failure isolation on), k_sess_trim applies
//             shape_used to the vehicle and keeps the reports the forwarding rule passes; the
//             triggered vehicles are the next round's work list; the host reads the round's counts
//             from pinned memory and stops at zero triggers
//   output    windows and forwarded reports of a call, radix-sorted by the triggering arrival
//
//   entries   push() stages host arrays through pinned memory; push_device() takes arrivals that
//             already lie in HBM (the line reader's points, rule 14) and joins push() at the append
//
// Nothing here loops over points or vehicles on the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "engine.hpp"
#include "sess_dist.hpp"

namespace rm {

namespace {

constexpr int kSeW = 16;          // lanes per vehicle (one DPP row)
constexpr int kSeThreads = 256;   // 16 vehicles per block

// device counters of a call (Session::Impl::ctr; the host reads them all at each round's read-back)
enum SessCtr : int {
  kSTrig = 0,      // triggered vehicles of the round (zeroed per round)
  kSPts,           // points of their windows (zeroed per round)
  kSWin,           // window records of the call
  kSRep,           // forwarded reports of the call
  kSTrims, kSCleared, kSFailed, kSInvalid,
  kSSkip,          // arrivals that found their vehicle empty (not evaluated)
  kSErr,           // bit 0 vehicle index out of range, 1 NaN time, 2 output overflow
  kSTotal,         // points in the store after the append
  kSActive,        // vehicles with new arrivals
  kSOwn,           // a sharded push: the points of the call whose vehicle this rank owns
  kSNumCtr = 16
};

struct PtBuf {   // one buffer of the store
  float* lon = nullptr; float* lat = nullptr; float* acc = nullptr; double* time = nullptr;
  uint32_t* arr = nullptr;   // arrival index in the current push (kNone: an older point)
  uint32_t* veh = nullptr;
  uint64_t cap = 0;
};

struct SessArgs {   // what the session kernels share, by value
  uint32_t nV;
  uint32_t* off; uint32_t* cnt; uint32_t* scan_from; uint32_t* try_from; float* max_sep; long long* last_update;
  const float* lon; const float* lat; const double* time; const uint32_t* arr;   // the current buffer
  uint32_t* ctr;
  // the round's triggered vehicles: vehicle, list index of the trigger, window size, window record
  uint32_t* tveh; uint32_t* tidx; uint32_t* wcnt; uint32_t* wslot;
  SessionWindow* win; unsigned long long* win_key; uint32_t win_cap;
  double dist_m, time_s; uint32_t count, max_pts;
};

__global__ void k_sess_keys(uint64_t n, const uint32_t* veh, const double* time, uint32_t nV, unsigned long long* key,
                            uint32_t* ctr) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t v = veh[j];
  const double t = time[j];
  if (v >= nV) atomicOr(ctr + kSErr, 1u);
  if (!(t == t)) atomicOr(ctr + kSErr, 2u);
  key[j] = ((unsigned long long)v << 32) | (unsigned long long)j;
}

// The masked push of a sharded stream (DESIGN.md §3 rule 16): the call's points whose vehicle this
// rank owns, then their keys packed in arrival order.  A key keeps the point's index among all the
// points of the call, so the copy reads the unmasked arrays and a window's arrival is the global one.
__global__ void k_sess_own(uint64_t n, const uint32_t* veh, int nranks, int rank, uint32_t* flag) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) flag[j] = vehicle_owner(veh[j], nranks) == rank ? 1u : 0u;
}
__global__ void k_sess_own_pack(uint64_t n, const unsigned long long* key, const uint32_t* flag, const uint32_t* ofs,
                                unsigned long long* out, uint32_t* ctr) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (flag[j]) out[ofs[j]] = key[j];
  if (j + 1 == n) ctr[kSOwn] = ofs[j] + flag[j];
}

// the new points of a vehicle are sorted[nstart[v] .. nend[v]) (both zeroed before: none)
__global__ void k_sess_runs(uint64_t n, const unsigned long long* key, uint32_t nV, uint32_t* nstart, uint32_t* nend) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t v = (uint32_t)(key[j] >> 32);
  if (v >= nV) return;
  if (j == 0 || (uint32_t)(key[j - 1] >> 32) != v) nstart[v] = (uint32_t)j;
  if (j + 1 == n || (uint32_t)(key[j + 1] >> 32) != v) nend[v] = (uint32_t)j + 1u;
}

__global__ void k_sess_tot(uint32_t nV, const uint32_t* cnt, const uint32_t* nstart, const uint32_t* nend, uint32_t* tot) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v > nV) return;
  tot[v] = v < nV ? cnt[v] + (nend[v] - nstart[v]) : 0u;   // (tot[nV] = 0: the scan's last entry is the total)
}

// one thread per point: the kept old points [0, extent) of `src`, then the n new ones in sorted order
__global__ void k_sess_copy(uint64_t extent, uint64_t n, uint64_t n_src, uint32_t nV, PtBuf src, PtBuf dst, const uint32_t* off,
                            const uint32_t* cnt, const uint32_t* noff, const uint32_t* nstart,
                            const unsigned long long* key, const float* b_lon, const float* b_lat, const double* b_time,
                            const float* b_acc) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < extent) {
    const uint32_t v = src.veh[q];
    if (v >= nV) return;
    const uint32_t o = off[v];
    if (q < o || q >= (uint64_t)o + cnt[v]) return;   // a trimmed prefix or a dropped list
    const uint64_t d = (uint64_t)noff[v] + (q - o);
    if (d >= dst.cap) return;
    dst.lon[d] = src.lon[q]; dst.lat[d] = src.lat[q]; dst.acc[d] = src.acc[q]; dst.time[d] = src.time[q];
    dst.arr[d] = kNone; dst.veh[d] = v;
    return;
  }
  const uint64_t j = q - extent;
  if (j >= n) return;
  const unsigned long long k = key[j];
  const uint32_t v = (uint32_t)(k >> 32), a = (uint32_t)k;
  if (v >= nV || a >= n_src) return;
  const uint64_t d = (uint64_t)noff[v] + cnt[v] + (j - nstart[v]);
  if (d >= dst.cap) return;
  dst.lon[d] = b_lon[a]; dst.lat[d] = b_lat[a]; dst.acc[d] = b_acc ? b_acc[a] : -1.0f; dst.time[d] = b_time[a];
  dst.arr[d] = a; dst.veh[d] = v;
}

// the new layout becomes the vehicles' state; vehicles with new arrivals form round 0's work list
__global__ void k_sess_commit(uint32_t nV, uint32_t* off, uint32_t* cnt, long long* last_update, const uint32_t* noff,
                              const uint32_t* nstart, const uint32_t* nend, const unsigned long long* key,
                              const long long* stamp, uint32_t* act, uint32_t* ctr) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nV) return;
  const uint32_t c = cnt[v], nn = nend[v] - nstart[v];
  off[v] = noff[v];
  if (!nn) return;
  cnt[v] = c + nn;
  last_update[v] = stamp[(uint32_t)key[nend[v] - 1u]];   // (a list the push leaves empty zeroes it again)
  if (c == 0u) atomicAdd(ctr + kSSkip, 1u);
  act[atomicAdd(ctr + kSActive, 1u)] = v;
}

// lane 0 of a group: the vehicle's list [0, i] goes to the matcher as one window of the round
__device__ __forceinline__ void sess_emit_window(const SessArgs& a, uint32_t v, uint32_t i, uint32_t tag, uint32_t err) {
  const uint32_t slot = atomicAdd(a.ctr + kSWin, 1u);
  if (slot < a.win_cap) {
    SessionWindow w;
    w.vehicle = v; w.arrival = tag; w.n_points = i + 1u; w.shape_used = -1; w.n_reports = 0u; w.err = err;
    a.win[slot] = w;
    a.win_key[slot] = tag;
  } else {
    atomicOr(a.ctr + kSErr, 4u);
  }
  if (err) return;   // (capped: recorded, not matched)
  const uint32_t k = atomicAdd(a.ctr + kSTrig, 1u);
  if (k < a.nV) {
    a.tveh[k] = v; a.tidx[k] = i; a.wcnt[k] = i + 1u; a.wslot[k] = slot;
    atomicAdd(a.ctr + kSPts, i + 1u);
  }
}

// Rule 12's arrival loop for the vehicles act[0 .. n_act): a 16-lane group per vehicle, four
// vehicles per wave.  Each step evaluates the arrivals base + lane of the vehicle's list.
__global__ void __launch_bounds__(kSeThreads) k_sess_trigger(SessArgs a, uint32_t n_act, const uint32_t* act) {
  const uint32_t g = (blockIdx.x * kSeThreads + threadIdx.x) / kSeW;
  const uint32_t lane = threadIdx.x & (kSeW - 1);
  if (g >= n_act) return;
  const uint32_t v = act[g];
  if (v >= a.nV) return;
  uint32_t off = a.off[v], cnt = a.cnt[v], tf = a.try_from[v], base = a.scan_from[v];
  float m = a.max_sep[v];
  bool fired = false;
  while (cnt > 0u) {
    const float lon0 = a.lon[off], lat0 = a.lat[off];
    const double t0 = a.time[off];
    bool restart = false;
    while (base < cnt) {
      const uint32_t i = base + lane;
      const bool valid = i < cnt;
      float d = 0.0f;
      double ti = t0;
      if (valid) {
        d = (float)sess_distance(a.lon[off + i], a.lat[off + i], lon0, lat0);
        ti = a.time[off + i];
      }
      float pm = d;   // inclusive prefix maximum across the group, then the carried one
#pragma unroll
      for (int s = 1; s < kSeW; s <<= 1) {
        const float o = __shfl_up(pm, s, kSeW);
        if ((int)lane >= s && o > pm) pm = o;
      }
      if (m > pm) pm = m;
      const bool tried = valid && i >= tf;
      const bool trig = tried && sess_reports(pm, i + 1u, t0, ti, a.dist_m, a.count, a.time_s);
      const bool capped = tried && !trig && a.max_pts > 0u && i + 1u >= a.max_pts;
      const uint32_t bal = (uint32_t)(__ballot(trig || capped) >> (threadIdx.x & 48u)) & 0xffffu;
      if (bal) {
        const uint32_t e = (uint32_t)__ffs((int)bal) - 1u;
        const bool e_trig = __shfl((int)trig, (int)e, kSeW) != 0;
        const uint32_t ie = base + e;
        if (lane == 0u) sess_emit_window(a, v, ie, a.arr[off + ie], e_trig ? 0u : kSessCapped);
        if (e_trig) { fired = true; break; }
        // cleared at the cap: the next arrival starts a new list
        off += ie + 1u; cnt -= ie + 1u;
        m = 0.0f; base = 1u; tf = 1u;
        if (lane == 0u && cnt > 0u) atomicAdd(a.ctr + kSSkip, 1u);
        restart = true;
        break;
      }
      m = __shfl(pm, kSeW - 1, kSeW);
      base += kSeW;
    }
    if (!restart) break;
  }
  if (lane != 0u) return;
  a.off[v] = off; a.cnt[v] = cnt;
  if (fired) return;   // (k_sess_trim sets the rest)
  const uint32_t at = cnt > 1u ? cnt : 1u;
  a.max_sep[v] = m; a.scan_from[v] = at; a.try_from[v] = at;
  if (cnt == 0u) a.last_update[v] = 0;
}

// punctuate (BatchingProcessor.java:86-106): a stale vehicle reports once with thresholds
// (0, 2, 0) -- its whole list is a window of the round -- or is dropped here when that bails
__global__ void k_sess_stale(SessArgs a, long long ts, long long gap) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.nV) return;
  const uint32_t c = a.cnt[v];
  if (c == 0u || !(ts - a.last_update[v] > gap)) return;
  const uint32_t o = a.off[v];
  if (sess_reports(a.max_sep[v], c, a.time[o], a.time[o + c - 1u], 0.0, 2u, 0.0)) {
    sess_emit_window(a, v, c - 1u, v, 0u);
    return;
  }
  a.cnt[v] = 0u; a.scan_from[v] = 1u; a.try_from[v] = 1u; a.max_sep[v] = 0.0f; a.last_update[v] = 0;
}

// one thread per destination point of the round's windows
__global__ void k_sess_gather(SessArgs a, uint32_t T, uint32_t P, const uint32_t* wofs, float* o_lon, float* o_lat,
                              double* o_time, float* o_acc, const float* s_acc, uint32_t* trace_off, uint32_t* trace_opt) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= P) return;
  uint32_t lo = 0u, hi = T;   // the window k with wofs[k] <= d < wofs[k + 1]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (wofs[mid] <= d) lo = mid; else hi = mid;
  }
  const uint32_t k = lo, w0 = wofs[k];
  const uint32_t src = a.off[a.tveh[k]] + (d - w0);
  o_lon[d] = a.lon[src]; o_lat[d] = a.lat[src]; o_time[d] = a.time[src]; o_acc[d] = s_acc[src];
  if (d == w0) { trace_off[k] = w0; trace_opt[k] = 0u; }
  if (d == 0u) trace_off[T] = P;
}

__device__ __forceinline__ bool sess_forwards(const ReportRec& r) {   // Segment.java:38-40
  return r.t0 > 0 && r.t1 > 0 && r.t1 > r.t0 && r.length > 0 && r.queue_length >= 0;
}

// one thread per window of the round: the trim (Batch.java:73-87) and the forwarding filter
__global__ void k_sess_trim(SessArgs a, uint32_t T, int evict, const ReportStats* stats, const uint32_t* trace_err,
                            const uint32_t* rep_cnt, const uint32_t* rep_base, const ReportRec* reps, SessionReport* out,
                            unsigned long long* out_key, uint32_t out_cap) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= T) return;
  const uint32_t v = a.tveh[k], n = a.tidx[k] + 1u, slot = a.wslot[k];
  const uint32_t err = trace_err[k];
  const int32_t su = stats[k].shape_used;
  const uint32_t nrep = err ? 0u : rep_cnt[k];
  uint32_t trim_to = n;
  if (err) atomicAdd(a.ctr + kSFailed, 1u);
  else if (su >= 0) { trim_to = (uint32_t)su < n ? (uint32_t)su : n; atomicAdd(a.ctr + kSTrims, 1u); }
  else atomicAdd(a.ctr + kSCleared, 1u);
  const uint32_t c = a.cnt[v];
  if (evict) trim_to = c;
  const uint32_t left = c - trim_to;
  a.off[v] += trim_to; a.cnt[v] = left;
  a.scan_from[v] = 1u; a.try_from[v] = n > trim_to + 1u ? n - trim_to : 1u; a.max_sep[v] = 0.0f;
  if (left == 0u) a.last_update[v] = 0;
  else if (trim_to == n) atomicAdd(a.ctr + kSSkip, 1u);   // the next arrival finds the list empty
  uint32_t tag = v;
  if (slot < a.win_cap) {
    a.win[slot].shape_used = err ? -1 : su; a.win[slot].n_reports = nrep; a.win[slot].err = err;
    tag = a.win[slot].arrival;
  }
  if (!nrep) return;
  const ReportRec* r = reps + rep_base[k];
  uint32_t kept = 0u;
  for (uint32_t q = 0; q < nrep; ++q) kept += sess_forwards(r[q]) ? 1u : 0u;
  if (nrep > kept) atomicAdd(a.ctr + kSInvalid, nrep - kept);
  if (!kept) return;
  const uint32_t at = atomicAdd(a.ctr + kSRep, kept);
  if ((uint64_t)at + kept > out_cap) { atomicOr(a.ctr + kSErr, 4u); return; }
  uint32_t j = 0u;
  for (uint32_t q = 0; q < nrep; ++q) {
    if (!sess_forwards(r[q])) continue;
    SessionReport s;
    s.r = r[q]; s.vehicle = v; s.window = slot;
    out[at + j] = s;
    out_key[at + j] = ((unsigned long long)tag << 32) | q;
    ++j;
  }
}

// the stream time of arrivals that come without one: one for all, or each point's own time
__global__ void k_sess_stamp(uint64_t n, const double* time, int has_stamp, long long stamp, long long* out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = has_stamp ? stamp : (long long)(time[j] * 1000.0);
}

__global__ void k_sess_sort_windows(uint32_t n, const uint32_t* perm, const SessionWindow* src, SessionWindow* dst, uint32_t* rank) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t s = perm[k];
  dst[k] = src[s];
  rank[s] = k;
}
__global__ void k_sess_sort_reports(uint32_t n, uint32_t n_win, const uint32_t* perm, const SessionReport* src, const uint32_t* rank,
                                    SessionReport* dst) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  SessionReport s = src[perm[k]];
  s.window = s.window < n_win ? rank[s.window] : kNone;
  dst[k] = s;
}

}  // namespace

struct PtStore {   // a PtBuf's owner
  DevBuf<float> lon, lat, acc;
  DevBuf<double> time;
  DevBuf<uint32_t> arr, veh;
  uint64_t cap = 0;
  PtBuf view() const { return PtBuf{lon, lat, acc, time, arr, veh, cap}; }
};

struct Session::Impl {
  static constexpr const char* kFull = "session buffers do not fit in HBM";
  Matcher* m = nullptr;
  SessionParams sp;
  uint32_t nV = 0;
  // per vehicle
  DevBuf<uint32_t> off, cnt, scan_from, try_from;
  DevBuf<float> max_sep;
  DevBuf<long long> last_update;
  DevBuf<uint32_t> nstart, nend, tot, noff, list[2], tidx, wcnt, wofs, wslot;
  DevBuf<uint32_t> ctr;
  PinBuf<uint32_t> hctr;   // pinned mirror of ctr
  // the store
  PtStore buf[2];
  int cur = 0;
  uint64_t extent = 0;        // points of buf[cur] in use (holes of trimmed prefixes included)
  // the micro-batch: pinned staging and its device copy (grow-only)
  PinBuf<char> hstage; DevBuf<char> dstage; uint64_t stage_cap = 0;
  DevBuf<unsigned long long> key0, key1; uint64_t key_cap = 0;
  DevBuf<long long> gen_stamp; uint64_t gen_cap = 0;   // push_device: stamps made on the device
  // a call's output: as written (unsorted) and sorted by triggering arrival
  DevBuf<SessionWindow> win, win_s; DevBuf<unsigned long long> win_key;
  DevBuf<uint32_t> win_rank; uint32_t win_cap = 0;
  DevBuf<SessionReport> rep, rep_s; DevBuf<unsigned long long> rep_key; uint32_t rep_cap = 0;
  DevBuf<unsigned long long> skey; DevBuf<uint32_t> sidx0, sidx1; uint64_t sort_cap = 0;
  ScanScratch scr{kFull};
  uint64_t rep_bound = 0;     // host bound on the reports written so far in the call
  uint64_t n_win = 0, n_rep = 0, rounds = 0, triggers = 0, arrivals = 0;
  int sh_nranks = 1, sh_rank = 0;   // the shard of the call under way (1, 0: every point is this rank's)
  bool sharded = false;             // a sharded push has been made: a tile store fed from here keys its rows
  // HIP-event pairs of the call, by part (0 upload, 1 append, 2 trigger, 3 match, 4 trim)
  PartTimer timer;
  double ms[5] = {0, 0, 0, 0, 0};

  void ensure_buf(PtStore& b, uint64_t n) {   // (no contents to keep: the copy's destination)
    if (n <= b.cap) return;
    b.cap = 0;
    const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
    b.lon.reserve(c, kFull); b.lat.reserve(c, kFull); b.acc.reserve(c, kFull); b.time.reserve(c, kFull);
    b.arr.reserve(c, kFull); b.veh.reserve(c, kFull);
    b.cap = c;
  }
  void ensure_stage(uint64_t n) {
    if (n > stage_cap) {
      stage_cap = 0;
      const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
      hstage.reserve(c * 32);
      dstage.reserve(c * 32, kFull);
      stage_cap = c;
    }
    ensure_keys(n);
  }
  void ensure_keys(uint64_t n) {
    if (n > key_cap) {
      key_cap = 0;
      const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
      key0.reserve(c, kFull); key1.reserve(c, kFull);
      key_cap = c;
    }
  }
  void ensure_win(uint64_t n) {
    if (n <= win_cap) return;
    if (n >= 0xffffffffull) throw BatchTooLarge("session call too large");
    win_cap = 0;
    const uint32_t c = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n + n / 2, 1024), 0xfffffffeull);
    win.reserve(c, kFull); win_s.reserve(c, kFull); win_key.reserve(c, kFull); win_rank.reserve(c, kFull);
    win_cap = c;
    ensure_sort(c);
  }
  void ensure_sort(uint64_t n) {
    if (n <= sort_cap) return;
    sort_cap = 0;
    skey.reserve(n, kFull); sidx0.reserve(n, kFull); sidx1.reserve(n, kFull);
    sort_cap = n;
  }
  // room for `more` reports behind the `keep` already written (their contents move)
  void ensure_rep(uint64_t keep, uint64_t more, hipStream_t st) {
    const uint64_t n = keep + more;
    if (n <= rep_cap) return;
    if (n >= 0xffffffffull) throw BatchTooLarge("session call too large");
    const uint32_t c = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n + n / 2, 4096), 0xfffffffeull);
    DevBuf<SessionReport> r2, s2;   // all three first: a full HBM leaves the session as it was
    DevBuf<unsigned long long> k2;
    r2.reserve(c, kFull); k2.reserve(c, kFull); s2.reserve(c, kFull);
    const uint64_t have = std::min<uint64_t>(keep, rep_cap);
    if (have) {
      RM_HIP(hipMemcpyAsync(r2, rep, have * sizeof(SessionReport), hipMemcpyDeviceToDevice, st));
      RM_HIP(hipMemcpyAsync(k2, rep_key, have * 8, hipMemcpyDeviceToDevice, st));
      RM_HIP(hipStreamSynchronize(st));
    }
    rep = std::move(r2); rep_key = std::move(k2); rep_s = std::move(s2);   // (the old blocks go with r2, k2, s2)
    rep_cap = c;
    ensure_sort(c);
  }
  SessArgs args() const {
    SessArgs a;
    a.nV = nV;
    a.off = off; a.cnt = cnt; a.scan_from = scan_from; a.try_from = try_from; a.max_sep = max_sep; a.last_update = last_update;
    a.lon = buf[cur].lon; a.lat = buf[cur].lat; a.time = buf[cur].time; a.arr = buf[cur].arr;
    a.ctr = ctr;
    a.tveh = nullptr; a.tidx = tidx; a.wcnt = wcnt; a.wslot = wslot;
    a.win = win; a.win_key = win_key; a.win_cap = win_cap;
    a.dist_m = sp.report_dist_m; a.time_s = sp.report_time_s; a.count = sp.report_count; a.max_pts = sp.max_vehicle_points;
    return a;
  }
  void begin_call(hipStream_t st) {
    timer.harvest(nullptr);   // (pairs a call that threw left behind)
    for (double& x : ms) x = 0.0;
    n_win = n_rep = rounds = triggers = arrivals = 0;
    rep_bound = 0;
    RM_HIP(hipMemsetAsync(ctr, 0, kSNumCtr * sizeof(uint32_t), st));
  }
  void read_ctr(hipStream_t st) {
    RM_HIP(hipMemcpyAsync(hctr, ctr, kSNumCtr * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RM_HIP(hipStreamSynchronize(st));
    timer.harvest(ms);
    if (hctr[kSErr] & 4u) throw std::runtime_error("session output buffers overflowed");
  }
  // lay the store out anew in the other buffer with the n sorted new points (key1; their arrival
  // indices run below n_src, the length of the b_ arrays) behind each vehicle's kept ones; the
  // vehicles' state is untouched until commit()
  void layout_and_copy(uint64_t n, uint64_t n_src, const float* b_lon, const float* b_lat, const double* b_time, const float* b_acc,
                       hipStream_t st) {
    RM_HIP(hipMemsetAsync(nstart, 0, nV * sizeof(uint32_t), st));
    RM_HIP(hipMemsetAsync(nend, 0, nV * sizeof(uint32_t), st));
    if (n) hipLaunchKernelGGL(k_sess_runs, dim3(grid(n)), dim3(256), 0, st, n, key1, nV, nstart, nend);
    hipLaunchKernelGGL(k_sess_tot, dim3(grid(nV + 1ull)), dim3(256), 0, st, nV, cnt, nstart, nend, tot);
    scr.scan<uint32_t>(tot, noff, nV + 1u, st);
    RM_HIP(hipMemcpyAsync(ctr + kSTotal, noff + nV, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    ensure_buf(buf[1 - cur], extent + n);
    if (extent + n)
      hipLaunchKernelGGL(k_sess_copy, dim3(grid(extent + n)), dim3(256), 0, st, extent, n, n_src, nV, buf[cur].view(),
                         buf[1 - cur].view(), off, cnt, noff, nstart, key1, b_lon, b_lat, b_time, b_acc);
  }
  void commit(const long long* stamp, hipStream_t st) {
    hipLaunchKernelGGL(k_sess_commit, dim3(grid(nV)), dim3(256), 0, st, nV, off, cnt, last_update, noff, nstart, nend, key1,
                       stamp, list[0], ctr);
    cur = 1 - cur;
  }
};

Session::Session(Matcher* m, uint32_t n_vehicles, const SessionParams& sp) : p_(new Impl) {
  Impl& s = *p_;
  if (!m) throw std::runtime_error("runner is NULL");
  if (n_vehicles == 0 || n_vehicles >= 0x7fffffffu) throw std::runtime_error("session needs 1 .. 2^31 - 2 vehicles");
  if (!(sp.report_dist_m >= 0.0) || !(sp.report_time_s == sp.report_time_s))
    throw std::runtime_error("session thresholds must be numbers, the distance non-negative");
  s.m = m; s.sp = sp; s.nV = n_vehicles;
  s.sp.run.do_report = 1;
  s.sp.run.zero_hist = 0;
  s.sp.run.prefetch_segments = 0;
  RM_HIP(hipSetDevice(m->eng_->device()));
  m->scan_options(&s.sp.opt, 1);   // the checks of a batch's option sets
  const uint64_t V = n_vehicles;
  for (DevBuf<uint32_t>* b : {&s.off, &s.cnt, &s.scan_from, &s.try_from, &s.nstart, &s.nend}) b->reserve(V, Impl::kFull);
  s.max_sep.reserve(V, Impl::kFull); s.last_update.reserve(V, Impl::kFull);
  for (DevBuf<uint32_t>* b : {&s.tot, &s.noff, &s.list[0], &s.list[1], &s.tidx, &s.wcnt, &s.wofs, &s.wslot})
    b->reserve(V + 1, Impl::kFull);
  s.ctr.reserve(kSNumCtr, Impl::kFull);
  s.hctr.reserve(kSNumCtr);
  hipStream_t st = m->stream_;
  RM_HIP(hipMemsetAsync(s.off, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.cnt, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.max_sep, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.last_update, 0, V * 8, st));
  // the counters: a read-out before the first call (get_store, the snapshot's pack) reads them
  RM_HIP(hipMemsetAsync(s.ctr, 0, kSNumCtr * sizeof(uint32_t), st));
  std::memset(s.hctr, 0, kSNumCtr * sizeof(uint32_t));
  // an empty vehicle: scan_from = try_from = 1 (its first point never triggers)
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(V)), dim3(256), 0, st, n_vehicles, s.scan_from, 1u);
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(V)), dim3(256), 0, st, n_vehicles, s.try_from, 1u);
  RM_HIP(hipGetLastError());
  RM_HIP(hipStreamSynchronize(st));
}

Session::~Session() {
  (void)hipSetDevice(p_->m->eng_->device());
  (void)hipStreamSynchronize(p_->m->stream_);
}

uint32_t Session::n_vehicles() const { return p_->nV; }
int Session::device() const { return p_->m->eng_->device(); }
const SessionReport* Session::reports_device() const { return p_->rep_s; }
const SessionWindow* Session::windows_device() const { return p_->win_s; }
bool Session::sharded() const { return p_->sharded; }
uint64_t Session::n_reports() const { return p_->n_rep; }
uint64_t Session::n_windows() const { return p_->n_win; }
void Session::times(double ms[5]) const { for (int i = 0; i < 5; ++i) ms[i] = p_->ms[i]; }

// gather the round's T windows (P points) into the matcher's workspace, match and report them,
// then trim their vehicles and keep the forwarded reports
void Session::match_round(uint32_t T, uint64_t P, bool evict) {
  Impl& s = *p_;
  Matcher& m = *s.m;
  hipStream_t st = m.stream_;
  if (P >= 0xffffffffull) throw BatchTooLarge("session round too large (points >= 2^32)");
  s.timer.tic(3, st);
  RM_HIP(hipMemsetAsync(s.wcnt + T, 0, sizeof(uint32_t), st));
  s.scr.scan<uint32_t>(s.wcnt, s.wofs, T + 1u, st);
  m.scan_options(&s.sp.opt, 1);
  m.ensure(P, T, 1);
  m.use_ws_inputs();
  m.from_points_ = false;
  m.n_traces_ = T;
  m.n_points_ = P;
  Workspace& w = m.ws_;
  RM_HIP(hipMemcpyAsync(w.opts, &s.sp.opt, sizeof(MatchOptions), hipMemcpyHostToDevice, st));
  SessArgs a = s.args();
  a.tveh = s.list[1];
  hipLaunchKernelGGL(k_sess_gather, dim3(grid(P)), dim3(256), 0, st, a, T, (uint32_t)P, s.wofs, w.lon, w.lat, w.time, w.acc,
                     s.buf[s.cur].acc, w.trace_off, w.trace_opt);
  RM_HIP(hipStreamSynchronize(st));
  const bool iso = m.isolate_;
  m.isolate_ = true;   // a failed window clears its vehicle alone (BatchingProcessor.java:83-87)
  try {
    m.run_device(s.sp.run);
  } catch (...) {
    m.isolate_ = iso;
    throw;
  }
  m.isolate_ = iso;
  s.timer.toc(st);
  // every report comes from one segment, every segment from at least one traversal record
  s.ensure_rep(s.rep_bound, m.seg_used_, st);
  s.rep_bound += m.seg_used_;
  s.timer.tic(4, st);
  hipLaunchKernelGGL(k_sess_trim, dim3(grid(T)), dim3(256), 0, st, a, T, evict ? 1 : 0, (const ReportStats*)w.stats,
                     (const uint32_t*)w.trace_err, (const uint32_t*)w.rep_cnt, (const uint32_t*)w.seg_base,
                     (const ReportRec*)w.reps, s.rep, s.rep_key, s.rep_cap);
  s.timer.toc(st);
  RM_HIP(hipGetLastError());
}

// list[0] holds the round's work list (hctr[kSActive] vehicles) on entry
void Session::rounds(bool evict, uint64_t out[8]) {
  Impl& s = *p_;
  hipStream_t st = s.m->stream_;
  uint32_t n_act = s.hctr[kSActive];
  for (;;) {
    SessArgs a = s.args();
    a.tveh = s.list[1];
    if (!evict) {
      if (!n_act) break;
      s.timer.tic(2, st);
      RM_HIP(hipMemsetAsync(s.ctr + kSTrig, 0, 2 * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_sess_trigger, dim3(grid((uint64_t)n_act * kSeW, kSeThreads)), dim3(kSeThreads), 0, st, a, n_act,
                         (const uint32_t*)s.list[0]);
      s.timer.toc(st);
      RM_HIP(hipGetLastError());
    }
    s.read_ctr(st);   // the round's triggered count (and the call's counters so far)
    const uint32_t T = s.hctr[kSTrig];
    if (T == 0) break;
    if (T > s.nV) throw std::runtime_error("session trigger list overflowed");
    s.triggers += T;
    s.rounds += 1;
    match_round(T, s.hctr[kSPts], evict);
    if (evict) break;
    std::swap(s.list[0], s.list[1]);   // the trimmed vehicles search on
    n_act = T;
  }
  finish_call(out);
}

// order the call's windows and reports by triggering arrival and fill `out`
void Session::finish_call(uint64_t out[8]) {
  Impl& s = *p_;
  hipStream_t st = s.m->stream_;
  s.read_ctr(st);
  const uint32_t nw = s.hctr[kSWin], nr = s.hctr[kSRep];
  if (nw > s.win_cap || nr > s.rep_cap) throw std::runtime_error("session output buffers overflowed");
  s.timer.tic(4, st);
  if (nw) {
    hipLaunchKernelGGL(k_iota<uint32_t>, dim3(grid(nw)), dim3(256), 0, st, nw, s.sidx0);
    s.scr.sort_pairs(s.win_key.get(), s.skey.get(), s.sidx0, s.sidx1, nw, 64, st);
    hipLaunchKernelGGL(k_sess_sort_windows, dim3(grid(nw)), dim3(256), 0, st, nw, (const uint32_t*)s.sidx1,
                       (const SessionWindow*)s.win, s.win_s, s.win_rank);
  }
  if (nr) {
    hipLaunchKernelGGL(k_iota<uint32_t>, dim3(grid(nr)), dim3(256), 0, st, nr, s.sidx0);
    s.scr.sort_pairs(s.rep_key.get(), s.skey.get(), s.sidx0, s.sidx1, nr, 64, st);
    hipLaunchKernelGGL(k_sess_sort_reports, dim3(grid(nr)), dim3(256), 0, st, nr, nw, (const uint32_t*)s.sidx1,
                       (const SessionReport*)s.rep, (const uint32_t*)s.win_rank, s.rep_s);
  }
  s.timer.toc(st);
  RM_HIP(hipGetLastError());
  RM_HIP(hipStreamSynchronize(st));
  s.timer.harvest(s.ms);
  s.n_win = nw; s.n_rep = nr;
  if (out) {
    out[0] = s.arrivals - std::min<uint64_t>(s.arrivals, s.hctr[kSSkip]);
    out[1] = s.triggers; out[2] = s.hctr[kSTrims]; out[3] = s.hctr[kSCleared]; out[4] = s.hctr[kSFailed];
    out[5] = nr; out[6] = s.hctr[kSInvalid]; out[7] = s.rounds;
  }
}

void Session::push(const SessionPoints& pts, uint64_t out[8]) {
  Impl& s = *p_;
  Matcher& m = *s.m;
  RM_HIP(hipSetDevice(m.eng_->device()));
  hipStream_t st = m.stream_;
  const uint64_t n = pts.n;
  if (n && (!pts.vehicle || !pts.time || !pts.lon || !pts.lat || !pts.stamp_ms)) throw std::runtime_error("session point arrays are NULL");
  if (s.extent + n >= 0xffffffffull) throw BatchTooLarge("session store too large (points >= 2^32)");
  m.sync();
  s.begin_call(st);
  if (n == 0) {
    s.hctr[kSActive] = 0;
    rounds(false, out);
    return;
  }
  s.ensure_stage(n);
  s.ensure_win(n);
  // the micro-batch through pinned staging: stamp, time (8 B each), vehicle, lon, lat, accuracy
  const uint64_t c = s.stage_cap;
  char* h = s.hstage;
  std::memcpy(h, pts.stamp_ms, n * 8);
  std::memcpy(h + c * 8, pts.time, n * 8);
  std::memcpy(h + c * 16, pts.vehicle, n * 4);
  std::memcpy(h + c * 20, pts.lon, n * 4);
  std::memcpy(h + c * 24, pts.lat, n * 4);
  if (pts.accuracy) std::memcpy(h + c * 28, pts.accuracy, n * 4);
  char* d = s.dstage;
  const long long* d_stamp = (const long long*)d;
  const double* d_time = (const double*)(d + c * 8);
  const uint32_t* d_veh = (const uint32_t*)(d + c * 16);
  const float* d_lon = (const float*)(d + c * 20);
  const float* d_lat = (const float*)(d + c * 24);
  const float* d_acc = pts.accuracy ? (const float*)(d + c * 28) : nullptr;
  s.timer.tic(0, st);
  RM_HIP(hipMemcpyAsync(d, h, n * 8, hipMemcpyHostToDevice, st));
  RM_HIP(hipMemcpyAsync(d + c * 8, h + c * 8, n * 8, hipMemcpyHostToDevice, st));
  for (int q = 0; q < (pts.accuracy ? 4 : 3); ++q)
    RM_HIP(hipMemcpyAsync(d + c * (16 + 4 * q), h + c * (16 + 4 * q), n * 4, hipMemcpyHostToDevice, st));
  s.timer.toc(st);
  append(n, d_veh, d_time, d_lon, d_lat, d_acc, d_stamp, out);
}

void Session::check_room(uint64_t n) const {
  if (p_->extent + n >= 0xffffffffull) throw BatchTooLarge("session store too large (points >= 2^32)");
}

void Session::push_device(uint64_t n, const uint32_t* d_vehicle, const double* d_time, const float* d_lon, const float* d_lat,
                          const float* d_acc, const long long* d_stamp, bool has_stamp, int64_t stamp, uint64_t out[8]) {
  Impl& s = *p_;
  Matcher& m = *s.m;
  RM_HIP(hipSetDevice(m.eng_->device()));
  hipStream_t st = m.stream_;
  if (n && (!d_vehicle || !d_time || !d_lon || !d_lat)) throw std::runtime_error("session point arrays are NULL");
  check_room(n);
  m.sync();
  s.begin_call(st);
  if (n == 0) {
    s.hctr[kSActive] = 0;
    rounds(false, out);
    return;
  }
  s.ensure_keys(n);
  s.ensure_win(n);
  if (!d_stamp) {
    if (n > s.gen_cap) {
      s.gen_cap = 0;
      const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
      s.gen_stamp.reserve(c, Impl::kFull);
      s.gen_cap = c;
    }
    s.timer.tic(1, st);
    hipLaunchKernelGGL(k_sess_stamp, dim3(grid(n)), dim3(256), 0, st, n, d_time, has_stamp ? 1 : 0, (long long)stamp, s.gen_stamp);
    s.timer.toc(st);
    d_stamp = s.gen_stamp;
  }
  append(n, d_vehicle, d_time, d_lon, d_lat, d_acc, d_stamp, out);
}

void Session::push_device_sharded(uint64_t n, const uint32_t* d_vehicle, const double* d_time, const float* d_lon,
                                  const float* d_lat, const float* d_acc, const long long* d_stamp, bool has_stamp, int64_t stamp,
                                  int nranks, int rank, uint64_t out[8], uint64_t shard[2]) {
  Impl& s = *p_;
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("session shard needs 0 <= rank < nranks");
  s.sh_nranks = nranks; s.sh_rank = rank;
  try {
    push_device(n, d_vehicle, d_time, d_lon, d_lat, d_acc, d_stamp, has_stamp, stamp, out);
  } catch (...) {
    s.sh_nranks = 1; s.sh_rank = 0;
    throw;
  }
  s.sh_nranks = 1; s.sh_rank = 0;
  s.sharded = true;
  if (shard) { shard[0] = s.arrivals; shard[1] = n - s.arrivals; }
}

// push() behind its staging: the n arrivals lie in HBM.  They are copied into the store before the
// first match round, which reuses the runner's workspace.
void Session::append(uint64_t n, const uint32_t* d_veh, const double* d_time, const float* d_lon, const float* d_lat,
                     const float* d_acc, const long long* d_stamp, uint64_t out[8]) {
  Impl& s = *p_;
  hipStream_t st = s.m->stream_;
  const auto check_input = [&s] {
    if (s.hctr[kSErr] & 1u) throw std::runtime_error("session vehicle index out of range");
    if (s.hctr[kSErr] & 2u) throw std::runtime_error("session point time is NaN");
  };
  s.timer.tic(1, st);
  hipLaunchKernelGGL(k_sess_keys, dim3(grid(n)), dim3(256), 0, st, n, d_veh, d_time, s.nV, s.key0, s.ctr);
  uint64_t m = n;   // the points this rank appends
  if (s.sh_nranks > 1) {
    // the owned points' keys packed in arrival order (the sort buffers of finish_call hold the
    // flags and offsets: ensure_win(n) has sized them), one read of their count
    if (s.sort_cap < n) s.ensure_sort(n);   // (push_device's ensure_win(n) has done it: held here against a reorder)
    uint32_t* flag = s.sidx0;
    uint32_t* ofs = s.sidx1;
    hipLaunchKernelGGL(k_sess_own, dim3(grid(n)), dim3(256), 0, st, n, d_veh, s.sh_nranks, s.sh_rank, flag);
    s.scr.scan<uint32_t>(flag, ofs, n, st);
    hipLaunchKernelGGL(k_sess_own_pack, dim3(grid(n)), dim3(256), 0, st, n, (const unsigned long long*)s.key0,
                       (const uint32_t*)flag, (const uint32_t*)ofs, s.key1, s.ctr);
    s.timer.toc(st);
    RM_HIP(hipGetLastError());
    s.read_ctr(st);
    check_input();   // (over every point of the call, owned or not: the ranks fail together)
    m = s.hctr[kSOwn];
    if (m > n) throw std::runtime_error("session owned-point count out of range");
    std::swap(s.key0, s.key1);
    if (m == 0) {   // nothing of this call is this rank's
      s.hctr[kSActive] = 0;
      rounds(false, out);
      return;
    }
    s.timer.tic(1, st);
  }
  s.scr.sort_keys(s.key0.get(), s.key1.get(), m, st);
  s.layout_and_copy(m, n, d_lon, d_lat, d_time, d_acc, st);
  s.timer.toc(st);
  RM_HIP(hipGetLastError());
  s.read_ctr(st);   // nothing of the session has changed yet: a bad input leaves it as it was
  check_input();
  s.timer.tic(1, st);
  s.commit(d_stamp, st);
  s.timer.toc(st);
  s.extent = s.hctr[kSTotal];
  s.arrivals = m;
  s.read_ctr(st);   // round 0's work list
  rounds(false, out);
}

void Session::punctuate(int64_t timestamp_ms, uint64_t out[8]) {
  Impl& s = *p_;
  Matcher& m = *s.m;
  RM_HIP(hipSetDevice(m.eng_->device()));
  hipStream_t st = m.stream_;
  m.sync();
  s.begin_call(st);
  s.ensure_win(s.nV);
  SessArgs a = s.args();
  a.tveh = s.list[1];
  s.timer.tic(2, st);
  hipLaunchKernelGGL(k_sess_stale, dim3(grid(s.nV)), dim3(256), 0, st, a, (long long)timestamp_ms, (long long)s.sp.session_gap_ms);
  s.timer.toc(st);
  RM_HIP(hipGetLastError());
  rounds(true, out);
}

void Session::get_reports(SessionReport* out) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.m->eng_->device()));
  if (s.n_rep) RM_HIP(hipMemcpy(out, s.rep_s, s.n_rep * sizeof(SessionReport), hipMemcpyDeviceToHost));
}

void Session::get_windows(SessionWindow* out) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.m->eng_->device()));
  if (s.n_win) RM_HIP(hipMemcpy(out, s.win_s, s.n_win * sizeof(SessionWindow), hipMemcpyDeviceToHost));
}

uint64_t Session::get_store(uint32_t* cnt, float* max_sep, int64_t* last_update, float* lon, float* lat, double* time, float* acc) {
  Impl& s = *p_;
  Matcher& m = *s.m;
  RM_HIP(hipSetDevice(m.eng_->device()));
  hipStream_t st = m.stream_;
  m.sync();
  // an append of nothing packs the store (holes of trimmed prefixes and dropped lists go)
  s.layout_and_copy(0, 0, nullptr, nullptr, nullptr, nullptr, st);
  RM_HIP(hipMemsetAsync(s.ctr + kSActive, 0, sizeof(uint32_t), st));
  s.commit(nullptr, st);
  s.read_ctr(st);
  s.extent = s.hctr[kSTotal];
  const uint64_t V = s.nV, n = s.extent;
  if (cnt) RM_HIP(hipMemcpy(cnt, s.cnt, V * 4, hipMemcpyDeviceToHost));
  if (max_sep) RM_HIP(hipMemcpy(max_sep, s.max_sep, V * 4, hipMemcpyDeviceToHost));
  if (last_update) RM_HIP(hipMemcpy(last_update, s.last_update, V * 8, hipMemcpyDeviceToHost));
  const PtStore& b = s.buf[s.cur];
  if (n && lon) RM_HIP(hipMemcpy(lon, b.lon, n * 4, hipMemcpyDeviceToHost));
  if (n && lat) RM_HIP(hipMemcpy(lat, b.lat, n * 4, hipMemcpyDeviceToHost));
  if (n && time) RM_HIP(hipMemcpy(time, b.time, n * 8, hipMemcpyDeviceToHost));
  if (n && acc) RM_HIP(hipMemcpy(acc, b.acc, n * 4, hipMemcpyDeviceToHost));
  return n;
}

// ---- the stream snapshot's access (DESIGN.md §3 rule 15; snapshot.hip holds the kernels) ----
namespace {
__global__ void k_sess_live(uint32_t nV, const uint32_t* cnt, uint32_t* flag) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v <= nV) flag[v] = v < nV && cnt[v] > 0u ? 1u : 0u;   // (flag[nV] = 0: the scan's last entry is the total)
}
}  // namespace

hipStream_t Session::stream() const { return p_->m->stream_; }

SessionSnap Session::snapshot_pack() {
  Impl& s = *p_;
  Matcher& m = *s.m;
  RM_HIP(hipSetDevice(m.eng_->device()));
  hipStream_t st = m.stream_;
  m.sync();
  // get_store's pack, then the rank of every non-empty vehicle among them.  The error word is
  // the last call's (an overflow there has been thrown already): the pack sets no bit of it
  RM_HIP(hipMemsetAsync(s.ctr + kSErr, 0, sizeof(uint32_t), st));
  s.layout_and_copy(0, 0, nullptr, nullptr, nullptr, nullptr, st);
  RM_HIP(hipMemsetAsync(s.ctr + kSActive, 0, sizeof(uint32_t), st));
  s.commit(nullptr, st);
  hipLaunchKernelGGL(k_sess_live, dim3(grid(s.nV + 1ull)), dim3(256), 0, st, s.nV, (const uint32_t*)s.cnt, s.tot);
  s.scr.scan<uint32_t>(s.tot, s.noff, s.nV + 1u, st);
  RM_HIP(hipMemcpyAsync(s.ctr + kSActive, s.noff + s.nV, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  RM_HIP(hipGetLastError());
  s.read_ctr(st);
  s.extent = s.hctr[kSTotal];
  return snap_view(s.extent, s.hctr[kSActive]);
}

SessionSnap Session::snapshot_room(uint64_t n_points) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.m->eng_->device()));
  if (n_points >= 0xffffffffull) throw BatchTooLarge("session store too large (points >= 2^32)");
  s.ensure_buf(s.buf[s.cur], n_points);   // (the session holds no points: nothing to keep)
  return snap_view(n_points, 0u);
}

void Session::snapshot_loaded(uint64_t n_points) {
  Impl& s = *p_;
  s.extent = n_points;
  s.n_win = s.n_rep = 0;   // the last call's outputs are not part of a snapshot
}

void Session::snapshot_sharded() { p_->sharded = true; }

void Session::snapshot_clear() {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.m->eng_->device()));
  hipStream_t st = s.m->stream_;
  const uint64_t V = s.nV;
  RM_HIP(hipMemsetAsync(s.off, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.cnt, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.max_sep, 0, V * 4, st));
  RM_HIP(hipMemsetAsync(s.last_update, 0, V * 8, st));
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(V)), dim3(256), 0, st, s.nV, s.scan_from, 1u);
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(V)), dim3(256), 0, st, s.nV, s.try_from, 1u);
  RM_HIP(hipGetLastError());
  RM_HIP(hipStreamSynchronize(st));
  s.extent = 0;
  s.n_win = s.n_rep = 0;
}

SessionSnap Session::snap_view(uint64_t n_points, uint32_t n_live) {
  Impl& s = *p_;
  SessionSnap v;
  v.n_vehicles = s.nV; v.n_live = n_live; v.n_points = n_points;
  v.off = s.off; v.cnt = s.cnt; v.scan_from = s.scan_from; v.try_from = s.try_from; v.max_sep = s.max_sep;
  v.last_update = s.last_update; v.rank = s.noff;
  const PtStore& b = s.buf[s.cur];
  v.lon = b.lon; v.lat = b.lat; v.acc = b.acc; v.time = b.time; v.arr = b.arr; v.veh = b.veh;
  v.stream = s.m->stream_;
  return v;
}

}  // namespace rm
