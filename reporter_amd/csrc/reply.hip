// reply.hip — the /report reply written on the device (DESIGN.md §3 rule 19; reference
// py/reporter_service.py:79-179, 240-243), from the segment, report and stats records a run left
// in HBM, and the host writer that gives the same bytes from host records.
//
//   items   a trace's reply is S + R + 3 pieces (reply_text.hpp rt_item): head, S segments,
//           middle, R reports, tail.  k_rp_count -> exclusive scan: the first item of every trace;
//           the host reads the total (4 bytes) and sizes the per-item arrays.
//   lengths k_rp_len: an item finds its trace in that scan (binary search), keeps it, and counts
//           its piece; a time outside the time routine's range flags the trace -> 64-bit exclusive
//           scan: the byte offset of every item; k_rp_offsets: of every reply.
//   write   k_rp_write: one wave per 64 consecutive items builds their contiguous span in LDS at
//           the blob offset's residue mod 16 and streams it out in aligned 16-byte stores, the
//           unaligned head and tail byte-wise (what tilestore.hip k_ts_write does).
//   one read of the offsets (the total sizes the blob), one download of the text into the reply
//   buffer, one of the flags.  A flagged trace is written again on the host from its records with
//   std::to_chars and spliced in: its bytes differ in length from the device's place-holder.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"
#include "host_pool.hpp"
#include "reply_text.hpp"
#include "trace_json.hpp"

namespace rm {

namespace {

constexpr uint64_t kRpMaxItems = 0x7ffffff0ull;   // (hipcub takes the item count as an int)

// trace k's records as the kernels read them: S segments at segs[seg_base[k]], R reports at
// reps[rep_base[k]]; lists that would leave the pools (cap records each) count as empty
struct RpSource {
  const uint32_t* seg_base;
  const uint32_t* seg_cnt;
  const uint32_t* rep_base;
  const SegmentRec* segs;
  const ReportRec* reps;
  const ReportStats* stats;
  unsigned long long cap;
};
__device__ __forceinline__ uint32_t rp_segments(const RpSource& s, uint32_t k) {
  const uint32_t n = s.seg_cnt[k];
  return (unsigned long long)s.seg_base[k] + n <= s.cap ? n : 0u;
}
__device__ __forceinline__ uint32_t rp_reports(const RpSource& s, uint32_t k, const ReportStats& st, uint32_t S) {
  const int32_t r = st.n_reports;
  if (r <= 0 || (unsigned long long)s.rep_base[k] + (uint32_t)r > s.cap) return 0u;
  return (uint32_t)r < S ? (uint32_t)r : S;   // (a trace reports at most its segments)
}

// items of trace k (cnt[T] = 0, so the scan's last entry is the total); counted and scanned in 64
// bits, so a total of 2^32 or more shows as such to the host, which refuses it before anything
// indexes by item
__global__ void k_rp_count(uint32_t T, RpSource s, unsigned long long* cnt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > T) return;
  if (k == T) { cnt[k] = 0ull; return; }
  const uint32_t S = rp_segments(s, k);
  cnt[k] = (unsigned long long)S + rp_reports(s, k, s.stats[k], S) + 3ull;
}

// item i of n = ioff[T] as the host read it (< 2^31): its trace (the last k with ioff[k] <= i; every
// trace has items) and its piece's bytes; len[n] = 0, so the scan's last entry is the total
__global__ void k_rp_len(uint32_t n, uint32_t T, const unsigned long long* ioff, RpSource s, uint32_t* item_trace,
                         unsigned long long* len, uint32_t* flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i >= n || i >= ioff[T]) { len[i] = 0ull; return; }
  uint32_t lo = 0, hi = T;   // ioff[lo] <= i < ioff[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (ioff[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t S = rp_segments(s, lo);
  const ReportStats st = s.stats[lo];
  RtCount c;
  rt_item(c, i - (uint32_t)ioff[lo], s.segs + s.seg_base[lo], S, s.reps + s.rep_base[lo], rp_reports(s, lo, st, S), st);
  item_trace[i] = lo;
  len[i] = c.n;
  if (c.other) flag[lo] = 1u;
}

// reply k starts where its first item does; roff[T] is the total (off[n])
__global__ void k_rp_offsets(uint32_t n, uint32_t T, const unsigned long long* ioff, const unsigned long long* off,
                             unsigned long long* roff) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k <= T) roff[k] = off[ioff[k] < n ? ioff[k] : n];
}

constexpr uint32_t kRpSpan = 64u * kRtMaxPiece + 16u;
static_assert(kRpSpan <= 65536u, "the span of one wave fits the LDS of a work-group");

// One wave per block, one item per lane: see k_ts_write.  off has the entry behind the last item.
__global__ void __launch_bounds__(64) k_rp_write(uint32_t n, const unsigned long long* ioff, RpSource s, const uint32_t* item_trace,
                                                 const unsigned long long* off, char* blob, unsigned long long total) {
  __shared__ __attribute__((aligned(16))) char sh[kRpSpan];
  const uint32_t lane = threadIdx.x;
  const uint32_t I = n;
  const uint32_t k0 = blockIdx.x * 64u;
  if (k0 >= I) return;
  const uint32_t kend = k0 + 64u < I ? k0 + 64u : I;
  const unsigned long long base = off[k0];
  unsigned long long end = off[kend];
  if (end > total) end = total;
  if (end < base || end - base > (unsigned long long)(kRpSpan - 16u)) return;   // (cannot happen: every piece <= kRtMaxPiece)
  const uint32_t shift = (uint32_t)(base & 15ull);
  const uint32_t k = k0 + lane;
  if (k < kend) {
    const unsigned long long o = off[k] - base, l = off[k + 1] - off[k];
    if (o + l <= end - base) {
      const uint32_t t = item_trace[k];
      const uint32_t S = rp_segments(s, t);
      const ReportStats st = s.stats[t];
      RtWrite w{sh + shift + (uint32_t)o};
      rt_item(w, k - (uint32_t)ioff[t], s.segs + s.seg_base[t], S, s.reps + s.rep_base[t], rp_reports(s, t, st, S), st);
    }
  }
  __syncthreads();
  const unsigned long long a0 = (base + 15ull) & ~15ull;   // first aligned position of the blob in the span
  if (a0 >= end) {                                         // the whole span lies inside one 16-byte line
    if (base + lane < end) blob[base + lane] = sh[shift + lane];
    return;
  }
  const unsigned long long a1 = end & ~15ull;
  if (base + lane < a0) blob[base + lane] = sh[shift + lane];                                      // head (< 16)
  for (unsigned long long g = a0 + 16ull * lane; g < a1; g += 16ull * 64ull)
    *(uint4*)(blob + g) = *(const uint4*)(sh + shift + (uint32_t)(g - base));
  if (a1 + lane < end) blob[a1 + lane] = sh[shift + (uint32_t)(a1 - base) + lane];                 // tail (< 16)
}

// the pieces against a string, times as tj::put_num writes them: a flagged trace's reply
struct RtString {
  std::string& o;
  bool other = false;
  template <uint32_t N> void lit(const char (&s)[N]) { o.append(s, N - 1u); }
  void u64(uint64_t v) { tj::put_u64(o, v); }
  void i64(int64_t v) { tj::put_i64(o, v); }
  void km(int32_t m) {
    char b[16];
    o.append(b, rt_put_km(b, m));
  }
  void time(double x) { tj::put_num(o, x); }
};

void reply_exact(const SegmentRec* segs, uint32_t S, const ReportRec* reps, uint32_t R, const ReportStats& st, std::string& o) {
  o.clear();
  RtString s{o};
  for (uint32_t j = 0; j < S + R + 3u; ++j) rt_item(s, j, segs, S, reps, R, st);
}

}  // namespace

uint64_t reply_device_min_points() {
  const char* e = std::getenv("RM_REPLY_DEVICE_MIN_POINTS");
  if (!e || !*e) return 65536;   // Matcher::run's small-run limit (RM_SMALL_BATCH_POINTS)
  const double v = std::strtod(e, nullptr);
  if (!(v > 0.0)) return 0;
  return v >= 1.8e19 ? ~0ull : (uint64_t)v;
}

void reply_format_host(uint32_t T, const uint32_t* seg_off, const SegmentRec* segs, const uint32_t* rep_base,
                       const uint32_t* rep_cnt, const ReportRec* reps, const ReportStats* stats, char** buf, uint64_t* off,
                       uint64_t* flagged) {
  for (uint32_t k = 0; k < T; ++k)
    if (seg_off[k + 1] < seg_off[k]) throw std::runtime_error("segment offsets not monotone");
  HostPool& pool = HostPool::get();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(pool.size(), ((size_t)T + 63) / 64));
  std::vector<uint64_t> len(T);
  std::vector<std::string> exact(T);   // the flagged traces' replies
  std::vector<uint8_t> flag(T, 0);
  auto trace = [&](size_t k, auto& sink) {
    const uint32_t S = seg_off[k + 1] - seg_off[k], R = rep_cnt[k];
    for (uint32_t j = 0; j < S + R + 3u; ++j) rt_item(sink, j, segs + seg_off[k], S, reps + rep_base[k], R, stats[k]);
  };
  pool.run(nt, [&](size_t t) {
    for (size_t k = (size_t)T * t / nt; k < (size_t)T * (t + 1) / nt; ++k) {
      RtCount c;
      trace(k, c);
      len[k] = c.n;
      if (c.other) {
        flag[k] = 1;
        reply_exact(segs + seg_off[k], seg_off[k + 1] - seg_off[k], reps + rep_base[k], rep_cnt[k], stats[k], exact[k]);
        len[k] = exact[k].size();
      }
    }
  });
  off[0] = 0;
  uint64_t nf = 0;
  for (uint32_t k = 0; k < T; ++k) { off[k + 1] = off[k] + len[k]; nf += flag[k]; }
  char* out = static_cast<char*>(std::malloc(off[T] + 1));
  if (!out) throw std::bad_alloc();
  pool.run(nt, [&](size_t t) {
    for (size_t k = (size_t)T * t / nt; k < (size_t)T * (t + 1) / nt; ++k) {
      if (flag[k]) { std::memcpy(out + off[k], exact[k].data(), exact[k].size()); continue; }
      RtWrite w{out + off[k]};
      trace(k, w);
    }
  });
  out[off[T]] = 0;
  *buf = out;
  if (flagged) *flagged = nf;
}

void reply_format_one(const SegmentRec* segs, uint32_t S, const ReportRec* reps, uint32_t R, const ReportStats& st, std::string& o) {
  RtCount c;
  for (uint32_t j = 0; j < S + R + 3u; ++j) rt_item(c, j, segs, S, reps, R, st);
  if (c.other) { reply_exact(segs, S, reps, R, st, o); return; }
  o.resize(c.n);
  RtWrite w{&o[0]};
  for (uint32_t j = 0; j < S + R + 3u; ++j) rt_item(w, j, segs, S, reps, R, st);
}

void ReplyWriter::write(int device, hipStream_t st, const ReplySource& src, char** buf, uint64_t* off, uint64_t* flagged,
                        double* ms) {
  RM_HIP(hipSetDevice(device));
  const uint32_t T = src.T;
  if (ms) *ms = 0.0;
  if (flagged) *flagged = 0;
  off[0] = 0;
  if (T == 0) {
    char* e = static_cast<char*>(std::malloc(1));
    if (!e) throw std::bad_alloc();
    e[0] = 0;
    *buf = e;
    return;
  }
  static constexpr const char* kFull = "reply buffers do not fit in HBM";
  const RpSource s{src.seg_base, src.seg_cnt, src.rep_base, src.segs, src.reps, src.stats, (unsigned long long)src.cap};
  if ((uint64_t)T + 1 > t_cap_) {
    RM_HIP(hipStreamSynchronize(st));
    t_cap_ = 0;
    const uint64_t c = (uint64_t)T + T / 4 + 1024;
    cnt_.reserve(c, kFull); ioff_.reserve(c, kFull); flag_.reserve(c, kFull); roff_.reserve(c, kFull);
    t_cap_ = c;
  }
  if (!hn_) hn_.reserve(4);
  double part[1] = {0.0};
  timer_.tic(0, st);
  RM_HIP(hipMemsetAsync(flag_, 0, T * 4ull, st));
  hipLaunchKernelGGL(k_rp_count, dim3(grid((uint64_t)T + 1)), dim3(256), 0, st, T, s, cnt_.get());
  scr_.scan((const unsigned long long*)cnt_, ioff_.get(), (uint64_t)T + 1, st);
  timer_.toc(st);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(hn_, ioff_ + T, 8, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  const uint64_t n = hn_[0];
  if (n < 3ull * T) throw std::runtime_error("reply item count out of range");   // (every trace has three)
  if (n >= kRpMaxItems) throw BatchTooLarge("batch too large (reply items >= 2^31)");
  if (n + 1 > i_cap_) {
    i_cap_ = 0;
    const uint64_t c = n + n / 4 + 4096;
    item_trace_.reserve(c, kFull); len_.reserve(c, kFull); ofs_.reserve(c, kFull);
    i_cap_ = c;
  }
  timer_.tic(0, st);
  hipLaunchKernelGGL(k_rp_len, dim3(grid(n + 1)), dim3(256), 0, st, (uint32_t)n, T, (const unsigned long long*)ioff_, s, item_trace_.get(),
                     len_.get(), flag_.get());
  scr_.scan((const unsigned long long*)len_, ofs_.get(), n + 1, st);
  hipLaunchKernelGGL(k_rp_offsets, dim3(grid((uint64_t)T + 1)), dim3(256), 0, st, (uint32_t)n, T,
                     (const unsigned long long*)ioff_, (const unsigned long long*)ofs_, roff_.get());
  timer_.toc(st);
  RM_HIP(hipGetLastError());
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are 64-bit");
  RM_HIP(hipMemcpyAsync(off, roff_, (T + 1) * 8ull, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  const uint64_t bytes = off[T];
  if (bytes > n * (uint64_t)kRtMaxPiece) throw std::runtime_error("reply size out of range");
  if (bytes + 16 > blob_cap_) {
    blob_cap_ = 0;
    const uint64_t c = bytes + bytes / 4 + 4096;
    blob_.reserve(c, kFull);   // (hipMalloc: 256-byte aligned, so blob offsets mod 16 are addresses mod 16)
    blob_cap_ = c;
  }
  timer_.tic(0, st);
  hipLaunchKernelGGL(k_rp_write, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, st, (uint32_t)n,
                     (const unsigned long long*)ioff_, s, (const uint32_t*)item_trace_, (const unsigned long long*)ofs_, blob_.get(), (unsigned long long)bytes);
  timer_.toc(st);
  RM_HIP(hipGetLastError());
  std::vector<uint32_t> hflag(T);
  struct Free { void operator()(char* p) const { std::free(p); } };
  std::unique_ptr<char, Free> host(static_cast<char*>(std::malloc(bytes + 1)));
  if (!host) throw std::bad_alloc();
  RM_HIP(hipMemcpyAsync(host.get(), blob_, bytes, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(hflag.data(), flag_, T * 4ull, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  host.get()[bytes] = 0;
  timer_.harvest(part);
  if (ms) *ms = part[0];
  // ---- flagged traces (rare): written from their records and spliced in.  The per-trace words
  // come down whole, then every flagged trace's records, with one wait for each of the two.
  std::vector<uint32_t> bad;
  for (uint32_t k = 0; k < T; ++k)
    if (hflag[k]) bad.push_back(k);
  if (bad.empty()) { *buf = host.release(); return; }
  std::vector<uint32_t> sb(T), sc(T), rb(T);
  std::vector<ReportStats> hs(T);
  RM_HIP(hipMemcpyAsync(sb.data(), src.seg_base, T * 4ull, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(sc.data(), src.seg_cnt, T * 4ull, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(rb.data(), src.rep_base, T * 4ull, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(hs.data(), src.stats, T * sizeof(ReportStats), hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  std::vector<std::vector<SegmentRec>> hsegs(bad.size());
  std::vector<std::vector<ReportRec>> hreps(bad.size());
  for (size_t b = 0; b < bad.size(); ++b) {
    const uint32_t k = bad[b];
    const uint32_t S = (uint64_t)sb[k] + sc[k] <= src.cap ? sc[k] : 0u;
    const int32_t r = hs[k].n_reports;
    const uint32_t R = r <= 0 || (uint64_t)rb[k] + (uint32_t)r > src.cap ? 0u : std::min<uint32_t>((uint32_t)r, S);
    hsegs[b].resize(S);
    hreps[b].resize(R);
    if (S) RM_HIP(hipMemcpyAsync(hsegs[b].data(), src.segs + sb[k], S * sizeof(SegmentRec), hipMemcpyDeviceToHost, st));
    if (R) RM_HIP(hipMemcpyAsync(hreps[b].data(), src.reps + rb[k], R * sizeof(ReportRec), hipMemcpyDeviceToHost, st));
  }
  RM_HIP(hipStreamSynchronize(st));
  std::vector<std::string> exact(bad.size());
  uint64_t grow = 0;
  for (size_t b = 0; b < bad.size(); ++b) {
    reply_exact(hsegs[b].data(), (uint32_t)hsegs[b].size(), hreps[b].data(), (uint32_t)hreps[b].size(), hs[bad[b]], exact[b]);
    grow += exact[b].size();
  }
  std::unique_ptr<char, Free> out(static_cast<char*>(std::malloc(bytes + grow + 1)));
  if (!out) throw std::bad_alloc();
  std::vector<uint64_t> noff(T + 1);
  uint64_t at = 0;
  size_t b = 0;
  for (uint32_t k = 0; k < T; ++k) {
    noff[k] = at;
    if (b < bad.size() && bad[b] == k) {
      std::memcpy(out.get() + at, exact[b].data(), exact[b].size());
      at += exact[b++].size();
    } else {
      std::memcpy(out.get() + at, host.get() + off[k], off[k + 1] - off[k]);
      at += off[k + 1] - off[k];
    }
  }
  noff[T] = at;
  out.get()[at] = 0;
  std::memcpy(off, noff.data(), (T + 1) * 8ull);
  *buf = out.release();
  if (flagged) *flagged = bad.size();
}

}  // namespace rm
