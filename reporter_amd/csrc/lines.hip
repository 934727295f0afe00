// lines.hip — the ingest stage of the batch pipeline on the device (DESIGN.md §3 rule 11): the text
// of trace files (reference py/simple_reporter.py:100-113, :137-140; Formatter.java:97-109) becomes
// the point arrays rm_runner_run_points starts from, with no interpreted loop per point.
//
//   upload      the chunks (one per file) laid end to end in one byte buffer, a '\n' inserted after
//               a chunk that lacks one, 16 bytes of '\n' in front (byte 0 is a line start like any
//               other) and zeros behind (a window may read past the end)
//   k_line_count / scan   line starts per 4096-byte window -> each window's first line index
//   k_line_parse          one wave per window: the window and the 256 bytes its lines can reach
//               staged in LDS with 16-byte loads, ballots over consecutive 64-byte chunks list the
//               line starts in order, lane j reads line j by sv::compact_line, 64 lines a round
//   host lines  lines outside the compact layout are read by sv::generic_line on the host pool
//               and patched into their slots; the first malformed line in input order fails the call
//   compaction  k_line_stats flags the points (and counts the blank, outside and host lines, so the
//               statuses come back only when there are host lines); scan over "is a point" -> the
//               kept points in input order in StageBufs
//   ids         stable sort of (hash, point), group starts + byte compare of neighbours, scan,
//               sort of the groups by their first point -> first-seen rank per point (dense_ids'
//               order); a hash collision sends the numbering to the host (same result)
// Every output position comes from a scan or a stable sort: no atomics, the same result each call.
//
// Stream messages (rule 14) take the same road: parse_messages reads either kind of msg::Format --
// k_line_parse<1> calls msg::compact_json for JSON lines, the host's generic reader is
// msg::generic_message -- and a tolerant call drops malformed lines (patched to "bad": no point),
// counts them and lists the first 64.  The directory (directory.hip) then turns the per-call vehicle
// numbers left here into indices that hold for the whole stream.
//
// Date patterns (rule 18): a time_format from 16 up is the id of a pattern registered in this
// process (time_pattern_register below).  time_pattern_of resolves it, once per call; the program
// goes to k_line_parse<KIND, true> by value and to the host's generic readers by pointer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <string_view>
#include <unordered_map>

#include "engine.hpp"
#include "host_pool.hpp"
#include "inflate.hpp"
#include "inflate_core.hpp"

namespace rm {

namespace {

constexpr uint32_t kLineWin = 4096;                               // bytes of text per wave
constexpr uint32_t kLineFront = 16;                               // '\n' bytes in front of the text
constexpr uint32_t kLineLds = kLineFront + kLineWin + sv::kMaxLine;   // a window's bytes in LDS
constexpr uint64_t kLineTail = kLineWin + kLineLds;               // zero bytes kept behind the text
constexpr uint32_t kLineRing = 128;                               // line starts listed ahead of a round
constexpr size_t kMaxDropped = 64;                                // dropped messages a tolerant call lists
static_assert(kLineLds % 16 == 0, "windows are staged with 16-byte loads");

// bytes of w equal to '\n'
__device__ __forceinline__ uint32_t newlines(uint32_t w) {
  const uint32_t x = w ^ 0x0a0a0a0au;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return (uint32_t)__popc(~(t | x | 0x7f7f7f7fu));
}

// line starts in window w: text positions p in [w * kLineWin, (w + 1) * kLineWin), p < N, whose
// previous byte is '\n'.  Counted as the '\n' of the window's bytes, shifted by one at either end.
__global__ void __launch_bounds__(64) k_line_count(const uint8_t* buf, uint64_t N, uint32_t* cnt) {
  const uint64_t a = (uint64_t)blockIdx.x * kLineWin;
  const uint4* src = reinterpret_cast<const uint4*>(buf + kLineFront + a);
  uint32_t n = 0;
  for (uint32_t r = 0; r < kLineWin / 16 / 64; ++r) {
    const uint4 v = src[r * 64 + threadIdx.x];
    n += newlines(v.x) + newlines(v.y) + newlines(v.z) + newlines(v.w);
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if (threadIdx.x == 0) {
    n += buf[kLineFront + a - 1] == '\n';
    n -= buf[kLineFront + a + kLineWin - 1] == '\n';
    if (N >= a && N < a + kLineWin) --n;   // the text's last '\n' starts no line
    cnt[blockIdx.x] = n;
  }
}

struct LineArrays {   // one entry per line
  uint8_t* status;
  float* lat;
  float* lon;
  float* acc;
  double* time;
  uint32_t* id_off;   // the id's offset in the text; of a host line: the line's
  uint32_t* id_len;
  unsigned long long* hash;
};

// KIND 0: separated values (rule 11); KIND 1: JSON messages (rule 14), whose five keys arrive by
// value in `keys` (KIND 0 takes an empty struct there: its code and arguments are what they were)
struct NoKeys {};
// PAT: the time is read by a date pattern (rule 18), whose program arrives by value in `prog`; it
// is wave-uniform, so the step loop of tp::match branches on scalars.  Without one `prog` is an
// empty struct behind the other arguments, which stay where they were.
struct NoProgram {};
template <int KIND, bool PAT>
__global__ void __launch_bounds__(64) k_line_parse(const uint8_t* buf, uint64_t N, const uint32_t* first,
                                                   const uint32_t* cnt, uint32_t L, sv::Format fmt,
                                                   std::conditional_t<KIND == 1, msg::Keys, NoKeys> keys, LineArrays o,
                                                   uint32_t* err, std::conditional_t<PAT, tp::Program, NoProgram> prog) {
  __shared__ uint4 win4[kLineLds / 16];
  __shared__ uint16_t starts[kLineRing];
  const uint8_t* win = reinterpret_cast<const uint8_t*>(win4);   // win[i]: text position a - kLineFront + i
  const uint32_t lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint64_t a = (uint64_t)blockIdx.x * kLineWin;
  for (uint32_t x = lane; x < kLineLds / 16; x += 64) win4[x] = reinterpret_cast<const uint4*>(buf + a)[x];
  __syncthreads();
  const uint32_t lim = N - a < (uint64_t)kLineWin ? (uint32_t)(N - a) : kLineWin;
  const uint32_t base = first[blockIdx.x];
  uint32_t head = 0, tail = 0;
  auto round = [&](uint32_t nr) {   // lines head .. head + nr of the window, one per lane
    __syncthreads();
    const uint32_t k = base + head + lane;
    if (lane < nr && k < L) {   // k < L always, unless the two kernels disagree (err below)
      const uint32_t pos = starts[(head + lane) & (kLineRing - 1)];
      sv::Line ln;
      uint32_t st;
      const tp::Program* pp = nullptr;
      if constexpr (PAT) pp = &prog;
      if constexpr (KIND == 1) st = msg::compact_json(win + kLineFront + pos, fmt, keys, ln, pp);
      else st = sv::compact_line(win + kLineFront + pos, fmt, ln, pp);
      o.status[k] = (uint8_t)st;
      if (st == sv::kPoint) {
        o.lat[k] = ln.lat;
        o.lon[k] = ln.lon;
        o.acc[k] = ln.acc;
        o.time[k] = ln.time;
        o.id_off[k] = (uint32_t)a + pos + ln.id_off;
        o.id_len[k] = ln.id_len;
        o.hash[k] = ln.hash;
      } else if (st == sv::kHost) {
        o.id_off[k] = (uint32_t)a + pos;
      }
    }
    head += nr;
  };
  for (uint32_t c0 = 0; c0 < lim; c0 += 64) {
    const uint32_t pos = c0 + lane;
    const bool open = pos < lim && win[kLineFront + pos - 1] == '\n';
    const unsigned long long m = __ballot(open);
    if (open) starts[(tail + (uint32_t)__popcll(m & below)) & (kLineRing - 1)] = (uint16_t)pos;
    tail += (uint32_t)__popcll(m);
    if (tail - head >= 64u) round(64u);
  }
  if (tail > head) round(tail - head);
  if (lane == 0 && tail != cnt[blockIdx.x]) err[0] = 1u;   // the two kernels disagree: the host throws
}

struct LinePatch {   // the host lines' results, one entry per host line
  const uint32_t* line;
  const uint8_t* status;
  const float* lat;
  const float* lon;
  const float* acc;
  const double* time;
  const uint32_t* id_off;
  const uint32_t* id_len;
  const unsigned long long* hash;
};

__global__ void k_line_patch(uint32_t n, LinePatch p, LineArrays o) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = p.line[i];
  o.status[k] = p.status[i];
  o.lat[k] = p.lat[i];
  o.lon[k] = p.lon[i];
  o.acc[k] = p.acc[i];
  o.time[k] = p.time[i];
  o.id_off[k] = p.id_off[i];
  o.id_len[k] = p.id_len[i];
  o.hash[k] = p.hash[i];
}

// "is a point" per line for the compaction scan, and per block the blank, outside and host lines
// (the host folds the at most 1024 triples)
__global__ void __launch_bounds__(256) k_line_stats(uint64_t L, const uint8_t* status, uint32_t* flag, uint32_t* part) {
  __shared__ uint32_t acc[4][3];
  uint32_t nb = 0, no = 0, nh = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < L; k += (uint64_t)gridDim.x * 256) {
    const uint32_t st = status[k];
    flag[k] = st == sv::kPoint ? 1u : 0u;
    nb += st == sv::kBlank;
    no += st == sv::kOutside;
    nh += st == sv::kHost;
  }
  for (int o = 32; o > 0; o >>= 1) { nb += __shfl_xor(nb, o); no += __shfl_xor(no, o); nh += __shfl_xor(nh, o); }
  if ((threadIdx.x & 63) == 0) { acc[threadIdx.x >> 6][0] = nb; acc[threadIdx.x >> 6][1] = no; acc[threadIdx.x >> 6][2] = nh; }
  __syncthreads();
  if (threadIdx.x < 3) part[3 * blockIdx.x + threadIdx.x] = acc[0][threadIdx.x] + acc[1][threadIdx.x] + acc[2][threadIdx.x] + acc[3][threadIdx.x];
}

// the kept points in input order: the point arrays, the id spans, the sort's (hash, point) pairs
__global__ void k_line_compact(uint64_t L, LineArrays o, const uint32_t* flag, const uint32_t* pos, unsigned long long mask,
                               double* p_time, float* p_lon, float* p_lat, float* p_acc, uint32_t* p_off, uint32_t* p_len,
                               unsigned long long* key, uint32_t* val) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= L || !flag[k]) return;
  const uint32_t d = pos[k];
  p_time[d] = o.time[k];
  p_lon[d] = o.lon[k];
  p_lat[d] = o.lat[k];
  p_acc[d] = o.acc[k];
  p_off[d] = o.id_off[k];
  p_len[d] = o.id_len[k];
  key[d] = o.hash[k] & mask;
  val[d] = d;
}

// sorted by hash (stable: by point within a hash): a group starts where the hash changes; inside
// a group every point's id bytes must equal its neighbour's, else two ids share the hash
__global__ void k_id_flags(uint64_t P, const unsigned long long* key, const uint32_t* pt, const uint32_t* p_off,
                           const uint32_t* p_len, const uint8_t* text, uint32_t* flag, uint32_t* collide) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  uint32_t f = 1;
  if (k > 0 && key[k] == key[k - 1]) {
    f = 0;
    const uint32_t x = pt[k], y = pt[k - 1], n = p_len[x];
    bool same = n == p_len[y];
    const uint8_t* sx = text + p_off[x];
    const uint8_t* sy = text + p_off[y];
    for (uint32_t i = 0; same && i < n; ++i) same = sx[i] == sy[i];
    if (!same) collide[0] = 1u;
  }
  flag[k] = f;
}

// group g's first point (the sort is stable, so it is the smallest), and each point's group
__global__ void k_id_groups(uint64_t P, const uint32_t* flag, const uint32_t* gidx, const uint32_t* pt,
                            unsigned long long* gfirst, uint32_t* gval, uint32_t* p_group, uint32_t* hctl) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  const uint32_t g = gidx[k] + flag[k] - 1u;
  p_group[pt[k]] = g;
  if (flag[k]) { gfirst[g] = pt[k]; gval[g] = g; }
  if (k + 1 == P) hctl[0] = g + 1u;
}

// groups sorted by first point: rank r is vehicle r, named by that point's id span
__global__ void k_id_rank(uint32_t G, const unsigned long long* gfirst, const uint32_t* gval, const uint32_t* p_off,
                          const uint32_t* p_len, uint32_t* rank, uint32_t* v_off, uint32_t* v_len) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= G) return;
  const uint32_t p = (uint32_t)gfirst[r];
  rank[gval[r]] = r;
  v_off[r] = p_off[p];
  v_len[r] = p_len[p];
}

__global__ void k_id_scatter(uint64_t P, const uint32_t* p_group, const uint32_t* rank, uint32_t* p_uuid) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < P) p_uuid[k] = rank[p_group[k]];
}

// per block the smallest and largest time; the host folds the (at most 1024) pairs
__global__ void __launch_bounds__(256) k_time_span(uint64_t P, const double* time, double* part) {
  __shared__ double lo[4], hi[4];
  double a = time[0], b = a;
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < P; k += (uint64_t)gridDim.x * 256) {
    const double t = time[k];
    a = t < a ? t : a;
    b = t > b ? t : b;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double x = __shfl_xor(a, o), y = __shfl_xor(b, o);
    a = x < a ? x : a;
    b = y > b ? y : b;
  }
  if ((threadIdx.x & 63) == 0) { lo[threadIdx.x >> 6] = a; hi[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { a = lo[w] < a ? lo[w] : a; b = hi[w] > b ? hi[w] : b; }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = b;
  }
}

// room for n elements, grow-only, by a quarter and 256 bytes; the old block may still be in
// flight on the stream
template <class T>
void need(DevBuf<T>& b, uint64_t n, hipStream_t st) {
  if (n <= b.cap() && b) return;
  if (b) RM_HIP(hipStreamSynchronize(st));
  const uint64_t bytes = n * sizeof(T);
  b.reserve((bytes + bytes / 4 + 256 + sizeof(T) - 1) / sizeof(T));
}

unsigned long long hash_mask() {   // RM_LINES_HASH_BITS (1-64, default 64), read at every call
  long bits = 64;
  if (const char* e = std::getenv("RM_LINES_HASH_BITS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v >= 1 && v <= 64) bits = v;
  }
  return bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
}

struct HostLine {
  uint32_t line = 0, status = 0;
  sv::Line v{};
  const char* why = nullptr;
};

// the process's date patterns: entries are written once, under the lock, and never move
struct PatternTable {
  std::mutex mu;
  int32_t n = 0;
  tp::Pattern at[tp::kMaxPatterns];
};
PatternTable& patterns() {
  static PatternTable t;
  return t;
}

// the one place a format's time_format becomes a program: null for 0, 1 and ids nobody registered
// (format_error then says so)
const tp::Pattern* time_pattern_of(const sv::Format& f) { return time_pattern_find(f.time_format); }

}  // namespace

unsigned long long lines_hash_mask() { return hash_mask(); }

int32_t time_pattern_register(const char* pattern, std::string& err) {
  if (!pattern) { err = "the pattern is NULL"; return -1; }
  tp::Pattern p;
  if (!tp::compile(pattern, p, err)) return -1;
  PatternTable& t = patterns();
  std::lock_guard<std::mutex> lock(t.mu);
  for (int32_t i = 0; i < t.n; ++i)
    if (!std::strcmp(t.at[i].text, p.text)) return tp::kFirstId + i;
  if (t.n == tp::kMaxPatterns) { err = "a process registers at most 240 time patterns"; return -1; }
  t.at[t.n] = p;
  return tp::kFirstId + t.n++;
}

const tp::Pattern* time_pattern_find(int32_t id) {
  PatternTable& t = patterns();
  std::lock_guard<std::mutex> lock(t.mu);
  return id >= tp::kFirstId && id - tp::kFirstId < t.n ? &t.at[id - tp::kFirstId] : nullptr;
}

struct LineState {
  DevBuf<uint8_t> text, status, patch;
  DevBuf<uint32_t> wcnt, wfirst, id_off, id_len, flag, pos, p_off, p_len, v_off, v_len, stats, derr;
  DevBuf<float> lat, lon, acc;
  DevBuf<double> time, part;
  DevBuf<unsigned long long> hash;
  ScanScratch scr;
  PartTimer timer;            // parts: ms[0 .. 3]
  PinBuf<uint32_t> hctl;      // pinned read-back words
  // the last call
  std::vector<uint64_t> chunk_base;   // n_chunks + 1: where each chunk starts in the text
  std::vector<uint32_t> veh_off, veh_len;
  uint64_t info[7] = {0, 0, 0, 0, 0, 0, 0};
  uint64_t n_dropped = 0;                 // malformed lines of a tolerant call
  std::vector<DroppedMessage> dropped;    // the first 64 of them, in input order
  uint32_t n_groups = 0;                  // v_off / v_len entries on the device
  uint64_t n_points = 0;
  double tmin = 0.0, tmax = 0.0;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  bool parsed = false;
  // rule 20: the last call's gzip chunks
  InflateJob job;
  PartTimer gz_timer;                      // parts: gz_ms[0 .. 2]
  std::vector<uint32_t> gz_status;         // per chunk
  std::vector<std::vector<uint8_t>> gz_host;   // a chunk's inflated bytes where the host has them
  uint64_t gz_info[6] = {0, 0, 0, 0, 0, 0};
  double gz_ms[3] = {0.0, 0.0, 0.0};
  // the chunk holding text position `at`
  uint32_t chunk_of(uint64_t at) const {
    return (uint32_t)(std::upper_bound(chunk_base.begin(), chunk_base.end() - 1, at) - chunk_base.begin()) - 1u;
  }
};

void Matcher::parse_lines(const LinesDesc& d) {
  if (ls_) ls_->parsed = false;
  if (d.n_chunks && (!d.data || !d.len)) throw std::runtime_error("line chunks are NULL");
  const tp::Pattern* pat = time_pattern_of(d.fmt);
  if (const char* e = sv::format_error(d.fmt, pat ? &pat->prog : nullptr); *e) throw std::runtime_error(std::string("line format: ") + e);
  MessagesDesc md;
  md.n_chunks = d.n_chunks; md.data = d.data; md.len = d.len;
  std::memset(&md.fmt, 0, sizeof md.fmt);
  md.fmt.line = d.fmt;
  md.strict = 1;
  parse_text(md, pat);
}

void Matcher::parse_messages(const MessagesDesc& d) {
  if (ls_) ls_->parsed = false;
  if (d.n_chunks && (!d.data || !d.len)) throw std::runtime_error("message chunks are NULL");
  const tp::Pattern* pat = time_pattern_of(d.fmt.line);
  if (const char* e = msg::format_error(d.fmt, pat ? &pat->prog : nullptr); *e) throw std::runtime_error(std::string("message format: ") + e);
  parse_text(d, pat);
}

// rule 11 (d.fmt.kind 0) and rule 14 over the chunks: the kept points in StageBufs, numbered per call
void Matcher::parse_text(const MessagesDesc& d, const tp::Pattern* pat) {
  RM_HIP(hipSetDevice(eng_->device()));
  if (!ls_) ls_ = std::make_shared<LineState>();
  LineState& z = *ls_;
  z.parsed = false;
  z.n_dropped = 0;
  z.dropped.clear();
  z.n_groups = 0;
  hipStream_t st = stream_;
  if (!z.hctl) z.hctl.reserve(16);
  z.timer.harvest(nullptr);   // (pairs a call that threw left behind)
  // ---- the text: chunks end to end, each ending in '\n'
  z.chunk_base.assign(d.n_chunks + 1ull, 0);
  for (uint32_t c = 0; c < d.n_chunks; ++c)
    if (d.len[c] && !d.data[c]) throw std::runtime_error("line chunk is NULL");
  // ---- rule 20: gzip chunks inflated, on the device (their bytes stay there: src null) or, for a
  // call of few, on the host pool (then they are plain chunks from here on)
  std::vector<const char*> src(d.data, d.data + d.n_chunks);
  std::vector<uint64_t> slen(d.len, d.len + d.n_chunks);
  std::vector<uint8_t> on_dev(d.n_chunks, 0), ends_nl(d.n_chunks, 0);
  z.gz_status.assign(d.n_chunks, 0);
  z.gz_host.clear();
  z.gz_host.resize(d.n_chunks);
  std::fill(z.gz_info, z.gz_info + 6, 0);
  std::fill(z.gz_ms, z.gz_ms + 3, 0.0);
  z.gz_timer.harvest(nullptr);
  uint32_t n_gz = 0;
  if (input_coding_)
    for (uint32_t c = 0; c < d.n_chunks; ++c) {
      const bool magic = d.len[c] >= 2 && (uint8_t)d.data[c][0] == 0x1f && (uint8_t)d.data[c][1] == 0x8b;
      on_dev[c] = input_coding_ == 1 || magic;
      n_gz += on_dev[c];
    }
  const std::vector<uint8_t> is_gz(on_dev);
  if (n_gz) {
    uint64_t members = 0;
    if (n_gz < inflate_device_min_chunks()) {
      std::vector<const char*> gd;
      std::vector<uint64_t> gl;
      std::vector<uint32_t> which;
      for (uint32_t c = 0; c < d.n_chunks; ++c)
        if (on_dev[c]) { gd.push_back(d.data[c]); gl.push_back(d.len[c]); which.push_back(c); on_dev[c] = 0; }
      InflateResult r;
      inflate_host(n_gz, gd.data(), gl.data(), r);
      for (uint32_t k = 0; k < n_gz; ++k) {
        const uint32_t c = which[k];
        z.gz_status[c] = r.status[k];
        z.gz_host[c].assign(r.blob.begin() + (ptrdiff_t)r.off[k], r.blob.begin() + (ptrdiff_t)r.off[k + 1]);
        src[c] = (const char*)z.gz_host[c].data();
        slen[c] = z.gz_host[c].size();
        members += r.members[k];
        z.gz_info[2] += d.len[c];
      }
      z.gz_info[5] = n_gz;
    } else {
      z.job.run(d.n_chunks, d.data, d.len, on_dev.data(), st, z.gz_timer);
      for (uint32_t c = 0; c < d.n_chunks; ++c) {
        if (!on_dev[c]) continue;
        z.gz_status[c] = z.job.res[c].status;
        src[c] = nullptr;
        slen[c] = z.job.res[c].status == inf::kOk ? z.job.res[c].count : 0;
        ends_nl[c] = z.job.res[c].last == (uint32_t)'\n';
        members += z.job.res[c].members;
      }
      z.gz_info[2] = z.job.bytes_in;
      z.gz_info[4] = z.job.second_pass;
    }
    z.gz_info[0] = n_gz;
    z.gz_info[1] = members;
    for (uint32_t c = 0; c < d.n_chunks; ++c) {
      if (z.gz_status[c] == inf::kOk) continue;
      if (!skip_bad_chunks_)
        throw std::runtime_error("chunk " + std::to_string(c + 1) + ": gzip: " + inf::status_text(z.gz_status[c]));
      slen[c] = 0;   // (a skipped chunk counts as empty)
    }
  }
  for (uint32_t c = 0; c < d.n_chunks; ++c)
    if (!on_dev[c]) ends_nl[c] = slen[c] && src[c][slen[c] - 1] == '\n';
  uint64_t N = 0;
  for (uint32_t c = 0; c < d.n_chunks; ++c) {
    z.chunk_base[c] = N;
    N += slen[c];
    if (slen[c] && !ends_nl[c]) ++N;
    if (N >= (1ull << 32)) {
      if (n_gz) throw std::runtime_error(std::string("gzip: ") + inf::status_text(inf::kTooLarge) + " (the chunks of one call must stay under 2^32 bytes)");
      throw std::runtime_error("line input too large (the chunks of one call must stay under 2^32 bytes)");
    }
  }
  for (uint32_t c = 0; c < d.n_chunks; ++c)
    if (is_gz[c]) z.gz_info[3] += slen[c];
  z.chunk_base[d.n_chunks] = N;
  std::fill(z.info, z.info + 7, 0);
  z.veh_off.clear();
  z.veh_len.clear();
  z.n_points = 0;
  std::fill(z.ms, z.ms + 4, 0.0);
  if (N == 0) { z.parsed = true; return; }
  z.timer.tic(0, st);
  need(z.text, kLineFront + N + kLineTail, st);
  uint8_t* text = z.text;
  RM_HIP(hipMemsetAsync(text, '\n', kLineFront, st));
  RM_HIP(hipMemsetAsync(text + kLineFront + N, 0, kLineTail, st));
  std::vector<GatherItem> gather;
  for (uint32_t c = 0; c < d.n_chunks; ++c) {
    if (!slen[c]) continue;
    uint8_t* at = text + kLineFront + z.chunk_base[c];
    if (on_dev[c]) { gather.push_back(GatherItem{z.job.item[c].out, slen[c], kLineFront + z.chunk_base[c], ends_nl[c] ? 0u : 1u, 0}); continue; }
    RM_HIP(hipMemcpyAsync(at, src[c], slen[c], hipMemcpyHostToDevice, st));
    if (!ends_nl[c]) RM_HIP(hipMemsetAsync(at + slen[c], '\n', 1, st));
  }
  z.timer.toc(st);
  double gz_upload = 0.0;
  if (n_gz) {   // (the chunks inflated on the device: one copy puts them where plain chunks are uploaded to)
    z.job.gather(gather, text, st, z.gz_timer);
    double gm[4] = {0.0, 0.0, 0.0, 0.0};
    z.gz_timer.harvest(gm);
    std::copy(gm, gm + 3, z.gz_ms);
    gz_upload = gm[3];
  }
  // a chunk's bytes on the host: the caller's, or fetched from the device text (before any use from the pool)
  auto host_chunk = [&](uint32_t c) -> const char* {
    if (!src[c] && slen[c]) {
      z.gz_host[c].resize(slen[c]);
      RM_HIP(hipMemcpy(z.gz_host[c].data(), text + kLineFront + z.chunk_base[c], slen[c], hipMemcpyDeviceToHost));
      src[c] = (const char*)z.gz_host[c].data();
    }
    return src[c];
  };
  z.timer.tic(1, st);
  // ---- lines per window, each window's first line
  const uint32_t nwin = (uint32_t)((N + kLineWin - 1) / kLineWin);
  need(z.wcnt, nwin, st);
  need(z.wfirst, nwin, st);
  need(z.derr, 2, st);
  RM_HIP(hipMemsetAsync(z.derr, 0, 8, st));
  hipLaunchKernelGGL(k_line_count, dim3(nwin), dim3(64), 0, st, text, N, z.wcnt);
  z.scr.scan<uint32_t>(z.wcnt, z.wfirst, nwin, st);
  RM_HIP(hipMemcpyAsync(z.hctl + 0, z.wfirst + (nwin - 1), 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(z.hctl + 1, z.wcnt + (nwin - 1), 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  const uint64_t L = (uint64_t)z.hctl[0] + z.hctl[1];
  if (L == 0 || L >= 0x7fffffffull) throw std::runtime_error("line input: line count out of range");
  // ---- every line read
  need(z.status, L, st); need(z.lat, L, st); need(z.lon, L, st); need(z.acc, L, st); need(z.time, L, st);
  need(z.id_off, L, st); need(z.id_len, L, st); need(z.hash, L, st); need(z.flag, L, st); need(z.pos, L, st);
  LineArrays la{z.status, z.lat, z.lon, z.acc, z.time, z.id_off, z.id_len, z.hash};
  const msg::Keys keys = msg::make_keys(d.fmt);
  if (d.fmt.kind == 1 && pat)
    hipLaunchKernelGGL((k_line_parse<1, true>), dim3(nwin), dim3(64), 0, st, text, N, z.wfirst, z.wcnt,
                       (uint32_t)L, d.fmt.line, keys, la, z.derr, pat->prog);
  else if (d.fmt.kind == 1)
    hipLaunchKernelGGL((k_line_parse<1, false>), dim3(nwin), dim3(64), 0, st, text, N, z.wfirst, z.wcnt,
                       (uint32_t)L, d.fmt.line, keys, la, z.derr, NoProgram{});
  else if (pat)
    hipLaunchKernelGGL((k_line_parse<0, true>), dim3(nwin), dim3(64), 0, st, text, N, z.wfirst, z.wcnt,
                       (uint32_t)L, d.fmt.line, NoKeys{}, la, z.derr, pat->prog);
  else
    hipLaunchKernelGGL((k_line_parse<0, false>), dim3(nwin), dim3(64), 0, st, text, N, z.wfirst, z.wcnt,
                       (uint32_t)L, d.fmt.line, NoKeys{}, la, z.derr, NoProgram{});
  RM_HIP(hipGetLastError());
  // ---- "is a point" flags and the counts of the rest
  const uint32_t sb = std::min<uint32_t>(1024u, grid(L));
  need(z.stats, sb * 3ull, st);
  std::vector<uint32_t> spart(3ull * sb);
  uint64_t count[3] = {0, 0, 0};   // blank, outside, host
  auto stats = [&] {
    hipLaunchKernelGGL(k_line_stats, dim3(sb), dim3(256), 0, st, L, la.status, z.flag, z.stats);
    RM_HIP(hipMemcpyAsync(spart.data(), z.stats, sb * 12ull, hipMemcpyDeviceToHost, st));
    RM_HIP(hipMemcpyAsync(z.hctl + 2, z.derr, 4, hipMemcpyDeviceToHost, st));
    RM_HIP(hipStreamSynchronize(st));
    count[0] = count[1] = count[2] = 0;
    for (uint32_t b = 0; b < sb; ++b)
      for (int i = 0; i < 3; ++i) count[i] += spart[3 * b + i];
  };
  stats();
  if (z.hctl[2]) throw std::runtime_error("line reader: the count and parse kernels disagree on a window's lines");
  // ---- host lines: the generic rule, patched into their slots
  const uint32_t H = (uint32_t)count[2];
  if (H) {
    std::vector<uint8_t> status(L);
    RM_HIP(hipMemcpy(status.data(), la.status, L, hipMemcpyDeviceToHost));
    std::vector<HostLine> hl;
    hl.reserve(H);
    for (const uint8_t* p = status.data(), *e = p + L; (p = (const uint8_t*)std::memchr(p, (int)sv::kHost, (size_t)(e - p))); ++p) {
      HostLine h;
      h.line = (uint32_t)(p - status.data());
      hl.push_back(h);
    }
    if (hl.size() != H) throw std::runtime_error("line reader: host line count changed");
    std::vector<uint32_t> off(L);
    RM_HIP(hipMemcpy(off.data(), la.id_off, L * 4, hipMemcpyDeviceToHost));
    for (const HostLine& h : hl) host_chunk(z.chunk_of(off[h.line]));
    HostPool& pool = HostPool::get();
    const size_t nt = std::max<size_t>(1, std::min<size_t>(pool.size(), H / 256u + 1u));
    pool.run(nt, [&](size_t t) {
      for (size_t i = H * t / nt, e = H * (t + 1) / nt; i < e; ++i) {
        HostLine& h = hl[i];
        const uint64_t at = off[h.line];
        const uint32_t c = z.chunk_of(at);
        const uint8_t* b = (const uint8_t*)src[c] + (at - z.chunk_base[c]);
        const uint8_t* ce = (const uint8_t*)src[c] + slen[c];
        const uint8_t* nl = (const uint8_t*)std::memchr(b, '\n', (size_t)(ce - b));
        h.status = msg::generic_message(b, nl ? nl : ce, d.fmt, h.v, &h.why, pat);
        h.v.id_off += (uint32_t)at;
      }
    });
    for (const HostLine& h : hl) {   // in input order: the first bad line fails a strict call
      if (h.status != sv::kBad) continue;
      ++z.n_dropped;
      if (!d.strict && z.dropped.size() >= kMaxDropped) continue;
      const uint64_t at = off[h.line];
      const uint32_t c = z.chunk_of(at);
      const char* b = src[c];
      const uint64_t line = 1 + (uint64_t)std::count(b, b + (at - z.chunk_base[c]), '\n');
      if (d.strict) throw std::runtime_error("chunk " + std::to_string(c + 1) + " line " + std::to_string(line) + ": " + h.why);
      z.dropped.push_back(DroppedMessage{c + 1, line, h.why});   // (its slot is patched to kBad: no point)
    }
    // one block: line, id_off, id_len, lat, lon, acc (u32 / f32), then time, hash, then status
    const uint64_t Hp = (H + 1ull) & ~1ull;
    std::vector<uint8_t> blk(Hp * 24 + Hp * 16 + Hp);
    uint32_t* w = (uint32_t*)blk.data();
    double* tm = (double*)(blk.data() + Hp * 24);
    unsigned long long* hs = (unsigned long long*)(blk.data() + Hp * 32);
    uint8_t* sp = blk.data() + Hp * 40;
    for (uint32_t i = 0; i < H; ++i) {
      const HostLine& h = hl[i];
      w[i] = h.line; w[Hp + i] = h.v.id_off; w[2 * Hp + i] = h.v.id_len;
      std::memcpy(&w[3 * Hp + i], &h.v.lat, 4); std::memcpy(&w[4 * Hp + i], &h.v.lon, 4); std::memcpy(&w[5 * Hp + i], &h.v.acc, 4);
      tm[i] = h.v.time; hs[i] = h.v.hash; sp[i] = (uint8_t)h.status;
    }
    need(z.patch, blk.size(), st);
    RM_HIP(hipMemcpy(z.patch, blk.data(), blk.size(), hipMemcpyHostToDevice));
    const uint8_t* pb = z.patch;
    const uint32_t* pw = (const uint32_t*)pb;
    LinePatch lp{pw, pb + Hp * 40, (const float*)(pw + 3 * Hp), (const float*)(pw + 4 * Hp), (const float*)(pw + 5 * Hp),
                 (const double*)(pb + Hp * 24), pw + Hp, pw + 2 * Hp, (const unsigned long long*)(pb + Hp * 32)};
    hipLaunchKernelGGL(k_line_patch, dim3(grid(H)), dim3(256), 0, st, H, lp, la);
    stats();   // again, over the patched statuses
    if (count[2]) throw std::runtime_error("line reader: a host line was left unread");
  }
  z.info[0] = L;
  z.info[1] = count[0];
  z.info[2] = count[1];
  z.info[5] = H;
  // ---- the kept points, in input order
  z.scr.scan<uint32_t>(z.flag, z.pos, L, st);
  z.timer.toc(st);
  z.timer.tic(2, st);
  const uint64_t P = L - z.info[1] - z.info[2] - z.n_dropped;
  z.info[3] = P;
  z.n_points = P;
  if (P == 0) { RM_HIP(hipStreamSynchronize(st)); z.timer.harvest(nullptr); z.parsed = true; return; }
  ensure_points(P, 0, 1);
  StageBufs& s = sb_;
  need(z.p_off, P, st); need(z.p_len, P, st);
  const unsigned long long mask = hash_mask();
  hipLaunchKernelGGL(k_line_compact, dim3(grid(L)), dim3(256), 0, st, L, la, z.flag, z.pos, mask,
                     s.p_time, s.p_lon, s.p_lat, s.p_acc, z.p_off, z.p_len, s.k0, s.v0);
  // ---- the time span (the window sort's key base)
  const uint32_t nb = std::min<uint32_t>(1024u, grid(P));
  need(z.part, nb * 2ull, st);
  hipLaunchKernelGGL(k_time_span, dim3(nb), dim3(256), 0, st, P, s.p_time, z.part);
  std::vector<double> part(2ull * nb);
  RM_HIP(hipMemcpyAsync(part.data(), z.part, nb * 16ull, hipMemcpyDeviceToHost, st));
  // ---- vehicle ids in first-seen order
  int bits = 0;
  while (bits < 64 && (mask >> bits)) ++bits;
  s.scr.sort_pairs(s.k0.get(), s.k1.get(), s.v0, s.v1, P, bits, st);
  hipLaunchKernelGGL(k_id_flags, dim3(grid(P)), dim3(256), 0, st, P, s.k1, s.v1, z.p_off, z.p_len,
                     text + kLineFront, s.flag, z.derr + 1);
  s.scr.scan<uint32_t>(s.flag, s.idx, P, st);
  // k0 / v0 are free again: the groups' (first point, group) pairs; wstart: each point's group
  hipLaunchKernelGGL(k_id_groups, dim3(grid(P)), dim3(256), 0, st, P, s.flag, s.idx, s.v1, s.k0, s.v0, s.wstart, z.hctl + 4);
  RM_HIP(hipMemcpyAsync(z.hctl + 3, z.derr + 1, 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  z.tmin = part[0];
  z.tmax = part[1];
  for (uint32_t b = 1; b < nb; ++b) { z.tmin = std::min(z.tmin, part[2 * b]); z.tmax = std::max(z.tmax, part[2 * b + 1]); }
  if (!z.hctl[3]) {
    const uint32_t G = z.hctl[4];
    need(z.v_off, G, st); need(z.v_len, G, st);
    s.scr.sort_pairs(s.k0.get(), s.k1.get(), s.v0, s.v1, G, 32, st);
    hipLaunchKernelGGL(k_id_rank, dim3(grid(G)), dim3(256), 0, st, G, s.k1, s.v1, z.p_off, z.p_len,
                       s.wcnt, z.v_off, z.v_len);
    hipLaunchKernelGGL(k_id_scatter, dim3(grid(P)), dim3(256), 0, st, P, s.wstart, s.wcnt, s.p_uuid);
    z.veh_off.resize(G);
    z.veh_len.resize(G);
    RM_HIP(hipMemcpyAsync(z.veh_off.data(), z.v_off, G * 4ull, hipMemcpyDeviceToHost, st));
    RM_HIP(hipMemcpyAsync(z.veh_len.data(), z.v_len, G * 4ull, hipMemcpyDeviceToHost, st));
  } else {
    // two ids share a hash: number them on the host from their bytes (the same numbering)
    std::vector<uint32_t> off(P), len(P), id(P);
    RM_HIP(hipMemcpy(off.data(), z.p_off, P * 4, hipMemcpyDeviceToHost));
    RM_HIP(hipMemcpy(len.data(), z.p_len, P * 4, hipMemcpyDeviceToHost));
    std::unordered_map<std::string_view, uint32_t> table;
    uint32_t c = 0;
    for (uint64_t k = 0; k < P; ++k) {
      while (off[k] >= z.chunk_base[c + 1]) ++c;   // points are in input order
      const std::string_view name(host_chunk(c) + (off[k] - z.chunk_base[c]), len[k]);
      const auto it = table.emplace(name, (uint32_t)table.size());
      if (it.second) { z.veh_off.push_back(off[k]); z.veh_len.push_back(len[k]); }
      id[k] = it.first->second;
    }
    RM_HIP(hipMemcpy(s.p_uuid, id.data(), P * 4, hipMemcpyHostToDevice));
    z.info[6] = 1;
    // (the name spans on the device too, as the other branch leaves them: the directory reads them)
    const uint64_t G = z.veh_off.size();
    need(z.v_off, G, st); need(z.v_len, G, st);
    RM_HIP(hipMemcpy(z.v_off, z.veh_off.data(), G * 4, hipMemcpyHostToDevice));
    RM_HIP(hipMemcpy(z.v_len, z.veh_len.data(), G * 4, hipMemcpyHostToDevice));
  }
  z.timer.toc(st);
  RM_HIP(hipStreamSynchronize(st));
  z.timer.harvest(z.ms);
  z.ms[0] += gz_upload;
  z.info[4] = z.veh_off.size();
  z.n_groups = (uint32_t)z.veh_off.size();
  z.parsed = true;
}

int Matcher::device() const { return eng_->device(); }

bool Matcher::line_time_span(double t[2]) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  if (!ls_->n_points) return false;
  t[0] = ls_->tmin;
  t[1] = ls_->tmax;
  return true;
}

LineGroups Matcher::line_groups() const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  const LineState& z = *ls_;
  LineGroups g;
  g.n_points = z.n_points;
  g.n_groups = z.n_points ? z.n_groups : 0u;
  g.text = z.n_points ? z.text + kLineFront : nullptr;
  g.v_off = z.v_off; g.v_len = z.v_len;
  g.p_uuid = sb_.p_uuid; g.p_time = sb_.p_time; g.p_lon = sb_.p_lon; g.p_lat = sb_.p_lat; g.p_acc = sb_.p_acc;
  g.hash_mask = hash_mask();
  return g;
}

uint64_t Matcher::dropped_messages(std::vector<DroppedMessage>* first) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  if (first) *first = ls_->dropped;
  return ls_->n_dropped;
}

void Matcher::run_lines(const LinesDesc& d, const RunParams& rp) {
  if (d.n_opts == 0 || !d.opts) throw std::runtime_error("line batch needs at least one option set");
  scan_options(d.opts, 1);   // every window takes opts[0]
  parse_lines(d);
  LineState& z = *ls_;
  from_points_ = true;
  const uint64_t n = z.n_points;
  if (n == 0) { n_traces_ = 0; n_points_ = 0; n_trans_ = 0; n_path_ = 0; seg_used_ = 0; return; }
  const double tbase = std::floor(z.tmin);
  if (std::floor(z.tmax) - tbase >= 4294967295.0) throw std::runtime_error("point times span more than 2^32 s");
  z.timer.tic(3, stream_);   // the windows: closed inside run_points_device
  run_points_device(n, tbase, d.inactivity, d.opts, 1, 0, rp, &z.timer);
  z.timer.harvest(z.ms);
}

void Matcher::lines_info(uint64_t out[7]) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  std::copy(ls_->info, ls_->info + 7, out);
}

void Matcher::lines_time(double ms[4]) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  std::copy(ls_->ms, ls_->ms + 4, ms);
}

void Matcher::get_line_points(uint32_t* uuid, double* time, float* lon, float* lat, float* acc) {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  const uint64_t P = ls_->n_points;
  if (!P) return;
  RM_HIP(hipSetDevice(eng_->device()));
  RM_HIP(hipStreamSynchronize(stream_));
  const StageBufs& s = sb_;
  RM_HIP(hipMemcpy(uuid, s.p_uuid, P * 4, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(time, s.p_time, P * 8, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(lon, s.p_lon, P * 4, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(lat, s.p_lat, P * 4, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(acc, s.p_acc, P * 4, hipMemcpyDeviceToHost));
}

void Matcher::set_input_coding(int coding, bool skip_bad) {
  if (coding < 0 || coding > 2) throw std::runtime_error("input coding must be 0 (plain), 1 (gzip) or 2 (by magic)");
  input_coding_ = coding;
  skip_bad_chunks_ = skip_bad;
}

uint32_t Matcher::chunk_count() const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  return (uint32_t)ls_->gz_status.size();
}

void Matcher::chunk_status(uint32_t* status) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  std::copy(ls_->gz_status.begin(), ls_->gz_status.end(), status);
}

void Matcher::inflate_info(uint64_t out[6]) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  std::copy(ls_->gz_info, ls_->gz_info + 6, out);
}

void Matcher::inflate_time(double ms[3]) const {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  std::copy(ls_->gz_ms, ls_->gz_ms + 3, ms);
}

void Matcher::get_text(uint32_t chunk, uint64_t off, uint64_t len, char* out) {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  const LineState& z = *ls_;
  if (chunk + 1ull >= z.chunk_base.size()) throw std::runtime_error("get_text: no such chunk");
  const uint64_t room = z.chunk_base[chunk + 1] - z.chunk_base[chunk];
  if (off > room || len > room - off) throw std::runtime_error("get_text: the span leaves the chunk");
  if (!len) return;
  if (!out) throw std::runtime_error("get_text: out is NULL");
  RM_HIP(hipSetDevice(eng_->device()));
  RM_HIP(hipStreamSynchronize(stream_));
  RM_HIP(hipMemcpy(out, z.text + kLineFront + z.chunk_base[chunk] + off, len, hipMemcpyDeviceToHost));
}

void Matcher::get_vehicles(uint32_t* chunk, uint64_t* off, uint32_t* len) {
  if (!ls_ || !ls_->parsed) throw std::runtime_error("no lines have been parsed");
  const LineState& z = *ls_;
  for (size_t v = 0; v < z.veh_off.size(); ++v) {
    const uint32_t c = z.chunk_of(z.veh_off[v]);
    chunk[v] = c;
    off[v] = z.veh_off[v] - z.chunk_base[c];
    len[v] = z.veh_len[v];
  }
}

// The generic rule over the same input, on the host alone (rm_lines_parse_host): every array may be
// null (a first call sizes them from info[3] points and info[4] vehicles)
void lines_parse_host(const LinesDesc& d, uint64_t info[7], uint32_t* uuid, double* time, float* lon, float* lat, float* acc,
                      uint32_t* v_chunk, uint64_t* v_off, uint32_t* v_len) {
  if (d.n_chunks && (!d.data || !d.len)) throw std::runtime_error("line chunks are NULL");
  const tp::Pattern* pat = time_pattern_of(d.fmt);
  if (const char* e = sv::format_error(d.fmt, pat ? &pat->prog : nullptr); *e) throw std::runtime_error(std::string("line format: ") + e);
  std::fill(info, info + 7, 0);
  std::unordered_map<std::string_view, uint32_t> table;
  uint64_t P = 0;
  for (uint32_t c = 0; c < d.n_chunks; ++c) {
    const uint8_t* b = (const uint8_t*)d.data[c];
    const uint8_t* const b0 = b;
    const uint8_t* const e = b + d.len[c];
    uint64_t line = 0;
    while (b < e) {
      const uint8_t* nl = (const uint8_t*)std::memchr(b, '\n', (size_t)(e - b));
      const uint8_t* le = nl ? nl : e;
      ++line;
      sv::Line v{};
      const char* why = nullptr;
      const uint32_t st = sv::generic_line(b, le, d.fmt, v, &why, pat);
      if (st == sv::kBad) throw std::runtime_error("chunk " + std::to_string(c + 1) + " line " + std::to_string(line) + ": " + why);
      ++info[0];
      info[1] += st == sv::kBlank;
      info[2] += st == sv::kOutside;
      if (st == sv::kPoint) {
        const uint8_t* id = b + v.id_off;
        const auto it = table.emplace(std::string_view((const char*)id, v.id_len), (uint32_t)table.size());
        if (it.second) {
          const size_t r = table.size() - 1;
          if (v_chunk) v_chunk[r] = c;
          if (v_off) v_off[r] = (uint64_t)(id - b0);
          if (v_len) v_len[r] = v.id_len;
        }
        if (uuid) uuid[P] = it.first->second;
        if (time) time[P] = v.time;
        if (lon) lon[P] = v.lon;
        if (lat) lat[P] = v.lat;
        if (acc) acc[P] = v.acc;
        ++P;
      }
      b = nl ? nl + 1 : e;
    }
  }
  info[3] = P;
  info[4] = table.size();
}

// Rule 14's generic rule over the same input, on the host alone (rm_messages_parse_host): as
// lines_parse_host, with either kind; a tolerant call drops and lists malformed lines
void messages_parse_host(const MessagesDesc& d, uint64_t info[8], uint32_t* uuid, double* time, float* lon, float* lat, float* acc,
                         uint32_t* v_chunk, uint64_t* v_off, uint32_t* v_len, std::vector<DroppedMessage>* dropped) {
  if (d.n_chunks && (!d.data || !d.len)) throw std::runtime_error("message chunks are NULL");
  const tp::Pattern* pat = time_pattern_of(d.fmt.line);
  if (const char* e = msg::format_error(d.fmt, pat ? &pat->prog : nullptr); *e) throw std::runtime_error(std::string("message format: ") + e);
  std::fill(info, info + 8, 0);
  if (dropped) dropped->clear();
  std::unordered_map<std::string_view, uint32_t> table;
  uint64_t P = 0;
  for (uint32_t c = 0; c < d.n_chunks; ++c) {
    const uint8_t* b = (const uint8_t*)d.data[c];
    const uint8_t* const b0 = b;
    const uint8_t* const e = b + d.len[c];
    uint64_t line = 0;
    while (b < e) {
      const uint8_t* nl = (const uint8_t*)std::memchr(b, '\n', (size_t)(e - b));
      const uint8_t* le = nl ? nl : e;
      ++line;
      sv::Line v{};
      const char* why = nullptr;
      const uint32_t st = msg::generic_message(b, le, d.fmt, v, &why, pat);
      if (st == sv::kBad && d.strict)
        throw std::runtime_error("chunk " + std::to_string(c + 1) + " line " + std::to_string(line) + ": " + why);
      ++info[0];
      info[1] += st == sv::kBlank;
      info[2] += st == sv::kOutside;
      if (st == sv::kBad) {
        ++info[7];
        if (dropped && dropped->size() < kMaxDropped) dropped->push_back(DroppedMessage{c + 1, line, why});
      }
      if (st == sv::kPoint) {
        const uint8_t* id = b + v.id_off;
        const auto it = table.emplace(std::string_view((const char*)id, v.id_len), (uint32_t)table.size());
        if (it.second) {
          const size_t r = table.size() - 1;
          if (v_chunk) v_chunk[r] = c;
          if (v_off) v_off[r] = (uint64_t)(id - b0);
          if (v_len) v_len[r] = v.id_len;
        }
        if (uuid) uuid[P] = it.first->second;
        if (time) time[P] = v.time;
        if (lon) lon[P] = v.lon;
        if (lat) lat[P] = v.lat;
        if (acc) acc[P] = v.acc;
        ++P;
      }
      b = nl ? nl + 1 : e;
    }
  }
  info[3] = P;
  info[4] = table.size();
}

}  // namespace rm
