// tilestore.hip — the tile store (DESIGN.md §3 rule 13): the reference's streaming anonymiser
// (AnonymisingProcessor.java:120-153, 155-175, 222-266; TimeQuantisedTile.java:26-35;
// Segment.java:38-74) kept and flushed in HBM.
//
//   store   one growable array of TileStoreRow in arrival order (capacity doubles, device copy)
//   add     k_ts_count (rows per segment, the stated limits as error bits) -> exclusive scan ->
//           one host read of total and error word -> growth or failure -> k_ts_emit appends.
//           The segments come from host arrays through pinned staging, or straight from a
//           session's device buffer of forwarded reports: both are 40 bytes at a stride.
//   flush   sort: four stable radix passes from arrival order (next_id, id, tile, bucket);
//           cull: run flags, scan, the per-run keep rule of clean() inside a file, row flags,
//           compaction of the kept rows' indices;
//           text: bytes per kept row (k_ts_len), a 64-bit exclusive scan, and k_ts_write, in which
//           a wave builds the contiguous span of its 64 rows in LDS and streams it to the blob in
//           aligned 16-byte stores (the unaligned head and tail byte-wise);
//           one download of the blob.
//
// One stream, no graph, HIP events per stage.  Nothing loops over segments or rows on the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "engine.hpp"
#include "tile_cull.hpp"
#include "tile_text.hpp"

namespace rm {

namespace {

constexpr uint32_t kTsErrId = 1u, kTsErrTime = 2u, kTsErrSpan = 4u;
constexpr uint64_t kTsMaxSpan = 65536;
constexpr uint64_t kTsMaxRows = 0x7fffffffull;   // (hipcub takes the item count as an int)
constexpr double kTwo53 = 9007199254740992.0;

// device counters (u64), mirrored in pinned memory
enum TsCtr : int { kTKept = 0, kTSkipped, kTErr, kTTotal, kTTiles, kTFiles, kTRuns, kTKeptRows, kTBytes, kTNumCtr = 16 };

struct SegSrc {   // segment j: {u64 id, u64 next_id, f64 min, f64 max, i32 length, i32 queue} at base + j * stride
  const char* base;
  uint32_t stride;
};
struct SegIn {
  uint64_t id, next_id;
  double mn, mx;
  int32_t length, queue;
};
__device__ __forceinline__ SegIn load_seg(SegSrc s, uint64_t j) {
  const char* p = s.base + j * (uint64_t)s.stride;   // base and stride are multiples of 8
  SegIn g;
  g.id = *(const uint64_t*)p; g.next_id = *(const uint64_t*)(p + 8);
  g.mn = *(const double*)(p + 16); g.mx = *(const double*)(p + 24);
  g.length = *(const int32_t*)(p + 32); g.queue = *(const int32_t*)(p + 36);
  return g;
}

// one atomic per block for a predicate's count; every thread of the block calls it
__device__ __forceinline__ void block_count(unsigned long long* c, bool p) {
  const int n = __syncthreads_count(p ? 1 : 0);
  if (threadIdx.x == 0 && n) atomicAdd(c, (unsigned long long)n);
}

// the stated limits of rule 13 (error bits; 0: none), then the rows a segment adds
__device__ __forceinline__ uint32_t seg_rows(const SegIn& g, uint64_t q, uint64_t& first_bucket, uint32_t& err) {
  err = 0u;
  if (g.id > 0x7fffffffffffffffull || g.next_id > 0x7fffffffffffffffull) err |= kTsErrId;
  if (!(g.mn - g.mn == 0.0) || !(g.mx - g.mx == 0.0) || g.mx >= kTwo53) err |= kTsErrTime;
  if (err || !tt_valid(g.mn, g.mx, g.length, g.queue)) return 0u;
  // TimeQuantisedTile.java:28-30: the times truncated (0 < min < max < 2^53)
  const uint64_t lo = (uint64_t)g.mn / q, hi = (uint64_t)g.mx / q;
  first_bucket = lo;
  if (hi - lo + 1ull > kTsMaxSpan) { err |= kTsErrSpan; return 0u; }
  return (uint32_t)(hi - lo + 1ull);
}

__global__ void k_ts_count(SegSrc s, uint64_t n, uint64_t q, unsigned long long* cnt, unsigned long long* ctr) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool kept = false, skipped = false;
  if (j < n) {
    const SegIn g = load_seg(s, j);
    uint64_t b0 = 0;
    uint32_t err = 0;
    const uint32_t rows = seg_rows(g, q, b0, err);
    cnt[j] = rows;
    if (err) atomicOr(ctr + kTErr, (unsigned long long)err);
    kept = rows > 0u;
    skipped = !err && !kept;
  } else if (j == n) {
    cnt[n] = 0ull;   // the scan's last entry is the total
  }
  block_count(ctr + kTKept, kept);
  block_count(ctr + kTSkipped, skipped);
}

__global__ void k_ts_emit(SegSrc s, uint64_t n, uint64_t q, const unsigned long long* ofs, TileStoreRow* rows, uint64_t at0,
                          uint64_t cap, uint64_t arrival0) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t o = ofs[j], c = ofs[j + 1] - o;
  if (!c) return;
  const SegIn g = load_seg(s, j);
  TileStoreRow t;
  t.id = g.id; t.next_id = g.next_id;
  t.start = (int64_t)floor(g.mn); t.end = (int64_t)ceil(g.mx);   // Segment.java:70-71
  t.duration = tt_duration(g.mn, g.mx); t.length = g.length; t.queue = g.queue;
  t.tile = (uint32_t)(g.id & 0x1FFFFFFull);                       // Segment.java:34-36
  t.arrival = arrival0 + j;
  const uint64_t b0 = (uint64_t)g.mn / q;
  for (uint64_t i = 0; i < c; ++i) {
    const uint64_t at = at0 + o + i;
    if (at >= cap) return;
    t.bucket = b0 + i;
    rows[at] = t;
  }
}

// sort key of a pass: 0 next_id, 1 id (Segment.compareTo, least significant first), 2 tile, 3 bucket
__global__ void k_ts_key(uint64_t n, const TileStoreRow* rows, const uint32_t* perm, int which, unsigned long long* key) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const TileStoreRow& t = rows[perm[k]];
  key[k] = which == 0 ? t.next_id : (which == 1 ? t.id : (which == 2 ? (unsigned long long)t.tile : t.bucket));
}

__device__ __forceinline__ bool same_file(const TileStoreRow& a, const TileStoreRow& b) {
  return a.bucket == b.bucket && a.tile == b.tile;
}

struct TsSameFile {
  __device__ bool operator()(const TileStoreRow& a, const TileStoreRow& b) const { return same_file(a, b); }
};

// the kept rows' store indices in sorted order
__global__ void k_ts_compact(uint64_t n, const uint32_t* perm, const uint32_t* flag, const uint32_t* ofs, uint32_t* kperm,
                             unsigned long long* ctr) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (flag[k]) kperm[ofs[k]] = perm[k];
  if (k + 1 == n) ctr[kTKeptRows] = ofs[k] + flag[k];
}

// bytes of kept row k's piece of the blob (tile_text.hpp tt_piece_len); also counts the files
__global__ void k_ts_len(uint32_t K, const TileStoreRow* rows, const uint32_t* kperm, TileText tt, unsigned long long* len,
                         unsigned long long* ctr) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  bool first = false;
  if (k < K) {
    const TileStoreRow r = rows[kperm[k]];
    first = k == 0u || !same_file(rows[kperm[k - 1]], r);
    len[k] = tt_piece_len(r, tt, first, k == 0u, k + 1u == K);
  }
  block_count(ctr + kTFiles, first);
}

// total bytes = off[K - 1] + len[K - 1]
__global__ void k_ts_total(uint32_t K, const unsigned long long* off, const unsigned long long* len, unsigned long long* ctr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr[kTBytes] = off[K - 1u] + len[K - 1u];
}

// One wave per block, one kept row per lane.  The pieces of the block's 64 rows are contiguous in
// the blob ([off[k0], off[klast] + len[klast])), so the lanes write them into LDS at the blob
// offset's distance from the span's start, shifted by the start's offset inside its 16 bytes: LDS
// and blob positions are then congruent mod 16, and the span goes out as aligned 16-byte loads and
// stores, 1 KiB per wave instruction, with up to 15 head and 15 tail bytes stored singly.  The LDS
// holds the worst case, every row opening a file: 64 x kTtMaxPiece (+ 16 for the shift).
constexpr uint32_t kTsSpan = 64u * kTtMaxPiece + 16u;
static_assert(kTsSpan <= 65536u, "the span of one wave fits the LDS of a work-group");

__global__ void __launch_bounds__(64) k_ts_write(uint32_t K, const TileStoreRow* rows, const uint32_t* kperm, TileText tt,
                                                 const unsigned long long* off, const unsigned long long* len, char* blob,
                                                 unsigned long long total) {
  __shared__ __attribute__((aligned(16))) char sh[kTsSpan];
  const uint32_t lane = threadIdx.x;
  const uint32_t k0 = blockIdx.x * 64u;
  if (k0 >= K) return;
  const uint32_t klast = k0 + 63u < K ? k0 + 63u : K - 1u;
  const unsigned long long base = off[k0];
  unsigned long long end = off[klast] + len[klast];
  if (end > total) end = total;
  if (end - base > (unsigned long long)(kTsSpan - 16u)) return;   // (cannot happen: every piece <= kTtMaxPiece)
  const uint32_t shift = (uint32_t)(base & 15ull);
  const uint32_t k = k0 + lane;
  if (k <= klast) {
    const TileStoreRow r = rows[kperm[k]];
    const bool first = k == 0u || !same_file(rows[kperm[k - 1]], r);
    const unsigned long long o = off[k] - base;
    if (o + len[k] <= end - base) tt_put_piece(sh + shift + (uint32_t)o, r, tt, first, k == 0u, k + 1u == K);
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

}  // namespace

struct TileStore::Impl {
  static constexpr const char* kFull = "tile store buffers do not fit in HBM";
  int device = 0;
  TileParams tp;
  TileText tt;
  hipStream_t st = nullptr;
  // the store
  DevBuf<TileStoreRow> rows;
  uint64_t n_rows = 0, cap = 0, arrivals = 0;
  // counters
  DevBuf<unsigned long long> ctr;
  PinBuf<unsigned long long> hctr;   // pinned mirror
  // add: pinned staging and its device copy, counts and offsets
  PinBuf<char> hstage; DevBuf<char> dstage; uint64_t stage_cap = 0;
  DevBuf<unsigned long long> cnt, ofs; uint64_t cnt_cap = 0;
  // flush scratch (sized by the rows held)
  DevBuf<unsigned long long> k0, k1;
  DevBuf<uint32_t> p0, p1, flag, gid, gpos;
  DevBuf<uint8_t> gkeep; uint64_t fl_cap = 0;
  DevBuf<char> blob; uint64_t blob_cap = 0;
  ScanScratch scr{kFull};
  // HIP-event pairs by part: 0 upload, 1 expand, 2 sort, 3 cull, 4 text, 5 download
  PartTimer timer;
  double ms[6] = {0, 0, 0, 0, 0, 0};

  ~Impl() {
    if (st) (void)hipStreamDestroy(st);
  }
  void begin_call() {
    timer.harvest(nullptr);   // (pairs a call that threw left behind)
    for (double& x : ms) x = 0.0;
    RM_HIP(hipMemsetAsync(ctr, 0, kTNumCtr * sizeof(unsigned long long), st));
  }
  void read_ctr() {
    RM_HIP(hipMemcpyAsync(hctr, ctr, kTNumCtr * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    RM_HIP(hipStreamSynchronize(st));
    timer.harvest(ms);
  }
  // room for `need` rows: the capacity doubles and the rows held move by a device copy
  void ensure_rows(uint64_t need) {
    if (need <= cap) return;
    uint64_t c = std::max<uint64_t>(cap, 1);
    while (c < need) c *= 2;
    rows.reserve(c, kFull, n_rows, st);
    cap = c;
  }
  void ensure_counts(uint64_t n) {
    if (n + 1 <= cnt_cap) return;
    cnt_cap = 0;
    const uint64_t c = std::max<uint64_t>(n + n / 2 + 1, 4096);
    cnt.reserve(c, kFull); ofs.reserve(c, kFull);
    cnt_cap = c;
  }
  void ensure_stage(uint64_t n) {
    if (n <= stage_cap) return;
    stage_cap = 0;
    const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
    hstage.reserve(c * sizeof(TileSegment));
    dstage.reserve(c * sizeof(TileSegment), kFull);
    stage_cap = c;
  }
  void ensure_flush(uint64_t n) {
    if (n <= fl_cap) return;
    fl_cap = 0;
    k0.reserve(n, kFull); k1.reserve(n, kFull);
    p0.reserve(n, kFull); p1.reserve(n, kFull); flag.reserve(n, kFull); gid.reserve(n, kFull);
    gpos.reserve(n + 1, kFull); gkeep.reserve(n, kFull);
    fl_cap = n;
  }

  // count, scan, one read, growth or failure, emit: the n segments at `src` join the store
  void add_device(SegSrc src, uint64_t n, uint64_t out[4]) {
    if (n >= kTsMaxRows) throw BatchTooLarge("tile store call too large (segments >= 2^31 - 1)");
    ensure_counts(n);
    timer.tic(1, st);
    hipLaunchKernelGGL(k_ts_count, dim3(grid(n + 1)), dim3(256), 0, st, src, n, (uint64_t)tp.quantisation, cnt, ctr);
    scr.scan<unsigned long long>(cnt, ofs, n + 1, st);
    RM_HIP(hipMemcpyAsync(ctr + kTTotal, ofs + n, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    timer.toc(st);
    RM_HIP(hipGetLastError());
    read_ctr();   // nothing of the store has changed yet: a bad segment leaves it as it was
    const uint64_t err = hctr[kTErr];
    if (err & kTsErrId) throw std::runtime_error("tile segment id or next_id above 2^63 - 1");
    if (err & kTsErrTime) throw std::runtime_error("tile segment time is not finite or max >= 2^53");
    if (err & kTsErrSpan) throw std::runtime_error("tile segment spans more than 65536 time buckets");
    const uint64_t total = hctr[kTTotal];
    if (n_rows + total >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
    ensure_rows(n_rows + total);
    if (total) {
      timer.tic(1, st);
      hipLaunchKernelGGL(k_ts_emit, dim3(grid(n)), dim3(256), 0, st, src, n, (uint64_t)tp.quantisation,
                         (const unsigned long long*)ofs, rows, n_rows, cap, arrivals);
      timer.toc(st);
      RM_HIP(hipGetLastError());
      RM_HIP(hipStreamSynchronize(st));
      timer.harvest(ms);
    }
    n_rows += total;
    arrivals += n;
    if (out) { out[0] = hctr[kTKept]; out[1] = hctr[kTSkipped]; out[2] = total; out[3] = n_rows; }
  }
};

TileStore::TileStore(int device, const TileParams& tp, uint64_t initial_rows) : p_(new Impl) {
  Impl& s = *p_;
  // AnonymisingProcessor.java:73-80
  if (tp.privacy < 1) throw std::runtime_error("tile store needs a privacy parameter of 1 or more");
  if (tp.quantisation < 60) throw std::runtime_error("tile store needs a quantisation parameter of 60 or more");
  if (tp.source.size() > kTtMaxSource) throw std::runtime_error("tile store source is longer than 64 bytes");
  if (tp.mode.size() > kTtMaxMode) throw std::runtime_error("tile store mode is longer than 16 bytes");
  for (const std::string* x : {&tp.source, &tp.mode})
    for (char ch : *x)
      if (ch == ',' || ch == '\n' || ch == '\r' || ch == 0) throw std::runtime_error("tile store source and mode may not contain ',' or a newline");
  if (initial_rows >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  s.device = device;
  s.tp = tp;
  std::memset(&s.tt, 0, sizeof s.tt);
  s.tt.quantisation = tp.quantisation;
  s.tt.source_len = (uint32_t)tp.source.size();
  s.tt.mode_len = (uint32_t)tp.mode.size();
  std::memcpy(s.tt.source, tp.source.data(), tp.source.size());
  std::memcpy(s.tt.mode, tp.mode.data(), tp.mode.size());
  RM_HIP(hipSetDevice(device));
  RM_HIP(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
  s.ctr.reserve(kTNumCtr, Impl::kFull);
  s.hctr.reserve(kTNumCtr);
  s.cap = std::max<uint64_t>(initial_rows, 1);
  s.rows.reserve(s.cap, Impl::kFull);
}

TileStore::~TileStore() {
  (void)hipSetDevice(p_->device);
  (void)hipStreamSynchronize(p_->st);
}

int TileStore::device() const { return p_->device; }
uint64_t TileStore::rows_held() const { return p_->n_rows; }
uint64_t TileStore::capacity() const { return p_->cap; }
void TileStore::times(double ms[6]) const { for (int i = 0; i < 6; ++i) ms[i] = p_->ms[i]; }

// the stream snapshot's access (DESIGN.md §3 rule 15)
const void* TileStore::rows_device() const { return p_->rows; }
uint64_t TileStore::arrivals() const { return p_->arrivals; }
uint32_t TileStore::quantisation() const { return p_->tp.quantisation; }
hipStream_t TileStore::stream() const { return p_->st; }
void* TileStore::snapshot_room(uint64_t n_rows) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  if (s.n_rows) throw std::runtime_error("snapshot: the tile store is not empty");
  if (n_rows >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  s.ensure_rows(n_rows);
  return s.rows;
}
void TileStore::snapshot_loaded(uint64_t n_rows, uint64_t arrivals) {
  p_->n_rows = n_rows;
  p_->arrivals = arrivals;
}

void TileStore::add(const TileSegment* segs, uint64_t n, uint64_t out[4]) {
  Impl& s = *p_;
  if (n && !segs) throw std::runtime_error("tile segments are NULL");
  RM_HIP(hipSetDevice(s.device));
  s.begin_call();
  if (n >= kTsMaxRows) throw BatchTooLarge("tile store call too large (segments >= 2^31 - 1)");
  s.ensure_stage(n);
  if (n) {
    std::memcpy(s.hstage, segs, n * sizeof(TileSegment));
    s.timer.tic(0, s.st);
    RM_HIP(hipMemcpyAsync(s.dstage, s.hstage, n * sizeof(TileSegment), hipMemcpyHostToDevice, s.st));
    s.timer.toc(s.st);
  }
  s.add_device(SegSrc{s.dstage, (uint32_t)sizeof(TileSegment)}, n, out);
}

void TileStore::add_session(Session& sess, uint64_t out[4]) {
  Impl& s = *p_;
  if (sess.device() != s.device) throw std::runtime_error("the session is on another device than the tile store");
  RM_HIP(hipSetDevice(s.device));
  s.begin_call();
  // the session's calls return with their stream synchronised: rep_s is complete
  s.add_device(SegSrc{(const char*)sess.reports_device(), (uint32_t)sizeof(SessionReport)}, sess.n_reports(), out);
}

void TileStore::flush(char** blob_out, size_t* len_out, uint64_t out[5]) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  hipStream_t st = s.st;
  s.begin_call();
  const uint64_t R = s.n_rows;
  uint64_t K = 0, tiles = 0, files = 0, bytes = 0;
  if (R) {
    s.ensure_flush(R);
    // ---- Collections.sort over every tile at once: stable LSD passes from arrival order
    s.timer.tic(2, st);
    hipLaunchKernelGGL(k_iota<uint64_t>, dim3(grid(R)), dim3(256), 0, st, R, s.p0);
    uint32_t* pin = s.p0;
    uint32_t* pout = s.p1;
    static const int kBits[4] = {63, 63, 25, 48};   // ids <= 2^63 - 1; tile 25 bits; bucket < 2^53 / 60
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(k_ts_key, dim3(grid(R)), dim3(256), 0, st, R, (const TileStoreRow*)s.rows, (const uint32_t*)pin, pass, s.k0);
      s.scr.sort_pairs(s.k0.get(), s.k1.get(), pin, pout, R, kBits[pass], st);
      std::swap(pin, pout);
    }
    s.timer.toc(st);
    const uint32_t* perm = pin;
    // ---- clean(): runs, keep rule per run, keep flag per row, compaction
    s.timer.tic(3, st);
    hipLaunchKernelGGL((k_cull_gflags<TsSameFile, TileStoreRow>), dim3(grid(R)), dim3(256), 0, st, R, (const TileStoreRow*)s.rows,
                       perm, s.flag);
    s.scr.scan<uint32_t>(s.flag, s.gid, R, st);
    hipLaunchKernelGGL(k_cull_gpos<unsigned long long>, dim3(grid(R)), dim3(256), 0, st, R, (const uint32_t*)s.flag,
                       (const uint32_t*)s.gid, s.gpos, s.ctr + kTRuns);
    s.timer.toc(st);
    RM_HIP(hipGetLastError());
    s.read_ctr();
    const uint32_t G = (uint32_t)s.hctr[kTRuns];
    if (G == 0 || G > R) throw std::runtime_error("tile store run count out of range");
    s.timer.tic(3, st);
    hipLaunchKernelGGL((k_cull_gkeep<TsSameFile, true, TileStoreRow>), dim3(grid(G)), dim3(256), 0, st, G,
                       (const TileStoreRow*)s.rows, perm, (const uint32_t*)s.gpos, s.tp.privacy, s.gkeep, s.ctr + kTTiles);
    // buffers the stages before are done with, in stream order: the spare permutation buffer
    // takes the rows' keep flags; once k_cull_kflags has read them, gid takes the kept rows'
    // offsets and flag their indices; the sort keys take the text lengths and offsets
    uint32_t* kflag = pout;
    uint32_t* kofs = s.gid;
    uint32_t* kperm = s.flag;
    hipLaunchKernelGGL(k_cull_kflags<uint8_t>, dim3(grid(R)), dim3(256), 0, st, R, (const uint32_t*)s.gid, (const uint32_t*)s.flag,
                       (const uint8_t*)s.gkeep, kflag);
    s.scr.scan((const uint32_t*)kflag, kofs, R, st);
    hipLaunchKernelGGL(k_ts_compact, dim3(grid(R)), dim3(256), 0, st, R, perm, (const uint32_t*)kflag, (const uint32_t*)kofs, kperm, s.ctr);
    s.timer.toc(st);
    RM_HIP(hipGetLastError());
    s.read_ctr();
    K = s.hctr[kTKeptRows];
    tiles = s.hctr[kTTiles];
    if (K > R) throw std::runtime_error("tile store kept-row count out of range");
    if (K) {
      // ---- the CSV bytes: lengths, offsets, the write, one download
      unsigned long long* len = s.k1;
      unsigned long long* off = s.k0;
      s.timer.tic(4, st);
      hipLaunchKernelGGL(k_ts_len, dim3(grid(K)), dim3(256), 0, st, (uint32_t)K, (const TileStoreRow*)s.rows, (const uint32_t*)kperm,
                         s.tt, len, s.ctr);
      s.scr.scan((const unsigned long long*)len, off, K, st);
      hipLaunchKernelGGL(k_ts_total, dim3(1), dim3(64), 0, st, (uint32_t)K, (const unsigned long long*)off, (const unsigned long long*)len, s.ctr);
      s.timer.toc(st);
      RM_HIP(hipGetLastError());
      s.read_ctr();
      files = s.hctr[kTFiles];
      bytes = s.hctr[kTBytes];
      if (bytes > K * (uint64_t)kTtMaxPiece) throw std::runtime_error("tile store blob size out of range");
      if (bytes > s.blob_cap) {
        s.blob_cap = 0;
        s.blob.reserve(bytes + bytes / 4 + 16, Impl::kFull);   // (hipMalloc: 256-byte aligned, so blob offsets mod 16 are addresses mod 16)
        s.blob_cap = bytes + bytes / 4;
      }
      s.timer.tic(4, st);
      hipLaunchKernelGGL(k_ts_write, dim3((uint32_t)((K + 63) / 64)), dim3(64), 0, st, (uint32_t)K, (const TileStoreRow*)s.rows,
                         (const uint32_t*)kperm, s.tt, (const unsigned long long*)off, (const unsigned long long*)len, s.blob,
                         (unsigned long long)bytes);
      s.timer.toc(st);
      RM_HIP(hipGetLastError());
    }
  }
  // ---- one download into library memory (released with rm_free)
  char* host = (char*)std::malloc(bytes + 1);
  if (!host) throw std::bad_alloc();
  if (bytes) {
    s.timer.tic(5, st);
    const hipError_t e = hipMemcpyAsync(host, s.blob, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) s.timer.toc(st);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
    if (e2 != hipSuccess) {
      std::free(host);
      RM_HIP(e2);
    }
    s.timer.harvest(s.ms);
  }
  host[bytes] = 0;
  s.n_rows = 0;   // the store is empty after a flush (AnonymisingProcessor.java:229, 240)
  *blob_out = host;
  *len_out = bytes;
  if (out) { out[0] = R; out[1] = K; out[2] = tiles; out[3] = files; out[4] = bytes; }
}

}  // namespace rm
