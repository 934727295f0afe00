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
//   exchange  (rule 16, a stream on several ranks) a key per row beside the rows, call << 32 | a,
//           written by k_ts_emit once the store keeps keys; every rank's rows and keys gathered
//           (export / import through host blobs, or all-gathered through a TileComm), k_ts_own ->
//           scan -> k_ts_own_pack -> one stable radix sort on the key -> k_ts_take: the store then
//           holds the rows of the files it owns in the one-rank order, and flush runs unchanged.
//
// One stream, no graph, HIP events per stage.  Nothing loops over segments or rows on the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
enum TsCtr : int {
  kTKept = 0, kTSkipped, kTErr, kTTotal, kTTiles, kTFiles, kTRuns, kTKeptRows, kTBytes,
  kTOwnLo, kTOwnHi, kTOwned,   // the exchange: owned rows before and behind this rank's own rows, and of all
  kTNumCtr = 16
};

struct SegSrc {   // segment j: {u64 id, u64 next_id, f64 min, f64 max, i32 length, i32 queue} at base + j * stride
  const char* base;
  uint32_t stride;
  // a session's reports: the call's windows, for the triggering arrival of segment j's report (its
  // window index lies at base + j * stride + kRepWindow); null: host segments
  const SessionWindow* win;
  uint32_t n_win;
};
constexpr uint32_t kRepWindow = (uint32_t)offsetof(SessionReport, window);
constexpr unsigned long long kTsPadKey = ~0ull;   // the key of a padding row of the exchange (no row has it: calls < 2^32 - 1)
constexpr uint64_t kTsBlobMagic = 0x31574f5253544d52ull;   // "RMTSROW1"
constexpr uint64_t kTsBlobHead = 32;   // magic, rows, quantisation, 0; then the rows; then their keys
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

// keys null: a store that keeps no keys.  key_hi: the add call's number << 32 (rule 16's row key)
__global__ void k_ts_emit(SegSrc s, uint64_t n, uint64_t q, const unsigned long long* ofs, TileStoreRow* rows, uint64_t at0,
                          uint64_t cap, uint64_t arrival0, unsigned long long* keys, unsigned long long key_hi) {
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
  unsigned long long key = key_hi | (j & 0xffffffffull);
  if (keys && s.win) {
    const uint32_t w = *(const uint32_t*)(s.base + j * (uint64_t)s.stride + kRepWindow);
    key = key_hi | (w < s.n_win ? s.win[w].arrival : 0xffffffffu);
  }
  for (uint64_t i = 0; i < c; ++i) {
    const uint64_t at = at0 + o + i;
    if (at >= cap) return;
    t.bucket = b0 + i;
    rows[at] = t;
    if (keys) keys[at] = key;
  }
}

// rows [b, e) of a store that kept no keys so far, all of add call `key_hi >> 32` whose first
// segment had the running number arrival0: the key the call would have written (host segments: the
// index in the array; a session that was never sharded: the report's index, which orders one
// rank's rows as well as its arrival does)
__global__ void k_ts_backfill(uint64_t b, uint64_t e, const TileStoreRow* rows, uint64_t arrival0, unsigned long long key_hi,
                              unsigned long long* keys) {
  const uint64_t k = b + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < e) keys[k] = key_hi | ((rows[k].arrival - arrival0) & 0xffffffffull);
}

// rows [at, at + n) of the gathered rows, taken from a one-rank snapshot (rule 17): call 0, keyed by
// their position in that store, whose order is arrival order
__global__ void k_ts_poskey(uint64_t n, uint64_t at, unsigned long long* keys) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) keys[at + k] = k & 0xffffffffull;
}

// the exchange (rule 16): the gathered rows whose file this rank writes (padding rows carry kTsPadKey)
__global__ void k_ts_own(uint64_t n, const TileStoreRow* rows, const unsigned long long* keys, int rank, int nranks,
                         unsigned long long* flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) flag[k] = (keys[k] != kTsPadKey && tile_file_owner(rows[k].bucket, rows[k].tile, nranks) == rank) ? 1ull : 0ull;
  else if (k == n) flag[n] = 0ull;   // the scan's last entry is the total
}
// ... their keys and gathered indices packed in gathered order (ranks in rank order, store order inside)
__global__ void k_ts_own_pack(uint64_t n, const unsigned long long* keys, const unsigned long long* flag,
                              const unsigned long long* ofs, unsigned long long* okey, uint32_t* oidx) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || !flag[k]) return;
  okey[ofs[k]] = keys[k];
  oidx[ofs[k]] = (uint32_t)k;
}
// ... and, sorted stably by key, into the store
__global__ void k_ts_take(uint64_t n, const uint32_t* idx, const unsigned long long* skey, const TileStoreRow* src,
                          TileStoreRow* rows, unsigned long long* keys, uint64_t cap) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || k >= cap) return;
  rows[k] = src[idx[k]];
  keys[k] = skey[k];
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
  // rule 16: the rows' keys beside them (cap of them once `keyed`, none before), the add calls
  // numbered from 0, and the calls whose rows are held without keys: {first row, first segment's
  // running number, call}
  DevBuf<unsigned long long> keys;
  bool keyed = false;
  uint64_t calls = 0;
  struct CallRec { uint64_t row0, arrival0, call; };
  std::vector<CallRec> unkeyed;
  uint64_t restored = 0;   // rows a snapshot put here: their calls are not known, so they cannot be keyed
  // the exchange: every rank's rows and keys as gathered, and its three parts' times
  DevBuf<TileStoreRow> grows; DevBuf<unsigned long long> gkeys; uint64_t g_cap = 0;
  PartTimer xtimer;
  double xms[3] = {0, 0, 0};
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
    if (keyed) keys.reserve(c, kFull, n_rows, st);   // (first: a full HBM here leaves rows and cap as they were)
    rows.reserve(c, kFull, n_rows, st);
    cap = c;
  }
  // From here on the store keeps a key per row; the rows it holds get theirs call by call.
  void make_keyed() {
    if (keyed) return;
    if (restored) throw std::runtime_error("tile store holds rows restored from a snapshot: they cannot take part in an exchange");
    keys.reserve(cap, kFull);
    keyed = true;
    for (size_t i = 0; i < unkeyed.size(); ++i) {
      const uint64_t b = unkeyed[i].row0, e = i + 1 < unkeyed.size() ? unkeyed[i + 1].row0 : n_rows;
      if (e > b)
        hipLaunchKernelGGL(k_ts_backfill, dim3(grid(e - b)), dim3(256), 0, st, b, e, (const TileStoreRow*)rows,
                           unkeyed[i].arrival0, (unsigned long long)(unkeyed[i].call << 32), keys);
    }
    RM_HIP(hipGetLastError());
    unkeyed.clear();
  }
  void ensure_gather(uint64_t n) {
    if (n <= g_cap) return;
    g_cap = 0;
    const uint64_t c = std::max<uint64_t>(n + n / 2, 4096);
    grows.reserve(c, kFull); gkeys.reserve(c, kFull);
    g_cap = c;
  }
  void begin_exchange() {
    xtimer.harvest(nullptr);
    for (double& x : xms) x = 0.0;
  }
  // The device half of the exchange behind its transport: of the n gathered rows (grows, gkeys;
  // this rank's own are [own_b, own_e)) those whose file this rank writes replace the store's
  // contents, merged by one stable sort on the key.  out[1..3]: sent away, received, held
  void merge_owned(uint64_t n, uint64_t own_b, uint64_t own_e, int nranks, int rank, uint64_t out[4]) {
    n_rows = 0;
    restored = 0;
    unkeyed.clear();
    uint64_t K = 0, own_kept = 0;
    if (n) {
      ensure_counts(n);
      ensure_flush(n);
      RM_HIP(hipMemsetAsync(ctr, 0, kTNumCtr * sizeof(unsigned long long), st));
      xtimer.tic(0, st);
      hipLaunchKernelGGL(k_ts_own, dim3(grid(n + 1)), dim3(256), 0, st, n, (const TileStoreRow*)grows,
                         (const unsigned long long*)gkeys, rank, nranks, cnt);
      scr.scan<unsigned long long>(cnt, ofs, n + 1, st);
      RM_HIP(hipMemcpyAsync(ctr + kTOwnLo, ofs + own_b, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
      RM_HIP(hipMemcpyAsync(ctr + kTOwnHi, ofs + own_e, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
      RM_HIP(hipMemcpyAsync(ctr + kTOwned, ofs + n, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
      xtimer.toc(st);
      RM_HIP(hipGetLastError());
      read_ctr();
      K = hctr[kTOwned];
      own_kept = hctr[kTOwnHi] - hctr[kTOwnLo];
      if (K > n || hctr[kTOwnHi] > K || hctr[kTOwnLo] > hctr[kTOwnHi]) throw std::runtime_error("tile store owned-row count out of range");
      ensure_rows(K);
      if (K) {
        xtimer.tic(0, st);
        hipLaunchKernelGGL(k_ts_own_pack, dim3(grid(n)), dim3(256), 0, st, n, (const unsigned long long*)gkeys,
                           (const unsigned long long*)cnt, (const unsigned long long*)ofs, k0, p0);
        xtimer.toc(st);
        xtimer.tic(2, st);
        scr.sort_pairs(k0.get(), k1.get(), p0, p1, K, 64, st);
        hipLaunchKernelGGL(k_ts_take, dim3(grid(K)), dim3(256), 0, st, K, (const uint32_t*)p1, (const unsigned long long*)k1,
                           (const TileStoreRow*)grows, rows, keys, cap);
        xtimer.toc(st);
        RM_HIP(hipGetLastError());
      }
    }
    RM_HIP(hipStreamSynchronize(st));
    xtimer.harvest(xms);
    n_rows = K;
    if (out) { out[1] = (own_e - own_b) - own_kept; out[2] = K - own_kept; out[3] = K; }
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
    if (calls >= 0xfffffffeull) throw std::runtime_error("tile store has numbered 2^32 - 2 add calls");
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
                         (const unsigned long long*)ofs, rows, n_rows, cap, arrivals, keyed ? keys.get() : nullptr,
                         (unsigned long long)(calls << 32));
      timer.toc(st);
      RM_HIP(hipGetLastError());
      RM_HIP(hipStreamSynchronize(st));
      timer.harvest(ms);
    }
    if (!keyed && total) unkeyed.push_back(CallRec{n_rows, arrivals, calls});
    n_rows += total;
    arrivals += n;
    calls += 1;
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
  if (s.keyed) throw std::runtime_error("snapshot: a tile store that keeps row keys (a sharded stream's) cannot be restored into");
  if (n_rows >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  s.ensure_rows(n_rows);
  return s.rows;
}
void TileStore::snapshot_loaded(uint64_t n_rows, uint64_t arrivals) {
  p_->n_rows = n_rows;
  p_->arrivals = arrivals;
  p_->restored = n_rows;
  p_->unkeyed.clear();
}

// a sharded stream's snapshot (DESIGN.md §3 rule 17)
uint64_t TileStore::calls() const { return p_->calls; }
const void* TileStore::snapshot_keys() {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  s.make_keyed();
  return s.keys;
}
void TileStore::snapshot_clear() {
  Impl& s = *p_;
  s.n_rows = 0; s.arrivals = 0; s.calls = 0; s.restored = 0;
  s.unkeyed.clear();
}
void TileStore::snapshot_merge(const void* const* rows, const void* const* keys, const uint64_t* counts, uint32_t n_parts,
                               int nranks, int rank, uint64_t calls, uint64_t arrivals) {
  Impl& s = *p_;
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("tile store import needs 0 <= rank < nranks");
  RM_HIP(hipSetDevice(s.device));
  if (s.n_rows) throw std::runtime_error("snapshot: the tile store is not empty");
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_parts; ++i) {
    total += counts[i];
    if (total >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  }
  s.make_keyed();
  s.begin_exchange();
  try {
    s.ensure_gather(total);
    s.xtimer.tic(1, s.st);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
      const uint64_t c = counts[i];
      if (!c) continue;
      RM_HIP(hipMemcpyAsync(s.grows + at, rows[i], c * sizeof(TileStoreRow), hipMemcpyDeviceToDevice, s.st));
      if (keys[i]) RM_HIP(hipMemcpyAsync(s.gkeys + at, keys[i], c * 8, hipMemcpyDeviceToDevice, s.st));
      else hipLaunchKernelGGL(k_ts_poskey, dim3(grid(c)), dim3(256), 0, s.st, c, at, s.gkeys);
      at += c;
    }
    s.xtimer.toc(s.st);
    RM_HIP(hipGetLastError());
    s.merge_owned(total, 0, 0, nranks, rank, nullptr);
  } catch (...) {
    snapshot_clear();
    throw;
  }
  s.calls = calls;
  s.arrivals = arrivals;
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
  s.add_device(SegSrc{s.dstage, (uint32_t)sizeof(TileSegment), nullptr, 0u}, n, out);
}

void TileStore::add_session(Session& sess, uint64_t out[4]) {
  Impl& s = *p_;
  if (sess.device() != s.device) throw std::runtime_error("the session is on another device than the tile store");
  RM_HIP(hipSetDevice(s.device));
  s.begin_call();
  // the session's calls return with their stream synchronised: rep_s is complete
  if (sess.sharded()) s.make_keyed();   // a sharded stream's rows carry rule 16's keys
  s.add_device(SegSrc{(const char*)sess.reports_device(), (uint32_t)sizeof(SessionReport), sess.windows_device(),
                      (uint32_t)sess.n_windows()}, sess.n_reports(), out);
}

bool TileStore::keyed() const { return p_->keyed; }
void TileStore::exchange_times(double ms[3]) const { for (int i = 0; i < 3; ++i) ms[i] = p_->xms[i]; }

// rule 16's two device halves.  The blob: kTsBlobHead bytes {magic, rows, quantisation, 0}, the rows
// in store order, their keys.
void TileStore::export_rows(char** blob_out, size_t* len_out) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  s.make_keyed();
  const uint64_t n = s.n_rows;
  const size_t len = kTsBlobHead + n * (sizeof(TileStoreRow) + 8);
  char* host = (char*)std::malloc(len);
  if (!host) throw std::bad_alloc();
  const uint64_t head[4] = {kTsBlobMagic, n, s.tp.quantisation, 0};
  std::memcpy(host, head, sizeof head);
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(host + kTsBlobHead, s.rows, n * sizeof(TileStoreRow), hipMemcpyDeviceToHost, s.st);
    if (e == hipSuccess) e = hipMemcpyAsync(host + kTsBlobHead + n * sizeof(TileStoreRow), s.keys, n * 8, hipMemcpyDeviceToHost, s.st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s.st);
  if (e != hipSuccess) {
    std::free(host);
    RM_HIP(e);
  }
  *blob_out = host;
  *len_out = len;
}

void TileStore::import_owned(const char* const* blobs, const size_t* lens, uint32_t n, int nranks, int rank, uint64_t out[4]) {
  Impl& s = *p_;
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("tile store import needs 0 <= rank < nranks");
  if (n && (!blobs || !lens)) throw std::runtime_error("tile store import: blobs or lens is NULL");
  RM_HIP(hipSetDevice(s.device));
  // every blob is checked before the store is touched
  uint64_t total = 0, own_b = 0, own_e = 0;
  std::vector<uint64_t> cnt(n);
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t head[4];
    if (!blobs[i] || lens[i] < kTsBlobHead) throw std::runtime_error("tile store import: blob " + std::to_string(i) + " is too short");
    std::memcpy(head, blobs[i], sizeof head);
    if (head[0] != kTsBlobMagic) throw std::runtime_error("tile store import: blob " + std::to_string(i) + " is no row export");
    if (head[1] >= kTsMaxRows || lens[i] != kTsBlobHead + head[1] * (sizeof(TileStoreRow) + 8))
      throw std::runtime_error("tile store import: blob " + std::to_string(i) + " has another length than its row count gives");
    if (head[2] != s.tp.quantisation) throw std::runtime_error("tile store import: blob " + std::to_string(i) + " has another quantisation");
    cnt[i] = head[1];
    if ((int)i == rank) { own_b = total; own_e = total + cnt[i]; }
    total += cnt[i];
    if (total >= kTsMaxRows) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  }
  if ((int)n <= rank) own_b = own_e = total;
  s.make_keyed();
  s.begin_exchange();
  const uint64_t before = s.n_rows;
  s.ensure_gather(total);
  s.xtimer.tic(1, s.st);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!cnt[i]) continue;
    const char* src = blobs[i] + kTsBlobHead;
    RM_HIP(hipMemcpyAsync(s.grows + at, src, cnt[i] * sizeof(TileStoreRow), hipMemcpyHostToDevice, s.st));
    RM_HIP(hipMemcpyAsync(s.gkeys + at, src + cnt[i] * sizeof(TileStoreRow), cnt[i] * 8, hipMemcpyHostToDevice, s.st));
    at += cnt[i];
  }
  s.xtimer.toc(s.st);
  RM_HIP(hipStreamSynchronize(s.st));   // (the blobs are the caller's pageable memory)
  if (out) out[0] = before;
  s.merge_owned(total, own_b, own_e, nranks, rank, out);
}

// export -> all-gather -> import with the rows staying on the device: padded to the largest rank's
// count (padding keys kTsPadKey), every rank's rows and keys gathered in rank order
void TileStore::exchange(TileComm& comm, uint64_t out[4]) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  s.make_keyed();
  s.begin_exchange();
  const uint64_t R = s.n_rows, nr = (uint64_t)comm.nranks;
  const uint64_t Rm = comm.max_u64(R, s.st);
  if (Rm < R || Rm * nr >= kTsMaxRows) throw BatchTooLarge("tile store exchange too large (rows of all ranks >= 2^31 - 1)");
  const uint64_t all = Rm * nr;
  if (out) out[0] = R;
  if (all) {
    s.ensure_rows(Rm);
    s.ensure_gather(all);
    s.xtimer.tic(1, s.st);
    if (Rm > R) {
      RM_HIP(hipMemsetAsync(s.rows + R, 0, (Rm - R) * sizeof(TileStoreRow), s.st));
      RM_HIP(hipMemsetAsync(s.keys + R, 0xff, (Rm - R) * 8, s.st));
    }
    comm.allgather(s.rows, s.grows, Rm * sizeof(TileStoreRow), s.st);
    comm.allgather(s.keys, s.gkeys, Rm * 8, s.st);
    s.xtimer.toc(s.st);
  }
  const uint64_t b = (uint64_t)comm.rank * Rm;
  s.merge_owned(all, b, b + R, comm.nranks, comm.rank, out);
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
  s.unkeyed.clear();
  s.restored = 0;
  *blob_out = host;
  *len_out = bytes;
  if (out) { out[0] = R; out[1] = K; out[2] = tiles; out[3] = files; out[4] = bytes; }
}

}  // namespace rm
