// snapshot.hip — the stream snapshot (DESIGN.md §3 rule 15; layout, checksum and rule: snapshot.hpp):
// the vehicle sessions, the vehicle directory and the tile store saved into one blob and restored
// from it, so that a stream stopped anywhere and continued from the blob gives the output of the
// stream that never stopped.
//
//   save   the session packs its store (Session::snapshot_pack: get_store's append of nothing) and
//          ranks its non-empty vehicles; k_snap_recs compacts them into records by that rank; the
//          points, the names (Directory::snapshot_gather) and the rows are copied device to device
//          into one buffer laid out as the blob; k_snap_sum adds every section's checksum into
//          its table entry in that buffer; one download; the host writes header and table.
//   load   the host checks header and table (snap::parse_table) and what depends on the targets'
//          sizes; one upload; k_snap_sum and the k_snap_check_* kernels read only inside the
//          sections the table names and write only the check block {error bits, cnt sum, sums};
//          one read of that block; only with no bit set: room in the targets, the names inserted
//          under this process's hash mask (Directory::snapshot_insert; two equal names are the
//          one error that shows here, and the directory is emptied again), the records scattered,
//          cnt scanned into off, the points and rows copied in, veh[] found by a search over off.
//
//   shards (rule 17) save_shard is save with the rows' keys and the shard record as two more
//          sections.  load_shards takes the M blobs of one save into what one rank of N holds:
//          all blobs in one buffer, checked as above blob by blob; k_shard_own marks every
//          record's vehicle (twice: an error), writes every cnt for the scan that places each
//          record's points among all blobs', and sums what the loading rank owns; then the rows and
//          keys of all blobs through the tile store's own partition and merge
//          (TileStore::snapshot_merge), the names, k_shard_scatter of the owned records by
//          vehicle, the scan of cnt into off, and k_shard_gather, a thread per point of the new store.
//
// One stream (the session's, else the tile store's), HIP events per part.  Nothing here loops
// over points, vehicles, names or rows on the host.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>

#include "engine.hpp"
#include "snapshot.hpp"
#include "tile_text.hpp"

namespace rm {

namespace {

static_assert(sizeof(TileStoreRow) == snap::kRowBytes, "a tile section's element is TileStoreRow");

constexpr uint32_t kSumThreads = 256;
constexpr uint32_t kSumUnits = kSumThreads * 4u;   // 16-byte units of a block: 16 KiB
constexpr uint32_t kMaxSecs = snap::kNumKinds;

struct SumSecs {   // the sections of one k_snap_sum launch, by value
  uint32_t n;
  uint32_t first_block[kMaxSecs + 1];
  unsigned long long off[kMaxSecs], bytes[kMaxSecs], dst[kMaxSecs];   // dst: byte offset of the u64 that takes the sum
};

// the block's values summed into *dst by one atomic: shuffles inside each wave, LDS across the waves
__device__ __forceinline__ void block_add(unsigned long long* dst, unsigned long long v) {
  __shared__ unsigned long long part[kSumThreads / 64];
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) part[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long t = 0ull;
    for (uint32_t w = 0; w < blockDim.x / 64u; ++w) t += part[w];
    if (t) atomicAdd(dst, t);
  }
}

// snap::checksum of every section at once: a block takes 16 KiB of one section in 16-byte loads
// (sections are 16-byte aligned and zero-padded to 16 inside the buffer); a word counts only
// where it starts inside the section's bytes
__global__ void __launch_bounds__(kSumThreads) k_snap_sum(const uint8_t* blob, SumSecs s, uint8_t* dst_base) {
  uint32_t k = 0;
  while (k + 1u < s.n && blockIdx.x >= s.first_block[k + 1u]) ++k;
  const unsigned long long bytes = s.bytes[k];
  const unsigned long long units = (bytes + 15ull) >> 4;
  const uint4* p = (const uint4*)(blob + s.off[k]);
  const unsigned long long u0 = (unsigned long long)(blockIdx.x - s.first_block[k]) * kSumUnits + threadIdx.x;
  unsigned long long acc = 0ull;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    const unsigned long long u = u0 + (unsigned long long)j * kSumThreads;
    if (u >= units) break;
    const uint4 x = p[u];
    const unsigned long long w0 = (unsigned long long)x.x | ((unsigned long long)x.y << 32);
    const unsigned long long w1 = (unsigned long long)x.z | ((unsigned long long)x.w << 32);
    acc += snap::sum_word(w0, 2ull * u);
    if ((2ull * u + 1ull) * 8ull < bytes) acc += snap::sum_word(w1, 2ull * u + 1ull);
  }
  block_add((unsigned long long*)(dst_base + s.dst[k]), acc);
}

// ---- save
__global__ void k_snap_recs(SessionSnap v, snap::SessRec* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.n_vehicles) return;
  const uint32_t c = v.cnt[i];
  if (!c) return;
  const uint32_t r = v.rank[i];
  if (r >= v.n_live) return;
  snap::SessRec x;
  x.vehicle = i; x.cnt = c; x.max_sep = v.max_sep[i]; x.pad = 0u; x.last_update = v.last_update[i];
  out[r] = x;
}

// ---- load: the checks (chk[0] error bits, chk[1] the sum of cnt)
__global__ void __launch_bounds__(kSumThreads) k_snap_check_recs(const snap::SessRec* r, uint64_t n, uint32_t n_vehicles,
                                                                 unsigned long long* chk, unsigned long long* cnt_sum) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long c = 0ull;
  if (i < n) {
    const uint32_t e = snap::rec_bits(r, i, n_vehicles);
    if (e) atomicOr(chk, (unsigned long long)e);
    c = r[i].cnt;
  }
  block_add(cnt_sum, c);
}
__global__ void k_snap_check_times(const double* t, uint64_t n, unsigned long long* chk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = snap::time_bits(t[i]);
  if (e) atomicOr(chk, (unsigned long long)e);
}
__global__ void k_snap_check_names(const unsigned long long* off, uint64_t n, uint64_t n_bytes, unsigned long long* chk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = snap::name_bits((const uint64_t*)off, i, n, n_bytes);
  if (e) atomicOr(chk, (unsigned long long)e);
}

// ---- load: the unpack.  A record's vehicle gets the state k_sess_trigger leaves between calls.
__global__ void k_snap_scatter(const snap::SessRec* r, uint32_t n, SessionSnap v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const snap::SessRec x = r[i];
  if (x.vehicle >= v.n_vehicles) return;   // (checked: rec_bits)
  const uint32_t at = x.cnt > 1u ? x.cnt : 1u;
  v.cnt[x.vehicle] = x.cnt; v.max_sep[x.vehicle] = x.max_sep; v.last_update[x.vehicle] = x.last_update;
  v.scan_from[x.vehicle] = at; v.try_from[x.vehicle] = at;
}
// point q belongs to the last vehicle whose off is <= q (empty vehicles share their successor's off)
__global__ void k_snap_point_veh(uint64_t n, SessionSnap v) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t lo = 0u, hi = v.n_vehicles;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v.off[mid] <= q) lo = mid; else hi = mid;
  }
  v.veh[q] = lo;
  v.arr[q] = kNone;
}

// ---- load of shards (rule 17).  The blobs lie end to end in one buffer; record j of all blobs'
// records (in the order given) belongs to blob b with rec0[b] <= j < rec0[b + 1], whose points are
// the global points [pt0[b], pt0[b + 1]).
struct ShardBlobs {
  uint32_t n;
  uint32_t rec0[snap::kMaxRanks + 1];
  unsigned long long pt0[snap::kMaxRanks + 1];
  unsigned long long recs[snap::kMaxRanks], lon[snap::kMaxRanks], lat[snap::kMaxRanks], acc[snap::kMaxRanks],
      time[snap::kMaxRanks];   // byte offsets of the sections in the buffer
};
__device__ __forceinline__ uint32_t blob_of_rec(const ShardBlobs& sb, uint32_t j) {
  uint32_t b = 0;
  while (b + 1u < sb.n && j >= sb.rec0[b + 1u]) ++b;
  return b;
}
__device__ __forceinline__ uint32_t blob_of_point(const ShardBlobs& sb, unsigned long long g) {
  uint32_t b = 0;
  while (b + 1u < sb.n && g >= sb.pt0[b + 1u]) ++b;
  return b;
}
__global__ void k_snap_check_keys(const unsigned long long* key, uint64_t n, unsigned long long* chk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = snap::key_bits(key[i]);
  if (e) atomicOr(chk, (unsigned long long)e);
}
// Every record of every blob: its cnt into all[j] (the scan gives its points' global start), its
// vehicle marked in seen[] (a second mark is the error bit), and the cnt of the records whose
// vehicle the loading rank owns summed into *own_sum.  Writes scratch and the check block alone.
__global__ void __launch_bounds__(kSumThreads) k_shard_own(const uint8_t* buf, ShardBlobs sb, uint32_t n, uint32_t n_vehicles,
                                                           int rank, int nranks, uint32_t* all, uint32_t* seen,
                                                           unsigned long long* chk, unsigned long long* own_sum) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long c = 0ull;
  if (j < n) {
    const uint32_t b = blob_of_rec(sb, j);
    const snap::SessRec x = ((const snap::SessRec*)(buf + sb.recs[b]))[j - sb.rec0[b]];
    all[j] = x.cnt;
    if (x.vehicle < n_vehicles) {   // (else: rec_bits has set its bit)
      if (atomicExch(seen + x.vehicle, 1u)) atomicOr(chk, 1ull << snap::kEVehTwice);
      if (vehicle_owner(x.vehicle, nranks) == rank) c = (1ull << 32) | x.cnt;   // (all points < 2^32: records above, points below)
    }
  } else if (j == n) {
    all[n] = 0u;   // the scan's last entry is the total
  }
  block_add(own_sum, c);
}
// the owned records scattered by vehicle, as k_snap_scatter does, and where their points lie
__global__ void k_shard_scatter(const uint8_t* buf, ShardBlobs sb, uint32_t n, const uint32_t* start, int rank, int nranks,
                                SessionSnap v, uint32_t* src) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t b = blob_of_rec(sb, j);
  const snap::SessRec x = ((const snap::SessRec*)(buf + sb.recs[b]))[j - sb.rec0[b]];
  if (x.vehicle >= v.n_vehicles || vehicle_owner(x.vehicle, nranks) != rank) return;
  const uint32_t at = x.cnt > 1u ? x.cnt : 1u;
  v.cnt[x.vehicle] = x.cnt; v.max_sep[x.vehicle] = x.max_sep; v.last_update[x.vehicle] = x.last_update;
  v.scan_from[x.vehicle] = at; v.try_from[x.vehicle] = at;
  src[x.vehicle] = start[j];
}
// The segmented gather: point q of the new store belongs to the last vehicle whose off is <= q
// (k_snap_point_veh) and is that vehicle's point q - off in its blob's range.
__global__ void k_shard_gather(const uint8_t* buf, ShardBlobs sb, uint64_t n, const uint32_t* src, SessionSnap v) {
  const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  uint32_t lo = 0u, hi = v.n_vehicles;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v.off[mid] <= q) lo = mid; else hi = mid;
  }
  const unsigned long long g = (unsigned long long)src[lo] + (q - v.off[lo]);
  const uint32_t b = blob_of_point(sb, g);
  const unsigned long long i = g - sb.pt0[b];
  if (g >= sb.pt0[sb.n] || i >= sb.pt0[b + 1u] - sb.pt0[b]) return;   // (cannot happen: the cnt sums are checked)
  v.lon[q] = ((const float*)(buf + sb.lon[b]))[i];
  v.lat[q] = ((const float*)(buf + sb.lat[b]))[i];
  v.acc[q] = ((const float*)(buf + sb.acc[b]))[i];
  v.time[q] = ((const double*)(buf + sb.time[b]))[i];
  v.veh[q] = lo;
  v.arr[q] = kNone;
}

constexpr const char* kSnapFull = "the snapshot does not fit in HBM";

// a call's part times into its ms[6] (null: dropped), after a stream synchronise
void read_parts(PartTimer& ev, double ms[6]) {
  if (ms) for (int k = 0; k < 6; ++k) ms[k] = 0.0;
  ev.harvest(ms);
}

void launch_sum(const uint8_t* blob, const std::vector<snap::Entry>& ent, const std::vector<uint64_t>& dst, uint8_t* dst_base,
                hipStream_t st) {
  SumSecs s{};
  uint32_t blocks = 0;
  for (size_t k = 0; k < ent.size() && s.n < kMaxSecs; ++k) {
    if (!ent[k].bytes) continue;
    const uint64_t units = (ent[k].bytes + 15) / 16;
    s.first_block[s.n] = blocks;
    s.off[s.n] = ent[k].off; s.bytes[s.n] = ent[k].bytes; s.dst[s.n] = dst[k];
    blocks += (uint32_t)((units + kSumUnits - 1) / kSumUnits);
    ++s.n;
  }
  s.first_block[s.n] = blocks;
  if (!blocks) return;
  hipLaunchKernelGGL(k_snap_sum, dim3(blocks), dim3(kSumThreads), 0, st, blob, s, dst_base);
  RM_HIP(hipGetLastError());
}

int common_device(Session* s, Directory* d, TileStore* t) {
  int dev = -1;
  for (int x : {s ? s->device() : -1, d ? d->device() : -1, t ? t->device() : -1}) {
    if (x < 0) continue;
    if (dev >= 0 && x != dev) throw std::runtime_error("snapshot: the objects are on different devices");
    dev = x;
  }
  if (dev < 0) throw std::runtime_error("snapshot: session, directory and tile store are all NULL");
  return dev;
}

}  // namespace

namespace {

// shard null: the plain save; else the saving rank's record, and the store's keys go along (rule 17)
void save_any(Session* s, Directory* d, TileStore* t, const snap::ShardRec* shard, const char* user, size_t user_len,
              char** blob_out, size_t* len_out, uint64_t out[6], double ms[6]) {
  if (user_len && !user) throw std::runtime_error("snapshot: user bytes are NULL");
  // (the plain blob has no section for row keys: a keyed store is saved by rm_snapshot_save_shard)
  if (!shard && t && t->keyed())
    throw std::runtime_error("snapshot: a tile store that keeps row keys (a sharded stream's) cannot be saved");
  RM_HIP(hipSetDevice(common_device(s, d, t)));
  const void* keys = shard ? t->snapshot_keys() : nullptr;   // (before the store's stream is waited for)
  if (t) RM_HIP(hipStreamSynchronize(t->stream()));
  SessionSnap v;
  hipStream_t st = s ? s->stream() : (t ? t->stream() : nullptr);
  PartTimer ev;
  ev.tic(0, st);   // pack: the store as get_store packs it, the non-empty vehicles ranked
  if (s) v = s->snapshot_pack();
  ev.toc(st);   // (the pack synchronises and reads its counts back: the pair spans that read, and no more)
  const uint32_t n_names = d ? d->size() : 0u;
  const uint64_t name_bytes = d ? d->name_bytes() : 0, n_rows = t ? t->rows_held() : 0;
  if (v.n_points >= 0xffffffffull) throw BatchTooLarge("session store too large (points >= 2^32)");
  snap::Writer w;
  if (user_len) w.add(snap::kUser, nullptr, user_len);
  if (d) { w.add(snap::kDirOff, nullptr, n_names + 1ull); w.add(snap::kDirBytes, nullptr, name_bytes); }
  if (s) {
    w.add(snap::kSessRec, nullptr, v.n_live);
    for (uint32_t k : {(uint32_t)snap::kSessLon, (uint32_t)snap::kSessLat, (uint32_t)snap::kSessAcc, (uint32_t)snap::kSessTime})
      w.add(k, nullptr, v.n_points);
  }
  if (t) { w.add(snap::kTileRows, nullptr, n_rows); w.add(snap::kTileMeta, nullptr, 1); }
  if (shard) { w.add(snap::kTileKeys, nullptr, n_rows); w.add(snap::kShardRec, nullptr, 1); }
  const uint64_t len = w.layout();
  DevBuf<uint8_t> buf;
  buf.reserve(std::max<uint64_t>(len, 16), kSnapFull);
  uint8_t* b = buf;
  char* host = (char*)std::malloc(len);
  if (!host) throw std::bad_alloc();
  try {
    snap::TileMeta meta{};
    ev.tic(1, st);   // gather: records by rank, points, names and rows into the blob's layout
    RM_HIP(hipMemsetAsync(b, 0, len, st));
    std::vector<uint64_t> dst(w.ent.size());
    for (size_t k = 0; k < w.ent.size(); ++k) {
      const snap::Entry& e = w.ent[k];
      dst[k] = sizeof(snap::Header) + k * sizeof(snap::Entry) + offsetof(snap::Entry, sum);
      uint8_t* at = b + e.off;
      const void* src = nullptr;
      switch (e.kind) {
        case snap::kUser: RM_HIP(hipMemcpyAsync(at, user, user_len, hipMemcpyHostToDevice, st)); break;
        case snap::kDirOff: d->snapshot_gather((unsigned long long*)at, b + w.ent[k + 1].off, st); break;
        case snap::kDirBytes: break;   // (with the offsets)
        case snap::kSessRec:
          if (v.n_live) hipLaunchKernelGGL(k_snap_recs, dim3(grid(v.n_vehicles)), dim3(256), 0, st, v, (snap::SessRec*)at);
          break;
        case snap::kSessLon: src = v.lon; break;
        case snap::kSessLat: src = v.lat; break;
        case snap::kSessAcc: src = v.acc; break;
        case snap::kSessTime: src = v.time; break;
        case snap::kTileRows: src = t->rows_device(); break;
        case snap::kTileMeta:
          meta.arrivals = t->arrivals(); meta.quantisation = t->quantisation();
          RM_HIP(hipMemcpyAsync(at, &meta, sizeof meta, hipMemcpyHostToDevice, st));
          break;
        case snap::kTileKeys: src = keys; break;
        case snap::kShardRec: RM_HIP(hipMemcpyAsync(at, shard, sizeof *shard, hipMemcpyHostToDevice, st)); break;
        default: break;
      }
      if (src && e.bytes) RM_HIP(hipMemcpyAsync(at, src, e.bytes, hipMemcpyDeviceToDevice, st));
    }
    RM_HIP(hipGetLastError());
    ev.toc(st);
    ev.tic(2, st);   // checksum: every section's sum into its table entry in the buffer
    launch_sum(b, w.ent, dst, b, st);
    ev.toc(st);
    ev.tic(3, st);   // the one download
    RM_HIP(hipMemcpyAsync(host, b, len, hipMemcpyDeviceToHost, st));
    ev.toc(st);
    RM_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < w.ent.size(); ++k) std::memcpy(&w.ent[k].sum, host + dst[k], 8);
    w.seal(host, len);
  } catch (...) {
    std::free(host);
    throw;
  }
  read_parts(ev, ms);
  *blob_out = host;
  *len_out = len;
  if (out) { out[0] = len; out[1] = n_names; out[2] = v.n_live; out[3] = v.n_points; out[4] = n_rows; out[5] = user_len; }
}

}  // namespace

void snapshot_save(Session* s, Directory* d, TileStore* t, const char* user, size_t user_len, char** blob_out, size_t* len_out,
                   uint64_t out[6], double ms[6]) {
  save_any(s, d, t, nullptr, user, user_len, blob_out, len_out, out, ms);
}

void snapshot_save_shard(Session* s, Directory* d, TileStore* t, int rank, int nranks, const char* user, size_t user_len,
                         char** blob_out, size_t* len_out, uint64_t out[6], double ms[6]) {
  if (!t) throw std::runtime_error("snapshot: a shard is saved with its tile store");
  if (nranks < 1 || nranks > (int)snap::kMaxRanks || rank < 0 || rank >= nranks)
    throw std::runtime_error("snapshot: a shard needs 0 <= rank < nranks <= 16");
  snap::ShardRec rec{};
  rec.rank = (uint32_t)rank; rec.nranks = (uint32_t)nranks; rec.calls = (uint32_t)t->calls();
  save_any(s, d, t, &rec, user, user_len, blob_out, len_out, out, ms);
}

void snapshot_load(Session* s, Directory* d, TileStore* t, const char* blob, size_t len, uint64_t out[6], double ms[6]) {
  RM_HIP(hipSetDevice(common_device(s, d, t)));
  // ---- the host's part: header, table, what the targets' sizes decide, and that they are empty
  snap::Table tb;
  const std::string why = snap::parse_table(blob, len, tb);
  if (!why.empty()) throw std::runtime_error(why);
  if (tb.has[snap::kShardRec])
    throw std::runtime_error("snapshot: it carries row keys and a shard record (a sharded stream's): load it with rm_snapshot_load_shards");
  if (s && !tb.has[snap::kSessRec]) throw std::runtime_error("snapshot: it holds no sessions");
  if (d && !tb.has[snap::kDirOff]) throw std::runtime_error("snapshot: it holds no directory");
  if (t && !tb.has[snap::kTileRows]) throw std::runtime_error("snapshot: it holds no tile rows");
  const std::string why2 = snap::check_targets(blob, tb, s ? s->n_vehicles() : 0u, d ? d->max_vehicles() : 0u, t ? t->quantisation() : 0u);
  if (!why2.empty()) throw std::runtime_error(why2);
  if (d && d->size()) throw std::runtime_error("snapshot: the directory is not empty");
  if (t && t->rows_held()) throw std::runtime_error("snapshot: the tile store is not empty");
  if (t) RM_HIP(hipStreamSynchronize(t->stream()));
  hipStream_t st = s ? s->stream() : (t ? t->stream() : nullptr);
  if (s && s->snapshot_pack().n_points) throw std::runtime_error("snapshot: the session is not empty");
  PartTimer ev;
  // ---- one upload, the checksums and the checks; they write the check block alone
  std::vector<snap::Entry> ent;
  std::vector<uint64_t> dst;
  for (uint32_t k = 1; k < snap::kNumKinds; ++k)
    if (tb.has[k]) { ent.push_back(tb.ent[k]); dst.push_back((2 + ent.size() - 1) * 8); }
  DevBuf<uint8_t> buf;
  DevBuf<unsigned long long> chk_mem;
  buf.reserve(std::max<uint64_t>(len, 16), kSnapFull);
  chk_mem.reserve(32, kSnapFull);
  const uint8_t* b = buf;
  unsigned long long* chk = chk_mem;
  unsigned long long h[32];
  ev.tic(0, st);
  RM_HIP(hipMemcpyAsync(buf, blob, len, hipMemcpyHostToDevice, st));
  ev.toc(st);
  ev.tic(1, st);
  RM_HIP(hipMemsetAsync(chk, 0, 32 * 8, st));
  launch_sum(b, ent, dst, (uint8_t*)chk, st);
  const uint64_t n_rec = tb.vehicles(), n_pts = tb.points(), n_names = tb.names(), n_rows = tb.rows();
  const snap::SessRec* recs = (const snap::SessRec*)(b + tb.ent[snap::kSessRec].off);
  const unsigned long long* noff = (const unsigned long long*)(b + tb.ent[snap::kDirOff].off);
  if (s && n_rec)
    hipLaunchKernelGGL(k_snap_check_recs, dim3(grid(n_rec, kSumThreads)), dim3(kSumThreads), 0, st, recs, n_rec, s->n_vehicles(), chk, chk + 1);
  if (s && n_pts)
    hipLaunchKernelGGL(k_snap_check_times, dim3(grid(n_pts)), dim3(256), 0, st, (const double*)(b + tb.ent[snap::kSessTime].off), n_pts, chk);
  if (d && n_names)
    hipLaunchKernelGGL(k_snap_check_names, dim3(grid(n_names)), dim3(256), 0, st, noff, n_names, tb.ent[snap::kDirBytes].bytes, chk);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(h, chk, 32 * 8, hipMemcpyDeviceToHost, st));
  ev.toc(st);
  RM_HIP(hipStreamSynchronize(st));
  uint64_t bits = h[0];
  for (size_t k = 0; k < ent.size(); ++k)
    if (h[2 + k] != ent[k].sum) bits |= 1ull << snap::kESum;
  if (s && h[1] != n_pts) bits |= 1ull << snap::kECntSum;
  if (bits) throw std::runtime_error(snap::first_message(bits));
  // ---- the unpack: room first (a full HBM shows before anything is written), the names, the rest
  SessionSnap v;
  void* rows = nullptr;
  ScanScratch scr("the snapshot's scan does not fit in HBM");
  if (s) {
    v = s->snapshot_room(n_pts);
    scr.presize<false>(v.n_vehicles, st);
  }
  if (t) rows = t->snapshot_room(n_rows);
  ev.tic(2, st);
  if (d) {
    d->snapshot_insert((uint32_t)n_names, noff, b + tb.ent[snap::kDirBytes].off, tb.ent[snap::kDirBytes].bytes, chk, snap::kEDupName, st);
    RM_HIP(hipMemcpyAsync(h, chk, 8, hipMemcpyDeviceToHost, st));
    RM_HIP(hipStreamSynchronize(st));
    if (h[0]) {
      d->snapshot_clear(st);
      throw std::runtime_error(snap::first_message(h[0]));
    }
  }
  try {
    if (s) {
      if (n_rec) hipLaunchKernelGGL(k_snap_scatter, dim3(grid(n_rec)), dim3(256), 0, st, recs, (uint32_t)n_rec, v);
      scr.scan<uint32_t>(v.cnt, v.off, v.n_vehicles, st);
      if (n_pts) {
        RM_HIP(hipMemcpyAsync(v.lon, b + tb.ent[snap::kSessLon].off, n_pts * 4, hipMemcpyDeviceToDevice, st));
        RM_HIP(hipMemcpyAsync(v.lat, b + tb.ent[snap::kSessLat].off, n_pts * 4, hipMemcpyDeviceToDevice, st));
        RM_HIP(hipMemcpyAsync(v.acc, b + tb.ent[snap::kSessAcc].off, n_pts * 4, hipMemcpyDeviceToDevice, st));
        RM_HIP(hipMemcpyAsync(v.time, b + tb.ent[snap::kSessTime].off, n_pts * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_snap_point_veh, dim3(grid(n_pts)), dim3(256), 0, st, n_pts, v);
      }
    }
    if (t && n_rows) RM_HIP(hipMemcpyAsync(rows, b + tb.ent[snap::kTileRows].off, n_rows * snap::kRowBytes, hipMemcpyDeviceToDevice, st));
    RM_HIP(hipGetLastError());
    ev.toc(st);
    RM_HIP(hipStreamSynchronize(st));
  } catch (...) {   // written in part: every target goes back to empty (the store's rows do not count until snapshot_loaded)
    if (d) { try { d->snapshot_clear(st); } catch (...) {} }
    if (s) { try { s->snapshot_clear(); } catch (...) {} }
    throw;
  }
  if (s) s->snapshot_loaded(n_pts);
  if (t) t->snapshot_loaded(n_rows, snap::tile_meta(blob, tb).arrivals);
  read_parts(ev, ms);
  if (out) { out[0] = len; out[1] = n_names; out[2] = n_rec; out[3] = n_pts; out[4] = n_rows; out[5] = tb.ent[snap::kUser].bytes; }
}

// Rule 17's load: what `rank` of `nranks` holds of the state that M ranks saved.
void snapshot_load_shards(Session* s, Directory* d, TileStore* t, const char* const* blobs, const size_t* lens, uint32_t n,
                          int rank, int nranks, uint64_t out[8], double ms[6]) {
  RM_HIP(hipSetDevice(common_device(s, d, t)));
  if (nranks < 1 || nranks > (int)snap::kMaxRanks || rank < 0 || rank >= nranks)
    throw std::runtime_error("snapshot: a shard needs 0 <= rank < nranks <= 16");
  if (n < 1 || n > snap::kMaxRanks || !blobs || !lens) throw std::runtime_error("snapshot: a load of shards takes 1 .. 16 blobs");
  // ---- the host's part: every header and table, then what the blobs must agree on
  std::vector<snap::Table> tb(n);
  std::vector<snap::ShardRec> rec(n);
  for (uint32_t i = 0; i < n; ++i) {
    const std::string at = " (blob " + std::to_string(i) + ")";
    if (!blobs[i]) throw std::runtime_error("snapshot: blob is NULL" + at);
    const std::string why = snap::parse_table(blobs[i], lens[i], tb[i]);
    if (!why.empty()) throw std::runtime_error(why + at);
    if (!tb[i].has[snap::kShardRec]) {
      if (n > 1) throw std::runtime_error("snapshot: a blob without a shard record is loaded alone" + at);
      rec[i] = snap::ShardRec{0u, 1u, 1u, 0u};   // a one-rank blob: rank 0 of 1, its rows are call 0's
    } else {
      rec[i] = snap::shard_rec(blobs[i], tb[i]);
      const uint32_t e = snap::shard_bits(rec[i]);
      if (e) throw std::runtime_error(snap::first_message(e) + at);
    }
    if (s && !tb[i].has[snap::kSessRec]) throw std::runtime_error("snapshot: it holds no sessions" + at);
    if (d && !tb[i].has[snap::kDirOff]) throw std::runtime_error("snapshot: it holds no directory" + at);
    if (t && !tb[i].has[snap::kTileRows]) throw std::runtime_error("snapshot: it holds no tile rows" + at);
  }
  // blob i is rank order[rec.rank]'s: every rank of the save once
  std::vector<int> of_rank(n, -1);
  for (uint32_t i = 0; i < n; ++i) {
    if (rec[i].nranks != n)
      throw std::runtime_error("snapshot: blob " + std::to_string(i) + " is of a save of " + std::to_string(rec[i].nranks) +
                               " ranks, and " + std::to_string(n) + " blobs are given (one of the set is missing, or one too many)");
    if (of_rank[rec[i].rank] >= 0)
      throw std::runtime_error("snapshot: rank " + std::to_string(rec[i].rank) + " of the save is given twice");
    of_rank[rec[i].rank] = (int)i;
  }
  for (uint32_t i = 1; i < n; ++i)
    if (rec[i].calls != rec[0].calls) throw std::runtime_error("snapshot: the blobs are of different stops (their add-call counters differ)");
  for (uint32_t i = 0; i < n; ++i) {
    const std::string why = snap::check_targets(blobs[i], tb[i], s ? s->n_vehicles() : 0u, d ? d->max_vehicles() : 0u, t ? t->quantisation() : 0u);
    if (!why.empty()) throw std::runtime_error(why);
    if (!d || i == 0) continue;
    for (uint32_t k : {(uint32_t)snap::kDirOff, (uint32_t)snap::kDirBytes}) {
      const snap::Entry &a = tb[0].ent[k], &b = tb[i].ent[k];
      if (a.bytes != b.bytes || a.count != b.count || a.sum != b.sum)
        throw std::runtime_error("snapshot: the blobs' directories differ (the directory is replicated)");
    }
  }
  uint64_t total_len = 0, all_rec = 0, all_pts = 0, all_rows = 0;
  for (uint32_t i = 0; i < n; ++i) {
    total_len += lens[i]; all_rec += tb[i].vehicles(); all_pts += tb[i].points(); all_rows += tb[i].rows();
  }
  if (s && (all_pts >= 0xffffffffull || all_rec >= 0x7fffffffull)) throw BatchTooLarge("session store too large (points >= 2^32)");
  if (t && all_rows >= 0x7fffffffull) throw BatchTooLarge("tile store too large (rows >= 2^31 - 1)");
  if (d && d->size()) throw std::runtime_error("snapshot: the directory is not empty");
  if (t && t->rows_held()) throw std::runtime_error("snapshot: the tile store is not empty");
  if (t) RM_HIP(hipStreamSynchronize(t->stream()));
  hipStream_t st = s ? s->stream() : (t ? t->stream() : nullptr);
  if (s && s->snapshot_pack().n_points) throw std::runtime_error("snapshot: the session is not empty");
  PartTimer ev;
  // ---- one buffer for all blobs (in the order given), the checksums and the checks; they write
  // the check block {error bits, owned cnt sum, cnt sum per blob, section sums per blob} and scratch alone
  constexpr uint32_t kChkSum0 = 2u + snap::kMaxRanks, kChkWords = kChkSum0 + snap::kMaxRanks * snap::kNumKinds;
  DevBuf<uint8_t> buf;
  DevBuf<unsigned long long> chk_mem;
  DevBuf<uint32_t> all_cnt, start;
  buf.reserve(std::max<uint64_t>(total_len, 16), kSnapFull);
  chk_mem.reserve(kChkWords, kSnapFull);
  if (s) { all_cnt.reserve(all_rec + 1, kSnapFull); start.reserve(all_rec + 1, kSnapFull); }
  ScanScratch scr("the snapshot's scan does not fit in HBM");
  SessionSnap v;
  if (s) {
    v = s->snapshot_room(0);
    scr.presize<false>(std::max<uint64_t>(v.n_vehicles, all_rec + 1), st);
  }
  const uint8_t* b = buf;
  unsigned long long* chk = chk_mem;
  std::vector<unsigned long long> h(kChkWords);
  std::vector<uint64_t> base(n);
  ShardBlobs sb{};
  sb.n = n;
  ev.tic(0, st);
  {
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
      base[i] = at;
      RM_HIP(hipMemcpyAsync(buf + at, blobs[i], lens[i], hipMemcpyHostToDevice, st));
      sb.rec0[i + 1] = sb.rec0[i] + (uint32_t)tb[i].vehicles();
      sb.pt0[i + 1] = sb.pt0[i] + tb[i].points();
      sb.recs[i] = at + tb[i].ent[snap::kSessRec].off;
      sb.lon[i] = at + tb[i].ent[snap::kSessLon].off; sb.lat[i] = at + tb[i].ent[snap::kSessLat].off;
      sb.acc[i] = at + tb[i].ent[snap::kSessAcc].off; sb.time[i] = at + tb[i].ent[snap::kSessTime].off;
      at += lens[i];
    }
  }
  ev.toc(st);
  ev.tic(1, st);
  RM_HIP(hipMemsetAsync(chk, 0, kChkWords * 8, st));
  std::vector<std::vector<snap::Entry>> ent(n);
  for (uint32_t i = 0; i < n; ++i) {
    std::vector<uint64_t> dst;
    for (uint32_t k = 1; k < snap::kNumKinds; ++k)
      if (tb[i].has[k]) { ent[i].push_back(tb[i].ent[k]); dst.push_back((kChkSum0 + i * snap::kNumKinds + ent[i].size() - 1) * 8); }
    launch_sum(b + base[i], ent[i], dst, (uint8_t*)chk, st);
    const uint64_t n_rec = tb[i].vehicles(), n_pts = tb[i].points(), n_rows = tb[i].rows();
    if (s && n_rec)
      hipLaunchKernelGGL(k_snap_check_recs, dim3(grid(n_rec, kSumThreads)), dim3(kSumThreads), 0, st,
                         (const snap::SessRec*)(b + sb.recs[i]), n_rec, s->n_vehicles(), chk, chk + 2 + i);
    if (s && n_pts)
      hipLaunchKernelGGL(k_snap_check_times, dim3(grid(n_pts)), dim3(256), 0, st, (const double*)(b + sb.time[i]), n_pts, chk);
    if (t && n_rows && tb[i].has[snap::kTileKeys])
      hipLaunchKernelGGL(k_snap_check_keys, dim3(grid(n_rows)), dim3(256), 0, st,
                         (const unsigned long long*)(b + base[i] + tb[i].ent[snap::kTileKeys].off), n_rows, chk);
  }
  const uint64_t n_names = tb[0].names();
  const unsigned long long* noff = (const unsigned long long*)(b + base[0] + tb[0].ent[snap::kDirOff].off);
  const uint8_t* nbytes = b + base[0] + tb[0].ent[snap::kDirBytes].off;
  if (d && n_names)
    hipLaunchKernelGGL(k_snap_check_names, dim3(grid(n_names)), dim3(256), 0, st, noff, n_names, tb[0].ent[snap::kDirBytes].bytes, chk);
  if (s) {
    RM_HIP(hipMemsetAsync(v.rank, 0, (v.n_vehicles + 1ull) * 4, st));
    hipLaunchKernelGGL(k_shard_own, dim3(grid(all_rec + 1, kSumThreads)), dim3(kSumThreads), 0, st, b, sb, (uint32_t)all_rec,
                       v.n_vehicles, rank, nranks, all_cnt.get(), v.rank, chk, chk + 1);
    scr.scan<uint32_t>(all_cnt, start, all_rec + 1, st);
  }
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(h.data(), chk, kChkWords * 8, hipMemcpyDeviceToHost, st));
  ev.toc(st);
  RM_HIP(hipStreamSynchronize(st));
  uint64_t bits = h[0];
  for (uint32_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < ent[i].size(); ++k)
      if (h[kChkSum0 + i * snap::kNumKinds + k] != ent[i][k].sum) bits |= 1ull << snap::kESum;
    if (s && h[2 + i] != tb[i].points()) bits |= 1ull << snap::kECntSum;
  }
  if (bits) throw std::runtime_error(snap::first_message(bits));
  const uint64_t own_pts = s ? h[1] & 0xffffffffull : 0, own_rec = s ? h[1] >> 32 : 0;
  if (own_pts > all_pts || own_rec > all_rec) throw std::runtime_error("snapshot: owned point count out of range");
  // ---- the unpack: room first (a full HBM shows before anything is written), the rows through
  // the exchange's merge on the store's own stream, the names, the sessions
  uint64_t held = 0;
  if (s) v = s->snapshot_room(own_pts);
  const auto undo = [&] {
    if (d) { try { d->snapshot_clear(st); } catch (...) {} }
    if (s) { try { s->snapshot_clear(); } catch (...) {} }
    if (t) t->snapshot_clear();
  };
  double rows_ms[3] = {0, 0, 0};
  if (t) {
    const void* prow[snap::kMaxRanks];
    const void* pkey[snap::kMaxRanks];
    uint64_t cnt[snap::kMaxRanks];
    uint64_t arrivals = 0;
    for (uint32_t r = 0; r < n; ++r) {   // in rank order
      const uint32_t i = (uint32_t)of_rank[r];
      prow[r] = b + base[i] + tb[i].ent[snap::kTileRows].off;
      pkey[r] = tb[i].has[snap::kTileKeys] ? b + base[i] + tb[i].ent[snap::kTileKeys].off : nullptr;
      cnt[r] = tb[i].rows();
      arrivals = std::max<uint64_t>(arrivals, snap::tile_meta(blobs[i], tb[i]).arrivals);
    }
    t->snapshot_merge(prow, pkey, cnt, n, nranks, rank, rec[0].calls, arrivals);   // (a throw leaves the store empty)
    t->exchange_times(rows_ms);
    held = t->rows_held();
  }
  ev.tic(2, st);
  try {
    if (d) {
      d->snapshot_insert((uint32_t)n_names, noff, nbytes, tb[0].ent[snap::kDirBytes].bytes, chk, snap::kEDupName, st);
      RM_HIP(hipMemcpyAsync(h.data(), chk, 8, hipMemcpyDeviceToHost, st));
      RM_HIP(hipStreamSynchronize(st));
      if (h[0]) throw std::runtime_error(snap::first_message(h[0]));
    }
    if (s) {
      if (all_rec)
        hipLaunchKernelGGL(k_shard_scatter, dim3(grid(all_rec)), dim3(256), 0, st, b, sb, (uint32_t)all_rec, (const uint32_t*)start,
                           rank, nranks, v, v.rank);
      scr.scan<uint32_t>(v.cnt, v.off, v.n_vehicles, st);
      if (own_pts) hipLaunchKernelGGL(k_shard_gather, dim3(grid(own_pts)), dim3(256), 0, st, b, sb, own_pts, (const uint32_t*)v.rank, v);
    }
    RM_HIP(hipGetLastError());
    ev.toc(st);
    RM_HIP(hipStreamSynchronize(st));
  } catch (...) {   // written in part: every target goes back to empty
    undo();
    throw;
  }
  if (s) {
    s->snapshot_loaded(own_pts);
    s->snapshot_sharded();
  }
  read_parts(ev, ms);
  if (ms) ms[3] = rows_ms[0] + rows_ms[1] + rows_ms[2];
  if (out) {
    out[0] = total_len; out[1] = d ? n_names : 0; out[2] = own_rec; out[3] = own_pts; out[4] = held;
    out[5] = tb[0].ent[snap::kUser].bytes; out[6] = rec[0].calls; out[7] = n;
  }
}

}  // namespace rm
