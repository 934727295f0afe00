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
                                                                 unsigned long long* chk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long c = 0ull;
  if (i < n) {
    const uint32_t e = snap::rec_bits(r, i, n_vehicles);
    if (e) atomicOr(chk, (unsigned long long)e);
    c = r[i].cnt;
  }
  block_add(chk + 1, c);
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

void snapshot_save(Session* s, Directory* d, TileStore* t, const char* user, size_t user_len, char** blob_out, size_t* len_out,
                   uint64_t out[6], double ms[6]) {
  if (user_len && !user) throw std::runtime_error("snapshot: user bytes are NULL");
  // (rule 16: the format has no section for row keys, and a restored store could not rejoin its ranks)
  if (t && t->keyed()) throw std::runtime_error("snapshot: a tile store that keeps row keys (a sharded stream's) cannot be saved");
  RM_HIP(hipSetDevice(common_device(s, d, t)));
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

void snapshot_load(Session* s, Directory* d, TileStore* t, const char* blob, size_t len, uint64_t out[6], double ms[6]) {
  RM_HIP(hipSetDevice(common_device(s, d, t)));
  // ---- the host's part: header, table, what the targets' sizes decide, and that they are empty
  snap::Table tb;
  const std::string why = snap::parse_table(blob, len, tb);
  if (!why.empty()) throw std::runtime_error(why);
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
    hipLaunchKernelGGL(k_snap_check_recs, dim3(grid(n_rec, kSumThreads)), dim3(kSumThreads), 0, st, recs, n_rec, s->n_vehicles(), chk);
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

}  // namespace rm
