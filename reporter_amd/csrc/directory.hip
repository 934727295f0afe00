// directory.hip — the vehicle directory (DESIGN.md §3 rule 14): the map from vehicle id bytes to a
// dense index that holds for a whole stream, where rule 11's numbering holds for one call.
//
//   table     open addressing with linear probing in HBM, a power-of-two capacity of at least
//             2 * max_vehicles; per slot the (masked) FNV-1a hash, the vehicle, and the name's offset
//             and length in a grow-only arena of name bytes.  Nothing is ever removed.
//   assign    the line reader has left the call's ids as groups in first-seen order with a name
//             span each (lines.hip k_id_rank, or the host's numbering after a shared hash):
//               k_dir_lookup   one lane per group hashes its name and probes: hash, length, bytes;
//                              an equal hash with other bytes continues the probe
//               scans          over "not found" and over the new names' bytes, in first-seen order:
//                              new indices n_known + rank, arena offsets
//               (host)         the two totals come back; a call that would pass max_vehicles or
//                              the arena's 2^32 bytes fails here, before anything is written
//               k_dir_insert   one lane per new group copies its name into the arena, claims an
//                              empty slot with a compare-and-swap on the vehicle word, writes the rest
//               k_dir_scatter  every point's per-call number becomes its directory index
// Lookups and inserts are separate kernels, so a lookup never sees a half-written slot.  Which slot
// a name lands in may depend on timing; no output depends on slots.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "engine.hpp"

namespace rm {

namespace {

constexpr uint32_t kDirEmpty = 0xffffffffu;

struct DirTable {
  unsigned long long* hash;
  uint32_t* veh;
  uint32_t* noff;
  uint32_t* nlen;
  uint32_t mask;   // capacity - 1
  uint8_t* arena;
};

__device__ __forceinline__ uint32_t dir_slot(unsigned long long h, uint32_t mask) {
  return (uint32_t)(((h ^ (h >> 29)) * 0x9e3779b97f4a7c15ull) >> 32) & mask;
}

// per group: the masked hash, the vehicle found (kDirEmpty: new), and the scans' inputs (entry G
// of either is zeroed by the host: the scans' last entries are the totals)
__global__ void k_dir_lookup(uint32_t G, const uint8_t* text, const uint32_t* v_off, const uint32_t* v_len,
                             unsigned long long hmask, DirTable t, unsigned long long* ghash, uint32_t* found, uint32_t* isnew,
                             uint32_t* nbytes) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint32_t n = v_len[g];
  const uint8_t* s = text + v_off[g];
  const unsigned long long h = sv::id_hash(s, n) & hmask;
  uint32_t slot = dir_slot(h, t.mask), res = kDirEmpty;
  for (uint32_t probe = 0; probe <= t.mask; ++probe) {
    const uint32_t v = t.veh[slot];
    if (v == kDirEmpty) break;
    if (t.hash[slot] == h && t.nlen[slot] == n) {
      const uint8_t* q = t.arena + t.noff[slot];
      bool same = true;
      for (uint32_t i = 0; same && i < n; ++i) same = q[i] == s[i];
      if (same) { res = v; break; }
    }
    slot = (slot + 1u) & t.mask;
  }
  ghash[g] = h;
  found[g] = res;
  isnew[g] = res == kDirEmpty ? 1u : 0u;
  nbytes[g] = res == kDirEmpty ? n : 0u;
}

// map[g]: the directory index of the call's group g
__global__ void k_dir_insert(uint32_t G, const uint8_t* text, const uint32_t* v_off, const uint32_t* v_len,
                             const unsigned long long* ghash, const uint32_t* found, const uint32_t* rank, const uint32_t* aoff,
                             uint32_t n_known, uint32_t max_vehicles, uint32_t arena_used, uint64_t arena_cap, DirTable t,
                             uint32_t* map, uint32_t* err) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  if (found[g] != kDirEmpty) { map[g] = found[g]; return; }
  const uint32_t idx = n_known + rank[g], n = v_len[g];
  const uint64_t a = (uint64_t)arena_used + aoff[g];
  if (idx >= max_vehicles || a + n > arena_cap) { err[0] = 1u; map[g] = kDirEmpty; return; }   // (the host has checked both)
  const uint8_t* s = text + v_off[g];
  for (uint32_t i = 0; i < n; ++i) t.arena[a + i] = s[i];
  uint32_t slot = dir_slot(ghash[g], t.mask);
  bool placed = false;
  for (uint32_t probe = 0; probe <= t.mask; ++probe) {
    if (atomicCAS(t.veh + slot, kDirEmpty, idx) == kDirEmpty) {
      t.hash[slot] = ghash[g]; t.noff[slot] = (uint32_t)a; t.nlen[slot] = n;
      placed = true;
      break;
    }
    slot = (slot + 1u) & t.mask;
  }
  if (!placed) err[0] = 1u;
  map[g] = idx;
}

__global__ void k_dir_scatter(uint64_t P, uint32_t G, const uint32_t* map, uint32_t* p_uuid) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  const uint32_t u = p_uuid[k];
  p_uuid[k] = u < G ? map[u] : kDirEmpty;
}

// ---- the stream snapshot (DESIGN.md §3 rule 15) ----
// the arena holds the names in index order, so a name's arena offset is its snapshot offset
__global__ void k_dir_snap_off(uint32_t cap, DirTable t, uint32_t n_known, unsigned long long arena_used, unsigned long long* off) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0u) off[n_known] = arena_used;
  if (k >= cap) return;
  const uint32_t v = t.veh[k];
  if (v != kDirEmpty && v < n_known) off[v] = t.noff[k];
}

// name k of a snapshot takes index k: its bytes lie in the arena at off[k] already
__global__ void k_dir_snap_insert(uint32_t n, const unsigned long long* off, unsigned long long hmask, DirTable t, uint32_t* err) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t a = (uint32_t)off[k], len = (uint32_t)(off[k + 1] - off[k]);
  const unsigned long long h = sv::id_hash(t.arena + a, len) & hmask;
  uint32_t slot = dir_slot(h, t.mask);
  for (uint32_t probe = 0; probe <= t.mask; ++probe) {
    if (atomicCAS(t.veh + slot, kDirEmpty, k) == kDirEmpty) {
      t.hash[slot] = h; t.noff[slot] = a; t.nlen[slot] = len;
      return;
    }
    slot = (slot + 1u) & t.mask;
  }
  err[0] = 1u;
}

// ... and must be the first of its bytes that a lookup finds: of two equal names one is not
__global__ void k_dir_snap_verify(uint32_t n, const unsigned long long* off, unsigned long long hmask, DirTable t,
                                  unsigned long long* snap_err, unsigned long long dup) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
  const uint8_t* s = t.arena + (uint32_t)off[k];
  const unsigned long long h = sv::id_hash(s, len) & hmask;
  uint32_t slot = dir_slot(h, t.mask), res = kDirEmpty;
  for (uint32_t probe = 0; probe <= t.mask; ++probe) {
    const uint32_t v = t.veh[slot];
    if (v == kDirEmpty) break;
    if (t.hash[slot] == h && t.nlen[slot] == len) {
      const uint8_t* q = t.arena + t.noff[slot];
      bool same = true;
      for (uint32_t i = 0; same && i < len; ++i) same = q[i] == s[i];
      if (same) { res = v; break; }
    }
    slot = (slot + 1u) & t.mask;
  }
  if (res != k) atomicOr(snap_err, dup);
}

}  // namespace

struct Directory::Impl {
  int device = 0;
  uint32_t max_vehicles = 0, cap = 0, n_known = 0;
  // the table and the arena of names
  DevBuf<unsigned long long> hash;
  DevBuf<uint32_t> veh, noff, nlen;
  DevBuf<uint8_t> arena;
  uint64_t arena_cap = 0, arena_used = 0;
  // per call (grow-only): ghash, found, isnew, nbytes, rank, aoff, map
  DevBuf<unsigned long long> ghash;
  DevBuf<uint32_t> w[6];
  uint32_t call_cap = 0;
  ScanScratch scr;
  DevBuf<uint32_t> derr;
  PinBuf<uint32_t> hctl;   // pinned read-back words
  PartTimer timer;
  double ms = 0.0;

  DirTable table() const { return DirTable{hash, veh, noff, nlen, cap - 1u, arena}; }
  void ensure_call(uint32_t G) {
    if (G + 1u <= call_cap) return;
    call_cap = 0;
    const uint32_t c = G + G / 2u + 256u;
    ghash.reserve(c);
    for (DevBuf<uint32_t>& p : w) p.reserve(c);
    call_cap = c;
  }
  // room for n name bytes, the names held moving by a device copy; a full HBM is reported as
  // too_large where the caller names one (as the workspaces report it)
  void ensure_arena(uint64_t n, hipStream_t st, const char* too_large = nullptr) {
    if (n <= arena_cap) return;
    const uint64_t c = std::max<uint64_t>(n + n / 2, 1u << 16);
    arena.reserve(c, too_large, arena_used, st);
    arena_cap = c;
  }
};

Directory::Directory(int device, uint32_t max_vehicles) : p_(new Impl) {
  Impl& s = *p_;
  if (max_vehicles == 0 || max_vehicles >= 0x40000000u) throw std::runtime_error("directory needs 1 .. 2^30 - 1 vehicles");
  s.device = device;
  s.max_vehicles = max_vehicles;
  RM_HIP(hipSetDevice(device));
  uint32_t cap = 64;
  while (cap < 2ull * max_vehicles) cap <<= 1;
  s.cap = cap;
  s.hash.reserve(cap); s.veh.reserve(cap); s.noff.reserve(cap); s.nlen.reserve(cap);
  s.derr.reserve(2);
  s.hctl.reserve(4);
  RM_HIP(hipMemset(s.hash, 0, cap * 8ull));
  RM_HIP(hipMemset(s.noff, 0, cap * 4ull));
  RM_HIP(hipMemset(s.nlen, 0, cap * 4ull));
  RM_HIP(hipMemset(s.derr, 0, 8));
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(cap)), dim3(256), 0, nullptr, cap, s.veh, kDirEmpty);
  RM_HIP(hipGetLastError());
  RM_HIP(hipDeviceSynchronize());
}

Directory::~Directory() {
  (void)hipSetDevice(p_->device);
  (void)hipDeviceSynchronize();
}

uint32_t Directory::size() const { return p_->n_known; }
uint32_t Directory::max_vehicles() const { return p_->max_vehicles; }
int Directory::device() const { return p_->device; }
double Directory::last_ms() const { return p_->ms; }

void Directory::assign(Matcher& m) {
  Impl& s = *p_;
  if (m.device() != s.device) throw std::runtime_error("the directory is on another device than the runner");
  RM_HIP(hipSetDevice(s.device));
  const LineGroups g = m.line_groups();
  s.ms = 0.0;
  s.timer.harvest(nullptr);   // (a pair a call that threw left behind)
  const uint32_t G = g.n_groups;
  if (!g.n_points || !G) return;
  hipStream_t st = m.stream();
  s.ensure_call(G);
  uint32_t* found = s.w[0]; uint32_t* isnew = s.w[1]; uint32_t* nbytes = s.w[2];
  uint32_t* rank = s.w[3]; uint32_t* aoff = s.w[4]; uint32_t* map = s.w[5];
  s.timer.tic(0, st);
  RM_HIP(hipMemsetAsync(isnew + G, 0, 4, st));
  RM_HIP(hipMemsetAsync(nbytes + G, 0, 4, st));
  hipLaunchKernelGGL(k_dir_lookup, dim3(grid(G)), dim3(256), 0, st, G, g.text, g.v_off, g.v_len, g.hash_mask, s.table(), s.ghash, found,
                     isnew, nbytes);
  RM_HIP(hipGetLastError());
  s.scr.scan(isnew, rank, G + 1u, st);
  s.scr.scan(nbytes, aoff, G + 1u, st);
  RM_HIP(hipMemcpyAsync(s.hctl + 0, rank + G, 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipMemcpyAsync(s.hctl + 1, aoff + G, 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  const uint32_t n_new = s.hctl[0];
  const uint64_t new_bytes = s.hctl[1];
  // the fullness check, before anything is written
  if ((uint64_t)s.n_known + n_new > s.max_vehicles) throw std::runtime_error("directory full");
  if (s.arena_used + new_bytes >= (1ull << 32)) throw std::runtime_error("directory names pass 2^32 bytes");
  if (n_new) s.ensure_arena(s.arena_used + new_bytes, st);
  hipLaunchKernelGGL(k_dir_insert, dim3(grid(G)), dim3(256), 0, st, G, g.text, g.v_off, g.v_len, (const unsigned long long*)s.ghash,
                     (const uint32_t*)found, (const uint32_t*)rank, (const uint32_t*)aoff, s.n_known, s.max_vehicles,
                     (uint32_t)s.arena_used, s.arena_cap, s.table(), map, s.derr);
  hipLaunchKernelGGL(k_dir_scatter, dim3(grid(g.n_points)), dim3(256), 0, st, g.n_points, G, (const uint32_t*)map, g.p_uuid);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(s.hctl + 2, s.derr, 4, hipMemcpyDeviceToHost, st));
  s.timer.toc(st);
  RM_HIP(hipStreamSynchronize(st));
  if (s.hctl[2]) throw std::runtime_error("directory: an insert found no room (the table and the host disagree)");
  s.n_known += n_new;
  s.arena_used += new_bytes;
  s.timer.harvest(&s.ms);
}

uint64_t Directory::name_bytes() const { return p_->arena_used; }

void Directory::snapshot_gather(unsigned long long* d_off, uint8_t* d_bytes, hipStream_t st) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  hipLaunchKernelGGL(k_dir_snap_off, dim3(grid(s.cap)), dim3(256), 0, st, s.cap, s.table(), s.n_known, (unsigned long long)s.arena_used, d_off);
  RM_HIP(hipGetLastError());
  if (s.arena_used) RM_HIP(hipMemcpyAsync(d_bytes, s.arena, s.arena_used, hipMemcpyDeviceToDevice, st));
}

void Directory::snapshot_insert(uint32_t n, const unsigned long long* d_off, const uint8_t* d_bytes, uint64_t n_bytes,
                                unsigned long long* d_err, uint32_t dup_bit, hipStream_t st) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  if (s.n_known) throw std::runtime_error("snapshot: the directory is not empty");
  if (n > s.max_vehicles) throw std::runtime_error("snapshot: more names than the directory's max_vehicles");
  if (n_bytes >= (1ull << 32)) throw std::runtime_error("directory names pass 2^32 bytes");
  if (!n) return;
  s.ensure_arena(n_bytes, st, "directory names do not fit in HBM");   // (the directory is empty: nothing moves)
  if (n_bytes) RM_HIP(hipMemcpyAsync(s.arena, d_bytes, n_bytes, hipMemcpyDeviceToDevice, st));
  const unsigned long long hmask = lines_hash_mask();
  RM_HIP(hipMemsetAsync(s.derr, 0, 4, st));
  hipLaunchKernelGGL(k_dir_snap_insert, dim3(grid(n)), dim3(256), 0, st, n, d_off, hmask, s.table(), s.derr);
  hipLaunchKernelGGL(k_dir_snap_verify, dim3(grid(n)), dim3(256), 0, st, n, d_off, hmask, s.table(), d_err, 1ull << dup_bit);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(s.hctl + 2, s.derr, 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipStreamSynchronize(st));
  if (s.hctl[2]) {
    snapshot_clear(st);
    throw std::runtime_error("directory: an insert found no room (the table and the host disagree)");
  }
  s.n_known = n;
  s.arena_used = n_bytes;
}

void Directory::snapshot_clear(hipStream_t st) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  hipLaunchKernelGGL(k_fill<uint32_t>, dim3(grid(s.cap)), dim3(256), 0, st, s.cap, s.veh, kDirEmpty);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemsetAsync(s.derr, 0, 8, st));
  RM_HIP(hipStreamSynchronize(st));
  s.n_known = 0;
  s.arena_used = 0;
}

uint64_t Directory::names(uint32_t first, uint32_t n, uint64_t* off, char* bytes) {
  Impl& s = *p_;
  if ((uint64_t)first + n > s.n_known) throw std::runtime_error("directory names: range past its size");
  RM_HIP(hipSetDevice(s.device));
  // the slots in vehicle order (a diagnostic path: the table comes to the host whole)
  std::vector<uint32_t> veh(s.cap), noff(s.cap), nlen(s.cap);
  RM_HIP(hipMemcpy(veh.data(), s.veh, s.cap * 4ull, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(noff.data(), s.noff, s.cap * 4ull, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(nlen.data(), s.nlen, s.cap * 4ull, hipMemcpyDeviceToHost));
  std::vector<uint32_t> o(n, 0), l(n, 0);
  for (uint32_t k = 0; k < s.cap; ++k) {
    if (veh[k] == kDirEmpty || veh[k] < first || veh[k] >= first + n) continue;
    o[veh[k] - first] = noff[k];
    l[veh[k] - first] = nlen[k];
  }
  // the arena holds the names in vehicle order (its offsets come from a scan in that order), so a
  // range of vehicles is one range of bytes
  uint64_t total = 0;
  for (uint32_t v = 0; v < n; ++v) {
    if (off) off[v] = total;
    if (n && o[v] != o[0] + total) throw std::runtime_error("directory names: the arena is out of order");
    total += l[v];
  }
  if (off) off[n] = total;
  if (bytes && total) RM_HIP(hipMemcpy(bytes, s.arena + o[0], total, hipMemcpyDeviceToHost));
  return total;
}

}  // namespace rm
