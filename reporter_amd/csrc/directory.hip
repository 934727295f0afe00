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

inline uint32_t grid(uint64_t n, uint32_t b = 256) { return (uint32_t)std::max<uint64_t>((n + b - 1) / b, 1); }

__device__ __forceinline__ uint32_t dir_slot(unsigned long long h, uint32_t mask) {
  return (uint32_t)(((h ^ (h >> 29)) * 0x9e3779b97f4a7c15ull) >> 32) & mask;
}

__global__ void k_dir_fill(uint32_t n, uint32_t* v, uint32_t x) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) v[k] = x;
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
  DirTable t{};
  uint64_t arena_cap = 0, arena_used = 0;
  // per call (grow-only): ghash, found, isnew, nbytes, rank, aoff, map
  unsigned long long* ghash = nullptr;
  uint32_t* w[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t call_cap = 0;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint32_t* derr = nullptr;
  uint32_t* hctl = nullptr;   // pinned read-back words
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.0;

  void free_call() {
    if (ghash) (void)hipFree(ghash);
    for (uint32_t*& p : w) { if (p) (void)hipFree(p); p = nullptr; }
    ghash = nullptr;
    call_cap = 0;
  }
  void ensure_call(uint32_t G) {
    if (G + 1u <= call_cap) return;
    free_call();
    const uint32_t c = G + G / 2u + 256u;
    RM_HIP(hipMalloc((void**)&ghash, c * 8ull));
    for (uint32_t*& p : w) RM_HIP(hipMalloc((void**)&p, c * 4ull));
    call_cap = c;
  }
  void ensure_arena(uint64_t n, hipStream_t st) {
    if (n <= arena_cap) return;
    const uint64_t c = std::max<uint64_t>(n + n / 2, 1u << 16);
    uint8_t* a2 = nullptr;
    RM_HIP(hipMalloc((void**)&a2, c));
    if (arena_used) RM_HIP(hipMemcpyAsync(a2, t.arena, arena_used, hipMemcpyDeviceToDevice, st));
    RM_HIP(hipStreamSynchronize(st));
    if (t.arena) (void)hipFree(t.arena);
    t.arena = a2;
    arena_cap = c;
  }
  void scan(const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t st) {
    size_t b = 0;
    RM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, in, out, (int)n, st));
    if (b > tmp_bytes || !tmp) {
      if (tmp) { RM_HIP(hipStreamSynchronize(st)); (void)hipFree(tmp); tmp = nullptr; }
      tmp_bytes = b + b / 2 + 256;
      RM_HIP(hipMalloc(&tmp, tmp_bytes));
    }
    b = tmp_bytes;
    RM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, b, in, out, (int)n, st));
  }
  void release() {
    free_call();
    if (t.hash) (void)hipFree(t.hash);
    if (t.veh) (void)hipFree(t.veh);
    if (t.noff) (void)hipFree(t.noff);
    if (t.nlen) (void)hipFree(t.nlen);
    if (t.arena) (void)hipFree(t.arena);
    if (tmp) (void)hipFree(tmp);
    if (derr) (void)hipFree(derr);
    if (hctl) (void)hipHostFree(hctl);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

Directory::Directory(int device, uint32_t max_vehicles) : p_(new Impl) {
  Impl& s = *p_;
  try {
    if (max_vehicles == 0 || max_vehicles >= 0x40000000u) throw std::runtime_error("directory needs 1 .. 2^30 - 1 vehicles");
    s.device = device;
    s.max_vehicles = max_vehicles;
    RM_HIP(hipSetDevice(device));
    uint32_t cap = 64;
    while (cap < 2ull * max_vehicles) cap <<= 1;
    s.cap = cap;
    s.t.mask = cap - 1u;
    RM_HIP(hipMalloc((void**)&s.t.hash, cap * 8ull));
    RM_HIP(hipMalloc((void**)&s.t.veh, cap * 4ull));
    RM_HIP(hipMalloc((void**)&s.t.noff, cap * 4ull));
    RM_HIP(hipMalloc((void**)&s.t.nlen, cap * 4ull));
    RM_HIP(hipMalloc((void**)&s.derr, 8));
    RM_HIP(hipHostMalloc((void**)&s.hctl, 4 * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t& e : s.ev) RM_HIP(hipEventCreate(&e));
    RM_HIP(hipMemset(s.t.hash, 0, cap * 8ull));
    RM_HIP(hipMemset(s.t.noff, 0, cap * 4ull));
    RM_HIP(hipMemset(s.t.nlen, 0, cap * 4ull));
    RM_HIP(hipMemset(s.derr, 0, 8));
    hipLaunchKernelGGL(k_dir_fill, dim3(grid(cap)), dim3(256), 0, nullptr, cap, s.t.veh, kDirEmpty);
    RM_HIP(hipGetLastError());
    RM_HIP(hipDeviceSynchronize());
  } catch (...) {
    s.release();
    delete p_;
    throw;
  }
}

Directory::~Directory() {
  (void)hipSetDevice(p_->device);
  (void)hipDeviceSynchronize();
  p_->release();
  delete p_;
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
  const uint32_t G = g.n_groups;
  if (!g.n_points || !G) return;
  hipStream_t st = m.stream();
  s.ensure_call(G);
  uint32_t* found = s.w[0]; uint32_t* isnew = s.w[1]; uint32_t* nbytes = s.w[2];
  uint32_t* rank = s.w[3]; uint32_t* aoff = s.w[4]; uint32_t* map = s.w[5];
  RM_HIP(hipEventRecord(s.ev[0], st));
  RM_HIP(hipMemsetAsync(isnew + G, 0, 4, st));
  RM_HIP(hipMemsetAsync(nbytes + G, 0, 4, st));
  hipLaunchKernelGGL(k_dir_lookup, dim3(grid(G)), dim3(256), 0, st, G, g.text, g.v_off, g.v_len, g.hash_mask, s.t, s.ghash, found,
                     isnew, nbytes);
  RM_HIP(hipGetLastError());
  s.scan(isnew, rank, G + 1u, st);
  s.scan(nbytes, aoff, G + 1u, st);
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
                     (uint32_t)s.arena_used, s.arena_cap, s.t, map, s.derr);
  hipLaunchKernelGGL(k_dir_scatter, dim3(grid(g.n_points)), dim3(256), 0, st, g.n_points, G, (const uint32_t*)map, g.p_uuid);
  RM_HIP(hipGetLastError());
  RM_HIP(hipMemcpyAsync(s.hctl + 2, s.derr, 4, hipMemcpyDeviceToHost, st));
  RM_HIP(hipEventRecord(s.ev[1], st));
  RM_HIP(hipStreamSynchronize(st));
  if (s.hctl[2]) throw std::runtime_error("directory: an insert found no room (the table and the host disagree)");
  s.n_known += n_new;
  s.arena_used += new_bytes;
  float t = 0.f;
  if (hipEventElapsedTime(&t, s.ev[0], s.ev[1]) == hipSuccess) s.ms = t;
}

uint64_t Directory::name_bytes() const { return p_->arena_used; }

void Directory::snapshot_gather(unsigned long long* d_off, uint8_t* d_bytes, hipStream_t st) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  hipLaunchKernelGGL(k_dir_snap_off, dim3(grid(s.cap)), dim3(256), 0, st, s.cap, s.t, s.n_known, (unsigned long long)s.arena_used, d_off);
  RM_HIP(hipGetLastError());
  if (s.arena_used) RM_HIP(hipMemcpyAsync(d_bytes, s.t.arena, s.arena_used, hipMemcpyDeviceToDevice, st));
}

void Directory::snapshot_insert(uint32_t n, const unsigned long long* d_off, const uint8_t* d_bytes, uint64_t n_bytes,
                                unsigned long long* d_err, uint32_t dup_bit, hipStream_t st) {
  Impl& s = *p_;
  RM_HIP(hipSetDevice(s.device));
  if (s.n_known) throw std::runtime_error("snapshot: the directory is not empty");
  if (n > s.max_vehicles) throw std::runtime_error("snapshot: more names than the directory's max_vehicles");
  if (n_bytes >= (1ull << 32)) throw std::runtime_error("directory names pass 2^32 bytes");
  if (!n) return;
  if (n_bytes > s.arena_cap) {   // (ensure_arena, with a full HBM reported as the workspaces report it)
    const uint64_t c = std::max<uint64_t>(n_bytes + n_bytes / 2, 1u << 16);
    uint8_t* a2 = nullptr;
    const hipError_t e = hipMalloc((void**)&a2, c);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      throw BatchTooLarge("directory names do not fit in HBM");
    }
    RM_HIP(e);
    RM_HIP(hipStreamSynchronize(st));
    if (s.t.arena) (void)hipFree(s.t.arena);
    s.t.arena = a2;
    s.arena_cap = c;
  }
  if (n_bytes) RM_HIP(hipMemcpyAsync(s.t.arena, d_bytes, n_bytes, hipMemcpyDeviceToDevice, st));
  const unsigned long long hmask = lines_hash_mask();
  RM_HIP(hipMemsetAsync(s.derr, 0, 4, st));
  hipLaunchKernelGGL(k_dir_snap_insert, dim3(grid(n)), dim3(256), 0, st, n, d_off, hmask, s.t, s.derr);
  hipLaunchKernelGGL(k_dir_snap_verify, dim3(grid(n)), dim3(256), 0, st, n, d_off, hmask, s.t, d_err, 1ull << dup_bit);
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
  hipLaunchKernelGGL(k_dir_fill, dim3(grid(s.cap)), dim3(256), 0, st, s.cap, s.t.veh, kDirEmpty);
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
  RM_HIP(hipMemcpy(veh.data(), s.t.veh, s.cap * 4ull, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(noff.data(), s.t.noff, s.cap * 4ull, hipMemcpyDeviceToHost));
  RM_HIP(hipMemcpy(nlen.data(), s.t.nlen, s.cap * 4ull, hipMemcpyDeviceToHost));
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
  if (bytes && total) RM_HIP(hipMemcpy(bytes, s.t.arena + o[0], total, hipMemcpyDeviceToHost));
  return total;
}

}  // namespace rm
