// tile_cull.hpp — the privacy cull of the tile stages (stages.hip Matcher::tiles over TileRow,
// tilestore.hip TileStore::flush over TileStoreRow): over rows sorted by (file, id, next_id), the
// runs of equal (file, id, next_id), the keep rule per run, the keep flag per row.  The rule is a
// __host__ __device__ function free of HIP types, so the host program tests/cpp/tile_cull_test.cpp
// runs exactly the code the kernels run.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TC_HD __host__ __device__ __forceinline__
#else
#define TC_HD static inline
#endif

namespace rm {

// The reference's cull loop (simple_reporter.py:221-239; AnonymisingProcessor.java:155-175 clean()
// is the same loop) as a rule over the G runs of the sorted rows: run g, of size(g) rows, is kept
// iff it has >= privacy rows, except that the loop's end-of-list step closes the open run together
// with the final row, so a final run of one row that is not its file's only run shares the fate of
// the run before it, and the two are judged on their joint size (pinned by
// tests/golden/tiles_golden.json).  same_file(x, y): runs x and y lie in one file.
template <class Size, class SameFile>
TC_HD bool tile_run_kept(uint32_t g, uint32_t G, Size size, SameFile same_file, uint32_t privacy) {
  auto file_last = [&](uint32_t x) { return x + 1 == G || !same_file(x + 1, x); };
  auto file_first = [&](uint32_t x) { return x == 0 || !same_file(x - 1, x); };
  const uint32_t sz = size(g);
  bool k = sz >= privacy;
  if (file_last(g) && sz == 1 && !file_first(g)) k = size(g - 1) + 1 >= privacy;
  if (!file_last(g) && file_last(g + 1) && size(g + 1) == 1) k = sz + 1 >= privacy;
  return k;
}

#if defined(__HIP__) || defined(__HIPCC__)

// starts of the runs of equal (file, id, next_id) in sorted order; SameFile()(a, b): rows of one file
template <class SameFile, class Row>
__global__ void k_cull_gflags(uint64_t n, const Row* rows, const uint32_t* perm, uint32_t* flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const SameFile same{};
  uint32_t f = 1u;
  if (k > 0) {
    const Row& a = rows[perm[k - 1]];
    const Row& b = rows[perm[k]];
    f = (!same(a, b) || a.id != b.id || a.next_id != b.next_id) ? 1u : 0u;
  }
  flag[k] = f;
}

// gid: the exclusive scan of flag.  gpos[g]: the first row of run g (gpos[G] = n); *runs = G
template <class Ctr>
__global__ void k_cull_gpos(uint64_t n, const uint32_t* flag, const uint32_t* gid, uint32_t* gpos, Ctr* runs) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (flag[k]) gpos[gid[k]] = (uint32_t)k;
  if (k + 1 == n) {
    const uint32_t G = gid[k] + flag[k];
    gpos[G] = (uint32_t)n;
    *runs = G;
  }
}

// tile_run_kept per run; with kCountFiles also the files held, one atomic per block into *files
template <class SameFile, bool kCountFiles, class Row>
__global__ void k_cull_gkeep(uint32_t G, const Row* rows, const uint32_t* perm, const uint32_t* gpos, uint32_t privacy,
                             uint8_t* keep, unsigned long long* files) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const SameFile same{};
  auto same_file = [&](uint32_t x, uint32_t y) { return same(rows[perm[gpos[x]]], rows[perm[gpos[y]]]); };
  if (g < G) keep[g] = tile_run_kept(g, G, [&](uint32_t x) { return gpos[x + 1] - gpos[x]; }, same_file, privacy) ? 1 : 0;
  if constexpr (kCountFiles) {
    const int n = __syncthreads_count(g < G && (g == 0 || !same_file(g - 1, g)) ? 1 : 0);
    if (threadIdx.x == 0 && n) atomicAdd(files, (unsigned long long)n);
  }
}

template <class Keep>
__global__ void k_cull_kflags(uint64_t n, const uint32_t* gid, const uint32_t* gfl, const Keep* keep, uint32_t* flag) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) flag[k] = keep[gid[k] + gfl[k] - 1u];   // exclusive scan of run starts -> run of k
}

#endif

}  // namespace rm
