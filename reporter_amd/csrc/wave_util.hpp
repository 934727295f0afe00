// wave_util.hpp — the device helpers K4 (engine.hip k_seg_wave) and the matched-edges stage
// (edges.hip) share: ballot-mask searches, the wave scan, the lane read, and the two rules that
// make a matched edge's times bit-equal to its segment's (the fp64 operation order of
// interp_time, the chain test over transition slots).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rm {

// rule 6's time of route distance x of D between the two state times (the oracle's operation order)
__device__ __forceinline__ double interp_time(double ta, double tb, uint64_t x, uint64_t D) {
  if (D == 0) return ta;
  return ta + (tb - ta) * ((double)x / (double)D);
}

__device__ __forceinline__ bool same_chain(uint32_t slot_prev, uint32_t slot_next) {
  // traversal records of a chain come from consecutive transition slots; traces are
  // at least two slots apart, so this also separates traces
  return slot_next == slot_prev || slot_next == slot_prev + 1;
}

__device__ __forceinline__ int hi_le(unsigned long long m, int i) {   // highest set bit <= i, or -1
  if (i < 0) return -1;
  const unsigned long long mm = m & ((2ull << i) - 1ull);
  return mm ? 63 - __builtin_clzll(mm) : -1;
}
__device__ __forceinline__ int lo_gt(unsigned long long m, int i) {   // lowest set bit > i, or 64
  const unsigned long long mm = m & ~((2ull << i) - 1ull);
  return mm ? __builtin_ctzll(mm) : 64;
}
__device__ __forceinline__ unsigned long long wave_incl_sum(unsigned long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
// value of v in lane src (clamped to 0).  Called with every lane active: a bpermute under a
// divergent condition reads nothing from the lanes the condition switched off.
template <class T>
__device__ __forceinline__ T at_lane(T v, int src) { return __shfl(v, src < 0 ? 0 : src, 64); }

}  // namespace rm
