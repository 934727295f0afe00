// inflate_ring.hpp — the sink k_inflate (inflate.hip) decodes into: a 32 KiB window ring, flushed
// a half at a time to the chunk's slot and into the member's CRC-32, counting on past the slot's
// end without storing.  On the device one wave owns a ring and every lane runs this code with its
// own `ln`.  On the host the same code runs the 64 lanes one after the other inside each step
// (a step is what the wave does in lockstep: all reads of a match copy before its writes), so
// tests/cpp/inflate_core_test.cpp puts the ring arithmetic under the sanitizers: every ring index,
// every slot store, every slice of the CRC.
#pragma once
#include "inflate_core.hpp"

#if defined(__HIP__) || defined(__HIPCC__)
#define INF_M __host__ __device__ __forceinline__
#else
#define INF_M inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_EACH_LANE(l) for (uint32_t l = ln, once_ = 1; once_; once_ = 0)
#define INF_SLOT(l) 0
#define INF_SLOTS 1
#else
#define INF_EACH_LANE(l) for (uint32_t l = 0; l < ::rm::inf::kLanes; ++l)
#define INF_SLOT(l) (l)
#define INF_SLOTS ::rm::inf::kLanes
#endif

namespace rm {
namespace inf {

constexpr uint32_t kRing = 32768, kHalf = 16384, kLanes = 64;

struct alignas(16) Bytes16 {
  uint32_t w[4];
};

struct RingSink {
  uint8_t* ring;          // kRing bytes, 16-byte aligned (LDS on the device)
  uint8_t* out;           // the slot, 16-byte aligned
  uint64_t cap;           // bytes of the slot that may be written
  uint64_t pos = 0;       // bytes produced
  uint64_t kept = 0;      // bytes handed to the slot (a multiple of kHalf until the end)
  uint64_t crc_at = 0;    // bytes in crc
  uint32_t crc = 0xffffffffu;
  uint32_t ln = 0;        // this lane (device)

  INF_M uint32_t lane() const { return ln; }
  INF_M uint32_t lanes() const {
#if defined(__HIP_DEVICE_COMPILE__)
    return kLanes;
#else
    return 1;
#endif
  }
  INF_M void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
  }
  INF_M uint64_t produced() const { return pos; }

  // ring bytes [crc_at, to) into crc, a slice per lane: the range lies inside one half of the ring
  INF_M void crc_to(uint64_t to) {
    const uint32_t n = (uint32_t)(to - crc_at);
    if (n == 0) return;
    const uint32_t slice = (n + kLanes - 1u) / kLanes;
    const uint32_t base = (uint32_t)crc_at & (kRing - 1u);   // base + n <= kRing
    uint32_t part[INF_SLOTS];
    INF_EACH_LANE(l) {
      const uint32_t a = l * slice < n ? l * slice : n, b = a + slice < n ? a + slice : n;
      uint32_t p = 0;
      if (b > a && base + b <= kRing) p = crc_mul(crc_x8n(n - b), crc_bytes(0u, ring + base + a, b - a));
      part[INF_SLOT(l)] = p;
    }
    uint32_t all = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    all = part[0];
    for (int d = 32; d; d >>= 1) all ^= __shfl_xor(all, d, 64);
#else
    for (uint32_t l = 0; l < kLanes; ++l) all ^= part[l];
#endif
    crc = crc_mul(crc_x8n(n), crc) ^ all;
    crc_at = to;
  }
  // ring bytes [kept, to) to the slot, what of them fits: kept is a multiple of kHalf, to - kept <= kHalf
  INF_M void keep_to(uint64_t to) {
    const uint64_t end = to < cap ? to : cap;
    if (kept < end) {
      const uint32_t n = (uint32_t)(end - kept), base = (uint32_t)kept & (kRing - 1u);
      const uint32_t whole = n & ~15u;
      INF_EACH_LANE(l) {
        for (uint32_t k = l * 16u; k < whole; k += kLanes * 16u)
          *(Bytes16*)(out + kept + k) = *(const Bytes16*)(ring + base + k);
        for (uint32_t k = whole + l; k < n; k += kLanes) out[kept + k] = ring[base + k];
      }
    }
    kept = to;
  }
  INF_M void half_done() {   // pos has just reached or passed a half's end
    const uint64_t edge = pos & ~(uint64_t)(kHalf - 1u);
    sync();
    crc_to(edge);
    keep_to(edge);
  }
  INF_M void lit(uint8_t c) {
    INF_EACH_LANE(l) {
      if (l == 0) ring[(uint32_t)pos & (kRing - 1u)] = c;
    }
    ++pos;
    if (((uint32_t)pos & (kHalf - 1u)) == 0) half_done();
  }
  // lane i takes byte i (and i + 64, ...); for dist < len the source index wraps modulo dist, so
  // every source byte was there before the copy began
  INF_M void copy(uint32_t dist, uint32_t len) {   // 1 <= dist <= 32768, dist <= pos, len <= 258
    sync();
    const uint32_t from = (uint32_t)(pos - dist), to = (uint32_t)pos;
    for (uint32_t k0 = 0; k0 < len; k0 += kLanes) {
      uint8_t c[INF_SLOTS];
      INF_EACH_LANE(l) {
        const uint32_t k = k0 + l;
        c[INF_SLOT(l)] = k < len ? ring[(from + k % dist) & (kRing - 1u)] : (uint8_t)0;
      }
      INF_EACH_LANE(l) {
        const uint32_t k = k0 + l;
        if (k < len) ring[(to + k) & (kRing - 1u)] = c[INF_SLOT(l)];
      }
    }
    const uint64_t before = pos;
    pos += len;
    if ((before ^ pos) & ~(uint64_t)(kHalf - 1u)) half_done();
  }
  INF_M void raw(const uint8_t* src, uint32_t len) {
    while (len) {
      const uint32_t room = kHalf - ((uint32_t)pos & (kHalf - 1u)), m = len < room ? len : room;
      const uint32_t to = (uint32_t)pos & (kRing - 1u);   // to + m <= kRing
      INF_EACH_LANE(l) {
        for (uint32_t k = l; k < m; k += kLanes) ring[(to + k) & (kRing - 1u)] = src[k];
      }
      pos += m;
      src += m;
      len -= m;
      if (m == room) half_done();
    }
  }
  INF_M void member_begin() {
    crc = 0xffffffffu;
    crc_at = pos;
  }
  INF_M uint32_t member_crc() {
    sync();
    crc_to(pos);
    return ~crc;
  }
  INF_M void finish() {
    sync();
    keep_to(pos);
  }
  INF_M uint32_t last_byte() const { return pos ? ring[(uint32_t)(pos - 1u) & (kRing - 1u)] : 0u; }
};

// one chunk through the ring as a wave would run it
template <class Sink>
INF_HD uint32_t inflate_ring_chunk(const uint8_t* p, uint64_t n, Work& w, Sink& s, uint32_t& members) {
  const uint32_t ln = s.lane();
  (void)ln;
  INF_EACH_LANE(l) {
    for (uint32_t i = l; i < kMaxLens; i += kLanes) w.lens[i] = 0;
    if (l == 0) w.lit.maxlen = w.dist.maxlen = 0;
  }
  s.sync();
  const uint32_t status = read_chunk(p, n, w, s, members);
  s.finish();
  return status;
}

}  // namespace inf
}  // namespace rm
