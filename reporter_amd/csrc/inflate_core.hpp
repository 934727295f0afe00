// inflate_core.hpp — rule 20: a chunk of gzip members (RFC 1952) holding DEFLATE
// streams (RFC 1951), read the way Python's gzip module reads it.  One __host__ __device__ core,
// free of HIP types, shared by the host decoder (inflate_host_chunk below, and the program
// tests/cpp/inflate_core_test.cpp) and by k_inflate (inflate.hip): the bit reader, the member
// header and trailer, the code-length sets, the table construction, one symbol step, and the
// CRC-32 with its combine.  What differs between the two sides is the sink the symbols go to.
//
// A sink has:  lane() / lanes()   which of how many cooperating lanes runs this copy of the code
//              sync()             writes to the work area by one lane become visible to all
//              lit(b)  copy(dist, len)  raw(src, len)     the output
//              produced()         bytes of the chunk so far
//              member_begin()  member_crc()               the CRC-32 of the bytes since member_begin
// Every lane runs the whole decoder on the same values; only the sink and the table fill divide
// work by lane.  That includes plain (non-atomic) writes and read-modify-writes of the work area
// (w.lens[i] = c, h.count[l]++) by all 64 lanes at once.  It is correct because the lanes of a
// gfx9 wave64 execute one instruction stream in lockstep and every branch here is taken alike by
// all of them: the 64 loads of h.count[l] all complete before the 64 stores of the same value + 1,
// so the word advances by one, not by 64, and each lane later reads back what it wrote itself.
// The code must not be run by lanes that can diverge (several waves on one work area, or a
// target with independent thread scheduling): tables would then need one writer between syncs.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD static inline
#endif

#include <vector>

namespace rm {
namespace inf {

enum : uint32_t { kOk = 0, kHeader = 1, kTruncated = 2, kBlock = 3, kCrc = 4, kSize = 5, kTooLarge = 6, kStatusCount = 7 };

constexpr uint32_t kFastBits = 9;
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kMaxLens = 320;   // 286 + 30 rounded up; fixed sets use 288 + 32
constexpr uint64_t kMaxOut = 0xffffffffull;                         // a chunk's inflated bytes stay under 2^32

INF_HD const char* status_text(uint32_t s) {
  switch (s) {
    case kOk: return "ok";
    case kHeader: return "not a gzip member (bad magic or method)";
    case kTruncated: return "the data ends before the end of the member";
    case kBlock: return "malformed deflate block";
    case kCrc: return "CRC check failed";
    case kSize: return "incorrect length of data produced";
    case kTooLarge: return "inflated data too large";
  }
  return "unknown status";
}

// ---- the bit reader: LSB first, a 64-bit buffer; every read is limited by n
struct Bits {
  const uint8_t* p;
  uint64_t n, at;
  uint64_t buf;
  uint32_t cnt;
};

INF_HD void bits_init(Bits& b, const uint8_t* p, uint64_t n, uint64_t at) {
  b.p = p; b.n = n; b.at = at; b.buf = 0; b.cnt = 0;
}

// bits above cnt are either zero or the bits that follow in the input
INF_HD void refill(Bits& b) {
  if (b.at + 8 <= b.n && b.cnt < 64) {
    uint64_t w;
    __builtin_memcpy(&w, b.p + b.at, 8);
    b.buf |= w << b.cnt;
    b.at += (63 - b.cnt) >> 3;
    b.cnt |= 56;
  } else {
    while (b.cnt <= 56 && b.at < b.n) {
      b.buf |= (uint64_t)b.p[b.at++] << b.cnt;
      b.cnt += 8;
    }
  }
}

INF_HD void drop(Bits& b, uint32_t k) {   // k <= cnt
  b.buf = k >= 64 ? 0 : b.buf >> k;
  b.cnt -= k;
}

// k <= 32 bits, or false: the input ended
INF_HD bool take(Bits& b, uint32_t k, uint32_t& v) {
  if (b.cnt < k) {
    refill(b);
    if (b.cnt < k) return false;
  }
  v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
  drop(b, k);
  return true;
}

// to the next byte boundary, the buffered whole bytes handed back: at is the next unread byte
INF_HD void to_bytes(Bits& b) {
  b.at -= b.cnt >> 3;
  b.buf = 0;
  b.cnt = 0;
}

// ---- canonical codes: counts per length and the symbols in code order, plus a first-level lookup
struct Huff {
  uint16_t count[16];
  uint16_t sym[kMaxLit];
  uint16_t fast[1u << kFastBits];   // (symbol << 4) | length, 0: longer than kFastBits or invalid
  uint32_t maxlen;
};

// counts and symbol order of n lengths; returns what is left of the code space: < 0 over-subscribed,
// > 0 incomplete
INF_HD int huff_counts(Huff& h, const uint8_t* lens, uint32_t n) {
  uint16_t offs[16];
  for (uint32_t l = 0; l < 16; ++l) h.count[l] = 0;
  for (uint32_t i = 0; i < n; ++i) h.count[lens[i] & 15]++;
  h.maxlen = 0;
  for (uint32_t l = 1; l < 16; ++l)
    if (h.count[l]) h.maxlen = l;
  int left = 1;
  for (uint32_t l = 1; l < 16; ++l) {
    left <<= 1;
    left -= (int)h.count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t l = lens[i] & 15;
    if (l) {
      const uint32_t at = offs[l]++;
      if (at < kMaxLit) h.sym[at] = (uint16_t)i;
    }
  }
  return left;
}

// the symbol of the code at the low end of bits, of which avail are real: >= 0 the symbol (len set),
// -1 no such code, -2 more input needed
INF_HD int huff_walk(const Huff& h, uint64_t bits, uint32_t avail, uint32_t& len) {
  int code = 0, first = 0, index = 0;
  if (h.maxlen == 0) return avail ? -1 : -2;
  for (uint32_t l = 1; l <= h.maxlen; ++l) {
    if (l > avail) return -2;
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int count = h.count[l];
    if (code - count < first) {
      const int at = index + (code - first);
      if (at < 0 || at >= (int)kMaxLit) return -1;
      len = l;
      return h.sym[at];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// the first-level lookup, entries divided among the lanes
INF_HD void huff_fast(Huff& h, uint32_t lane, uint32_t lanes) {
  for (uint32_t i = lane; i < (1u << kFastBits); i += lanes) {
    uint32_t len = 0;
    const int s = huff_walk(h, i, kFastBits, len);
    h.fast[i] = s >= 0 ? (uint16_t)(((uint32_t)s << 4) | len) : (uint16_t)0;
  }
}

// one code read: >= 0 the symbol, -1 invalid code, -2 the input ended
template <bool kFast>
INF_HD int huff_read(Bits& b, const Huff& h) {
  if (b.cnt < 15) refill(b);
  if (kFast) {
    const uint32_t e = h.fast[b.buf & ((1u << kFastBits) - 1u)];
    if (e) {
      const uint32_t len = e & 15u;
      if (len > b.cnt) return -2;
      drop(b, len);
      return (int)(e >> 4);
    }
  }
  uint32_t len = 0;
  const int s = huff_walk(h, b.buf, b.cnt < 15 ? b.cnt : 15u, len);
  if (s >= 0) drop(b, len);
  return s;
}

// what a chunk's decoder works in: 3.6 KiB (in LDS on the device)
struct Work {
  Huff lit, dist;
  uint8_t lens[kMaxLens];
};

// ---- CRC-32 (reflected 0xedb88320), a nibble at a time, and its algebra
INF_HD uint32_t crc_bytes(uint32_t state, const uint8_t* p, uint64_t n) {
  const uint32_t t[16] = {0x00000000u, 0x1db71064u, 0x3b6e20c8u, 0x26d930acu, 0x76dc4190u, 0x6b6b51f4u, 0x4db26158u, 0x5005713cu,
                          0xedb88320u, 0xf00f9344u, 0xd6d6a3e8u, 0xcb61b38cu, 0x9b64c2b0u, 0x86d3d2d4u, 0xa00ae278u, 0xbdbdf21cu};
  for (uint64_t i = 0; i < n; ++i) {
    state ^= p[i];
    state = (state >> 4) ^ t[state & 15u];
    state = (state >> 4) ^ t[state & 15u];
  }
  return state;
}

// a * b mod P, polynomials bit-reflected (x^0 is bit 31)
INF_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}

// x^(8n) mod P
INF_HD uint32_t crc_x8n(uint64_t n) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;
  for (; n; n >>= 1) {
    if (n & 1u) r = crc_mul(r, sq);
    sq = crc_mul(sq, sq);
  }
  return r;
}

// the register after n more bytes whose own register (from 0) is `pure`
INF_HD uint32_t crc_append(uint32_t state, uint32_t pure, uint64_t n) { return crc_mul(crc_x8n(n), state) ^ pure; }

// ---- the member header at `at`: kOk (at past it), kHeader or kTruncated
INF_HD uint32_t read_header(const uint8_t* p, uint64_t n, uint64_t& at) {
  const uint64_t have = n - at;
  if (have < 2 || p[at] != 0x1f || p[at + 1] != 0x8b) return kHeader;
  if (have < 10) return kTruncated;
  if (p[at + 2] != 8) return kHeader;
  const uint32_t flg = p[at + 3];
  at += 10;
  if (flg & 4u) {   // FEXTRA
    if (n - at < 2) return kTruncated;
    const uint64_t x = (uint64_t)p[at] | ((uint64_t)p[at + 1] << 8);
    at += 2;
    if (n - at < x) return kTruncated;
    at += x;
  }
  for (uint32_t f = 8u; f <= 16u; f <<= 1) {   // FNAME, FCOMMENT
    if (!(flg & f)) continue;
    for (;;) {
      if (at >= n) return kTruncated;
      if (p[at++] == 0) break;
    }
  }
  if (flg & 2u) {   // FHCRC: skipped, not checked
    if (n - at < 2) return kTruncated;
    at += 2;
  }
  return kOk;
}

INF_HD void length_of(uint32_t s, uint32_t& base, uint32_t& extra) {   // s in 257 .. 285
  if (s < 265u) { base = s - 254u; extra = 0; return; }
  if (s == 285u) { base = 258u; extra = 0; return; }
  extra = (s - 261u) >> 2;
  base = 3u + ((4u + ((s - 265u) & 3u)) << extra);
}
INF_HD void distance_of(uint32_t d, uint32_t& base, uint32_t& extra) {   // d in 0 .. 29
  if (d < 4u) { base = d + 1u; extra = 0; return; }
  extra = (d >> 1) - 1u;
  base = 1u + ((2u + (d & 1u)) << extra);
}

// a dynamic block's two sets from its header: kOk, kTruncated or kBlock (zlib's inflate_table rules)
template <class Sink>
INF_HD uint32_t read_sets(Bits& b, Work& w, Sink& s) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t v;
  if (!take(b, 14, v)) return kTruncated;
  const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = ((v >> 10) & 15u) + 4u;
  if (nlen > 286u || ndist > 30u) return kBlock;
  const uint32_t total = nlen + ndist;
  for (uint32_t i = 0; i < 19; ++i) w.lens[i] = 0;
  for (uint32_t i = 0; i < ncode; ++i) {
    if (!take(b, 3, v)) return kTruncated;
    w.lens[order[i]] = (uint8_t)v;
  }
  Huff& cl = w.dist;   // (the distance set is built after the lengths are read)
  const int cl_left = huff_counts(cl, w.lens, 19);
  if (cl.maxlen == 0) {   // zlib accepts the empty set and reads a bit per length out of it, all zero: no symbol 256
    for (uint32_t i = 0; i < total; ++i)
      if (!take(b, 1, v)) return kTruncated;
    return kBlock;
  }
  if (cl_left != 0) return kBlock;
  s.sync();
  for (uint32_t i = 0; i < total;) {
    const int c = huff_read<false>(b, cl);
    if (c < 0) return c == -2 ? kTruncated : kBlock;
    if (c < 16) { w.lens[i++] = (uint8_t)c; continue; }
    uint32_t prev = 0, rep;
    if (c == 16) {
      if (!take(b, 2, v)) return kTruncated;
      if (i == 0) return kBlock;
      prev = w.lens[i - 1];
      rep = 3u + v;
    } else if (c == 17) {
      if (!take(b, 3, v)) return kTruncated;
      rep = 3u + v;
    } else {
      if (!take(b, 7, v)) return kTruncated;
      rep = 11u + v;
    }
    if (i + rep > total) return kBlock;
    while (rep--) w.lens[i++] = (uint8_t)prev;
  }
  if (w.lens[256] == 0) return kBlock;
  s.sync();
  int left = huff_counts(w.lit, w.lens, nlen);
  if (left < 0 || (left > 0 && w.lit.maxlen != 1)) return kBlock;
  left = huff_counts(w.dist, w.lens + nlen, ndist);
  if (left < 0 || (left > 0 && w.dist.maxlen > 1)) return kBlock;
  return kOk;
}

template <class Sink>
INF_HD void fixed_sets(Work& w, Sink& s) {
  for (uint32_t i = 0; i < 288; ++i) w.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (uint32_t i = 0; i < 32; ++i) w.lens[288 + i] = 5;
  s.sync();
  huff_counts(w.lit, w.lens, 288);
  huff_counts(w.dist, w.lens + 288, 32);
}

// the symbols of one block up to its end-of-block; mstart: produced() at the member's start
template <class Sink>
INF_HD uint32_t read_symbols(Bits& b, const Work& w, Sink& s, uint64_t mstart) {
  for (;;) {
    const int c = huff_read<true>(b, w.lit);
    if (c < 0) return c == -2 ? kTruncated : kBlock;
    if (c < 256) { s.lit((uint8_t)c); continue; }
    if (c == 256) return kOk;
    if (c >= 286) return kBlock;
    uint32_t base, extra, v = 0;
    length_of((uint32_t)c, base, extra);
    if (extra && !take(b, extra, v)) return kTruncated;
    const uint32_t len = base + v;
    const int dc = huff_read<true>(b, w.dist);
    if (dc < 0) return dc == -2 ? kTruncated : kBlock;
    if (dc >= 30) return kBlock;
    distance_of((uint32_t)dc, base, extra);
    v = 0;
    if (extra && !take(b, extra, v)) return kTruncated;
    const uint32_t dist = base + v;
    const uint64_t at = s.produced();
    if (dist > at - mstart) return kBlock;
    if (at + len > kMaxOut) return kTooLarge;
    s.copy(dist, len);
  }
}

// one member's DEFLATE stream from byte `at`, then its trailer; at ends past the trailer
template <class Sink>
INF_HD uint32_t read_member(const uint8_t* p, uint64_t n, uint64_t& at, Work& w, Sink& s) {
  Bits b;
  bits_init(b, p, n, at);
  const uint64_t mstart = s.produced();
  s.member_begin();
  for (;;) {
    uint32_t v;
    if (!take(b, 3, v)) return kTruncated;
    const uint32_t last = v & 1u, type = v >> 1;
    if (type == 0) {
      drop(b, b.cnt & 7u);
      to_bytes(b);
      if (b.n - b.at < 4) return kTruncated;
      const uint32_t len = (uint32_t)b.p[b.at] | ((uint32_t)b.p[b.at + 1] << 8);
      const uint32_t nlen = (uint32_t)b.p[b.at + 2] | ((uint32_t)b.p[b.at + 3] << 8);
      if (len != (nlen ^ 0xffffu)) return kBlock;
      b.at += 4;
      if (b.n - b.at < len) return kTruncated;
      if (s.produced() + len > kMaxOut) return kTooLarge;
      s.raw(b.p + b.at, len);
      b.at += len;
    } else if (type == 3) {
      return kBlock;
    } else {
      if (type == 1) {
        fixed_sets(w, s);
      } else {
        const uint32_t st = read_sets(b, w, s);
        if (st != kOk) return st;
      }
      s.sync();
      huff_fast(w.lit, s.lane(), s.lanes());
      huff_fast(w.dist, s.lane(), s.lanes());
      s.sync();
      const uint32_t st = read_symbols(b, w, s, mstart);
      if (st != kOk) return st;
    }
    if (last) break;
  }
  drop(b, b.cnt & 7u);
  to_bytes(b);
  at = b.at;
  if (n - at < 8) return kTruncated;
  const uint32_t crc = (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8) | ((uint32_t)p[at + 2] << 16) | ((uint32_t)p[at + 3] << 24);
  const uint32_t isz = (uint32_t)p[at + 4] | ((uint32_t)p[at + 5] << 8) | ((uint32_t)p[at + 6] << 16) | ((uint32_t)p[at + 7] << 24);
  at += 8;
  if (s.member_crc() != crc) return kCrc;
  if ((uint32_t)(s.produced() - mstart) != isz) return kSize;
  return kOk;
}

// a whole chunk: members until the input ends; zero bytes after a trailer are skipped
template <class Sink>
INF_HD uint32_t read_chunk(const uint8_t* p, uint64_t n, Work& w, Sink& s, uint32_t& members) {
  uint64_t at = 0;
  members = 0;
  while (at < n) {
    uint32_t st = read_header(p, n, at);
    if (st != kOk) return st;
    st = read_member(p, n, at, w, s);
    if (st != kOk) return st;
    ++members;
    while (at < n && p[at] == 0) ++at;
  }
  return kOk;
}

// the inflated size the last member's trailer promises (0 where the chunk is too short to have
// one): exact for a valid one-member chunk, a lower bound for a valid chunk of several
// (zero padding after the trailer makes it read low; DEFLATE cannot grow n bytes past 1032 n)
INF_HD uint64_t isize_hint(const uint8_t* p, uint64_t n) {
  if (n < 18) return 0;
  const uint64_t v = (uint64_t)p[n - 4] | ((uint64_t)p[n - 3] << 8) | ((uint64_t)p[n - 2] << 16) | ((uint64_t)p[n - 1] << 24);
  const uint64_t most = n * 1032ull;
  return v < most ? v : most;
}

// ---- the host decoder: the core run sequentially into a vector
struct HostSink {
  std::vector<uint8_t>& out;
  uint64_t mstart = 0;
  explicit HostSink(std::vector<uint8_t>& o) : out(o) {}
  uint32_t lane() const { return 0; }
  uint32_t lanes() const { return 1; }
  void sync() {}
  void lit(uint8_t c) { out.push_back(c); }
  void copy(uint32_t dist, uint32_t len) {
    const size_t at = out.size();
    out.resize(at + len);
    uint8_t* d = out.data() + at;
    const uint8_t* s = d - dist;
    for (uint32_t k = 0; k < len; ++k) d[k] = s[k];
  }
  void raw(const uint8_t* src, uint32_t len) { out.insert(out.end(), src, src + len); }
  uint64_t produced() const { return out.size(); }
  void member_begin() { mstart = out.size(); }
  uint32_t member_crc() const { return ~crc_bytes(0xffffffffu, out.data() + mstart, out.size() - mstart); }
};

// out: the chunk's bytes up to the first error
inline uint32_t inflate_host_chunk(const uint8_t* p, uint64_t n, std::vector<uint8_t>& out, uint32_t& members) {
  Work w;
  for (uint32_t i = 0; i < kMaxLens; ++i) w.lens[i] = 0;
  w.lit.maxlen = w.dist.maxlen = 0;
  HostSink s(out);
  return read_chunk(p, n, w, s, members);
}

}  // namespace inf
}  // namespace rm
