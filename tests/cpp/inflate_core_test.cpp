// The host decoder of reporter_amd/csrc/inflate_core.hpp (the code k_inflate runs per wave) over a
// catalogue file and over byte- and bit-mutated copies of its streams: every run must end with a
// status, the named streams with the status and bytes the file expects.  Built with
// AddressSanitizer and UBSan and run directly (tests/test_inflate_core_cpp.py writes the file).
//
// File: u32 count, then per stream u32 length, the bytes, u32 expected status, u32 expected output
// length, u32 expected CRC-32 of the output (both 0 for a bad stream).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate_core.hpp"
#include "inflate_ring.hpp"

namespace {

struct Stream {
  std::vector<uint8_t> z;
  uint32_t status, out_len, crc;
};

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

bool read_u32(FILE* f, uint32_t& v) { return std::fread(&v, 4, 1, f) == 1; }

// the chunk through the window ring, as a wave runs it, into a slot of exactly cap bytes rounded up
// to 16 (what inflate.hip allocates): false when it disagrees with the host decoder's result
struct alignas(16) Ring {
  uint8_t b[rm::inf::kRing];
};
bool ring_agrees(const std::vector<uint8_t>& z, uint64_t cap, uint32_t status, const std::vector<uint8_t>& bytes, uint32_t members) {
  static Ring ring;
  static rm::inf::Work work;
  const size_t room = (size_t)((cap + 15u) & ~(uint64_t)15u);
  uint8_t* slot = (uint8_t*)std::aligned_alloc(16, room ? room : 16);
  rm::inf::RingSink s;
  s.ring = ring.b;
  s.out = slot;
  s.cap = cap;
  uint32_t m = 0;
  const uint32_t st = rm::inf::inflate_ring_chunk(z.data(), z.size(), work, s, m);
  const size_t stored = (size_t)(s.pos < cap ? s.pos : cap);
  const bool same = st == status && m == members && s.pos == bytes.size() && std::memcmp(slot, bytes.data(), stored) == 0 &&
                    s.last_byte() == (bytes.empty() ? 0u : bytes.back());
  std::free(slot);
  return same;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: inflate_core_test <catalogue> <mutations>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror("catalogue"); return 2; }
  const long want = std::strtol(argv[2], nullptr, 10);
  uint32_t n = 0;
  if (!read_u32(f, n)) return 2;
  std::vector<Stream> cat(n);
  for (Stream& s : cat) {
    uint32_t len = 0;
    if (!read_u32(f, len)) return 2;
    s.z.resize(len);
    if (len && std::fread(s.z.data(), 1, len, f) != len) return 2;
    if (!read_u32(f, s.status) || !read_u32(f, s.out_len) || !read_u32(f, s.crc)) return 2;
  }
  std::fclose(f);
  // ---- the named streams
  std::vector<uint8_t> out;
  for (size_t i = 0; i < cat.size(); ++i) {
    const Stream& s = cat[i];
    uint32_t members = 0;
    out.clear();
    // (a copy of exactly the stream's size: a read past its end is the sanitizer's to see)
    std::vector<uint8_t> z(s.z);
    const uint32_t st = rm::inf::inflate_host_chunk(z.data(), z.size(), out, members);
    if (st != s.status) { std::printf("stream %zu: status %u, expected %u\n", i, st, s.status); return 1; }
    if (st == 0) {
      const uint32_t crc = ~rm::inf::crc_bytes(0xffffffffu, out.data(), out.size());
      if (out.size() != s.out_len || crc != s.crc) { std::printf("stream %zu: wrong bytes\n", i); return 1; }
    }
    // the ring: an exact slot, the slot the trailer promises, a slot a byte short, and counting alone
    const uint64_t caps[4] = {out.size(), rm::inf::isize_hint(z.data(), z.size()), out.empty() ? 0 : out.size() - 1, 0};
    for (uint64_t cap : caps)
      if (!ring_agrees(z, cap, st, out, members)) { std::printf("stream %zu: the ring disagrees at a slot of %llu\n", i, (unsigned long long)cap); return 1; }
  }
  // ---- the CRC algebra: a split stream's parts combine to the whole
  for (int k = 0; k < 200; ++k) {
    std::vector<uint8_t> a(rnd() % 5000), b(rnd() % 5000);
    for (uint8_t& c : a) c = (uint8_t)rnd();
    for (uint8_t& c : b) c = (uint8_t)rnd();
    std::vector<uint8_t> ab(a);
    ab.insert(ab.end(), b.begin(), b.end());
    const uint32_t whole = rm::inf::crc_bytes(0xffffffffu, ab.data(), ab.size());
    const uint32_t left = rm::inf::crc_bytes(0xffffffffu, a.data(), a.size());
    const uint32_t joined = rm::inf::crc_append(left, rm::inf::crc_bytes(0u, b.data(), b.size()), b.size());
    if (whole != joined) { std::printf("crc combine %d\n", k); return 1; }
  }
  // ---- mutated copies: the small streams in turn (a large one costs its whole length per run)
  std::vector<size_t> small;
  for (size_t i = 0; i < cat.size(); ++i)
    if (!cat[i].z.empty() && cat[i].z.size() <= 6000) small.push_back(i);
  if (small.empty()) { std::printf("no small streams\n"); return 1; }
  long runs = 0;
  uint64_t by_status[rm::inf::kStatusCount] = {0, 0, 0, 0, 0, 0, 0};
  for (; runs < want; ++runs) {
    std::vector<uint8_t> z(cat[small[(size_t)runs % small.size()]].z);
    const uint32_t kind = rnd() % 6u;
    const uint32_t hits = 1u + rnd() % 3u;
    for (uint32_t h = 0; h < hits && !z.empty(); ++h) {
      const size_t at = rnd() % z.size();
      switch (kind) {
        case 0: z[at] ^= (uint8_t)(1u << (rnd() % 8u)); break;   // a bit
        case 1: z[at] = (uint8_t)rnd(); break;                   // a byte
        case 2: z.resize(at); break;                             // cut
        case 3: z.insert(z.begin() + (long)at, (uint8_t)rnd()); break;
        case 4: z.erase(z.begin() + (long)at); break;
        default: z[at] = rnd() & 1u ? 0x00 : 0xff; break;
      }
    }
    std::vector<uint8_t> exact(z);   // (capacity == size)
    exact.shrink_to_fit();
    uint32_t members = 0;
    out.clear();
    const uint32_t st = rm::inf::inflate_host_chunk(exact.data(), exact.size(), out, members);
    if (st >= rm::inf::kStatusCount) { std::printf("run %ld: status %u\n", runs, st); return 1; }
    if (out.size() > exact.size() * 1032ull + 1032ull) { std::printf("run %ld: %zu bytes from %zu\n", runs, out.size(), exact.size()); return 1; }
    if (!ring_agrees(exact, rm::inf::isize_hint(exact.data(), exact.size()), st, out, members)) { std::printf("run %ld: the ring disagrees\n", runs); return 1; }
    ++by_status[st];
  }
  std::printf("inflate core ok: %zu streams, %ld mutated runs, statuses", cat.size(), runs);
  for (uint64_t c : by_status) std::printf(" %llu", (unsigned long long)c);
  std::printf("\n");
  return 0;
}
