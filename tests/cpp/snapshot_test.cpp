// The stream snapshot's layout, checksum and structural rule on the host (snapshot.hpp, the code
// rm_snapshot_check_host runs and whose element rules the kernels of snapshot.hip share): a blob
// from the host writer is accepted; every truncation, every single flipped bit of header and table
// and one forged blob per clause of the rule (checksums recomputed) are rejected, each with its
// message; the checksum changes under every single flipped bit of a 4 KiB section.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "snapshot.hpp"

using namespace rm;
using namespace rm::snap;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

struct State {
  std::string user = "hello";
  std::vector<uint64_t> off = {0, 3, 7, 12};
  std::string names = "abcdefghijkl";
  std::vector<SessRec> rec = {{1, 2, 3.5f, 0, 1000}, {4, 3, 0.0f, 0, 2000}};
  std::vector<float> lon = {1, 2, 3, 4, 5}, lat = {6, 7, 8, 9, 10}, acc = {-1, -1, 5, 5, 5};
  std::vector<double> time = {10, 11, 12, 13, 14};
  std::vector<uint8_t> rows = std::vector<uint8_t>(2 * kRowBytes, 7);
  TileMeta meta = {9, 60, 0};
};

static std::vector<uint8_t> write(const State& s) {
  Writer w;
  w.add(kUser, s.user.data(), s.user.size());
  w.add(kDirOff, s.off.data(), s.off.size());
  w.add(kDirBytes, s.names.data(), s.names.size());
  w.add(kSessRec, s.rec.data(), s.rec.size());
  w.add(kSessLon, s.lon.data(), s.lon.size());
  w.add(kSessLat, s.lat.data(), s.lat.size());
  w.add(kSessAcc, s.acc.data(), s.acc.size());
  w.add(kSessTime, s.time.data(), s.time.size());
  w.add(kTileRows, s.rows.data(), s.rows.size() / kRowBytes);
  w.add(kTileMeta, &s.meta, 1);
  return w.finish();
}

static std::string check(const std::vector<uint8_t>& b, uint32_t n_vehicles = 0) {
  // an exact-size copy on the heap: a read past the end is a sanitizer error
  std::vector<uint8_t> c(b.begin(), b.end());
  c.shrink_to_fit();
  uint64_t info[9];
  return check_host(c.data(), c.size(), info, n_vehicles);
}

// header or table rewritten, the table's checksum recomputed
static std::vector<uint8_t> retable(std::vector<uint8_t> b, const std::function<void(Header&, std::vector<Entry>&)>& f) {
  Header h;
  std::memcpy(&h, b.data(), sizeof h);
  std::vector<Entry> e(h.n_sections);
  std::memcpy(e.data(), b.data() + sizeof h, e.size() * sizeof(Entry));
  f(h, e);
  h.table_sum = table_checksum(h, e.data());
  std::memcpy(b.data(), &h, sizeof h);
  std::memcpy(b.data() + sizeof h, e.data(), e.size() * sizeof(Entry));
  return b;
}

static void expect(const char* what, const std::string& got, const std::string& want) {
  if (got != want) { std::printf("FAIL %s: got \"%s\", want \"%s\"\n", what, got.c_str(), want.c_str()); ++g_fail; }
}

int main() {
  const State ok;
  const std::vector<uint8_t> good = write(ok);
  {
    uint64_t info[9];
    CHECK(check_host(good.data(), good.size(), info).empty());
    CHECK(info[0] == kVersion && info[1] == good.size() && info[2] == 3 && info[3] == 2 && info[4] == 5 && info[5] == 2);
    CHECK(info[6] == 60 && info[8] == 5 && std::memcmp(good.data() + info[7], "hello", 5) == 0);
    CHECK(good.size() % 16 == 0);
    Writer none;
    CHECK(check(none.finish()).empty());
  }
  // every truncation
  for (size_t n = 0; n < good.size(); ++n) {
    const std::vector<uint8_t> cut(good.begin(), good.begin() + n);
    if (check(cut).empty()) { std::printf("FAIL truncation to %zu accepted\n", n); ++g_fail; }
  }
  // every single flipped bit of header and table (and of the padding behind the table)
  {
    Header h;
    std::memcpy(&h, good.data(), sizeof h);
    const uint64_t d0 = data_start(h.n_sections);
    for (uint64_t bit = 0; bit < d0 * 8; ++bit) {
      std::vector<uint8_t> b = good;
      b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      if (check(b).empty()) { std::printf("FAIL flipped bit %llu accepted\n", (unsigned long long)bit); ++g_fail; }
    }
    // ... and a flipped bit anywhere behind them
    for (uint64_t bit = d0 * 8; bit < good.size() * 8; ++bit) {
      std::vector<uint8_t> b = good;
      b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      if (check(b).empty()) { std::printf("FAIL flipped data bit %llu accepted\n", (unsigned long long)bit); ++g_fail; }
    }
  }
  // forged blobs, checksums recomputed: one per clause
  auto entry = [](std::vector<Entry>& e, uint32_t kind) -> Entry& {
    for (Entry& x : e)
      if (x.kind == kind) return x;
    std::abort();
  };
  expect("version", check(retable(good, [](Header& h, std::vector<Entry>&) { h.version = 2; })), "snapshot: unknown format version");
  expect("kind", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kUser).kind = 77; })), "snapshot: unknown section kind");
  expect("twice", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kSessLat).kind = kSessLon; })),
         "snapshot: a section kind appears twice");
  expect("misaligned", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kDirBytes).off += 8; })),
         "snapshot: a section is misaligned");
  expect("past the end", check(retable(good, [&](Header& h, std::vector<Entry>& e) { entry(e, kTileMeta).off = h.bytes; })),
         "snapshot: a section runs past the end");
  expect("overlap", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kDirBytes).off = entry(e, kDirOff).off; })),
         "snapshot: sections overlap");
  expect("count x size", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kSessRec).count += 1; })),
         "snapshot: a section's count times size is not its bytes");
  expect("element size", check(retable(good, [&](Header&, std::vector<Entry>& e) { entry(e, kSessLon).elem = 2; })),
         "snapshot: a section's count times size is not its bytes");
  {
    State s = ok;
    s.rec[1].vehicle = 1;
    expect("vehicle order", check(write(s)), message(kEVehOrder));
    s = ok; s.rec[0].vehicle = 9;
    expect("vehicle order", check(write(s)), message(kEVehOrder));
    s = ok; s.rec[0].cnt = 0; s.rec[1].cnt = 5;
    expect("cnt 0", check(write(s)), message(kECntZero));
    s = ok; s.rec[1].cnt = 4;
    expect("cnt sum", check(write(s)), message(kECntSum));
    s = ok; s.rec[0].max_sep = -1.0f;
    expect("max_sep < 0", check(write(s)), message(kEMaxSep));
    s = ok; s.rec[0].max_sep = std::numeric_limits<float>::infinity();
    expect("max_sep inf", check(write(s)), message(kEMaxSep));
    s = ok; s.rec[0].max_sep = std::nanf("");
    expect("max_sep NaN", check(write(s)), message(kEMaxSep));
    s = ok; s.time[3] = std::nan("");
    expect("NaN time", check(write(s)), message(kETimeNaN));
    s = ok; s.off[1] = 8;
    expect("offsets not monotone", check(write(s)), message(kEOffMono));
    s = ok; s.off[3] = 20;
    expect("offset past the bytes", check(write(s)), message(kEOffRange));
    s = ok; s.off[0] = 1;
    expect("first offset", check(write(s)), message(kEOffRange));
    s = ok; s.off[3] = 11;
    expect("bytes behind the names", check(write(s)), message(kEOffRange));
    s = ok; s.off[1] = 0;
    expect("empty name", check(write(s)), message(kENameLen));
    s = ok; s.names.assign(4097 + 9, 'x'); s.names.replace(0, 9, "abcdefghi"); s.off = {0, 3, 9, 9 + 4097};
    expect("long name", check(write(s)), message(kENameLen));
    s = ok; s.names = "abcdefgabcxx"; s.off = {0, 3, 7, 10}; s.names.resize(10);
    expect("equal names", check(write(s)), message(kEDupName));
    // what the loading objects decide
    expect("n_vehicles", check(good, 4), message(kEVehRange));
    expect("n_vehicles", check(good, 5), "");
    Table t;
    CHECK(parse_table(good.data(), good.size(), t).empty());
    expect("max_vehicles", check_targets(good.data(), t, 0, 2, 0), "snapshot: more names than the directory's max_vehicles");
    expect("max_vehicles", check_targets(good.data(), t, 0, 3, 60), "");
    expect("quantisation", check_targets(good.data(), t, 0, 0, 120), "snapshot: its quantisation is not the tile store's");
    // a group of sections comes whole
    Writer w;
    w.add(kSessRec, ok.rec.data(), ok.rec.size());
    expect("incomplete", check(w.finish()), "snapshot: the session sections are incomplete");
  }
  // the checksum under every single flipped bit of a 4 KiB section (and of a ragged one)
  for (size_t bytes : {(size_t)4096, (size_t)4093}) {
    std::vector<uint8_t> sec(bytes);
    uint64_t x = 88172645463325252ull;
    for (uint8_t& c : sec) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c = (uint8_t)x; }
    const uint64_t base = checksum(sec.data(), sec.size());
    size_t same = 0;
    for (size_t bit = 0; bit < sec.size() * 8; ++bit) {
      sec[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      same += checksum(sec.data(), sec.size()) == base ? 1 : 0;
      sec[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    }
    CHECK(same == 0);
    CHECK(checksum(sec.data(), sec.size()) == base);
  }
  CHECK(checksum(nullptr, 0) == 0);
  if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
  std::printf("snapshot ok\n");
  return 0;
}
