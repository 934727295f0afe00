// The two sections a sharded stream's snapshot adds (DESIGN.md §3 rule 17; snapshot.hpp kinds 11 and
// 12) on the host: a blob with them from the host writer is accepted and reports rank, nranks and
// calls; each new clause, broken one at a time with the checksums recomputed, is refused with its
// own message; a flipped bit in either section is a checksum error; the ten-kind blob still passes.
#include <cstdio>
#include <cstdlib>
#include <functional>
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
  std::vector<uint8_t> rows = std::vector<uint8_t>(3 * kRowBytes, 7);
  TileMeta meta = {9, 60, 0};
  std::vector<uint64_t> keys = {(2ull << 32) | 5, (2ull << 32) | 5, (3ull << 32) | 0};
  ShardRec shard = {1, 3, 4, 0};
  bool with_keys = true, with_shard = true, with_rows = true;
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
  if (s.with_rows) {
    w.add(kTileRows, s.rows.data(), s.rows.size() / kRowBytes);
    w.add(kTileMeta, &s.meta, 1);
  }
  if (s.with_keys) w.add(kTileKeys, s.keys.data(), s.keys.size());
  if (s.with_shard) w.add(kShardRec, &s.shard, 1);
  return w.finish();
}

static std::string check(const std::vector<uint8_t>& b, uint64_t* shard = nullptr) {
  // an exact-size copy on the heap: a read past the end is a sanitizer error
  std::vector<uint8_t> c(b.begin(), b.end());
  c.shrink_to_fit();
  uint64_t info[9];
  return check_host(c.data(), c.size(), info, 0, shard);
}

static void expect(const char* what, const std::string& got, const std::string& want) {
  if (got != want) { std::printf("FAIL %s: got \"%s\", want \"%s\"\n", what, got.c_str(), want.c_str()); ++g_fail; }
}

static std::string forged(const std::function<void(State&)>& f) {
  State s;
  f(s);
  return check(write(s));
}

int main() {
  const State ok;
  const std::vector<uint8_t> good = write(ok);
  {
    uint64_t info[9], shard[3] = {9, 9, 9};
    CHECK(check_host(good.data(), good.size(), info, 0, shard).empty());
    CHECK(info[0] == kVersion && info[1] == good.size() && info[2] == 3 && info[3] == 2 && info[4] == 5 && info[5] == 3);
    CHECK(shard[0] == 1 && shard[1] == 3 && shard[2] == 4);
    CHECK(check_host(good.data(), good.size(), info).empty());   // (the short call accepts it too)
    Table t;
    CHECK(parse_table(good.data(), good.size(), t).empty());
    CHECK(t.has[kTileKeys] && t.has[kShardRec] && t.ent[kTileKeys].count == t.rows() && t.h.version == 1 && t.h.n_sections == 12);
    CHECK(elem_size(kTileKeys) == 8 && elem_size(kShardRec) == 16 && kTileKeys == 11 && kShardRec == 12);
  }
  // the ten-kind blob is today's blob: accepted, and no shard is reported
  {
    State s;
    s.with_keys = s.with_shard = false;
    uint64_t shard[3] = {9, 9, 9};
    const std::vector<uint8_t> b = write(s);
    CHECK(check(b, shard).empty());
    CHECK(shard[0] == 0 && shard[1] == 0 && shard[2] == 0);
    Table t;
    CHECK(parse_table(b.data(), b.size(), t).empty() && t.h.n_sections == 10 && !t.has[kTileKeys] && !t.has[kShardRec]);
  }
  // an empty store's shard: no rows, no keys, the record alone
  CHECK(forged([](State& s) { s.rows.clear(); s.keys.clear(); }).empty());
  // each new clause, broken alone
  expect("key count", forged([](State& s) { s.keys.pop_back(); }), "snapshot: the tile keys' count is not the row count");
  expect("key count +", forged([](State& s) { s.keys.push_back(7); }), "snapshot: the tile keys' count is not the row count");
  expect("padding key", forged([](State& s) { s.keys[1] = ~0ull; }), "snapshot: a tile row's key is the padding key");
  expect("keys alone", forged([](State& s) { s.with_shard = false; }), "snapshot: tile keys without a shard record");
  expect("record alone", forged([](State& s) { s.with_keys = false; }), "snapshot: a shard record without tile keys");
  expect("no rows", forged([](State& s) { s.with_rows = false; }), "snapshot: tile keys and a shard record without tile rows");
  expect("rank", forged([](State& s) { s.shard.rank = 3; }), "snapshot: the shard record's rank is not below its nranks");
  expect("rank >", forged([](State& s) { s.shard.rank = 200; }), "snapshot: the shard record's rank is not below its nranks");
  expect("nranks", forged([](State& s) { s.shard.nranks = 17; }), "snapshot: the shard record's nranks is 0 or above 16");
  expect("nranks 16", forged([](State& s) { s.shard.nranks = 16; s.shard.rank = 15; }), "");
  // (rank 0 of 0 ranks: the lower bit, the rank's, is the one reported)
  expect("nranks 0", forged([](State& s) { s.shard.nranks = 0; s.shard.rank = 0; }), "snapshot: the shard record's rank is not below its nranks");
  expect("padding", forged([](State& s) { s.shard.pad = 1u << 31; }), "snapshot: the shard record's padding is not zero");
  // the lowest bit first: a padding key before a bad record, an older clause before both
  expect("order", forged([](State& s) { s.keys[0] = ~0ull; s.shard.pad = 1; }), "snapshot: a tile row's key is the padding key");
  expect("order 2", forged([](State& s) { s.rec[0].cnt = 0; s.shard.pad = 1; }), "snapshot: a session record has a cnt of 0");
  // two records in kind 12
  {
    State s;
    const ShardRec two[2] = {s.shard, s.shard};
    Writer w;
    w.add(kTileRows, s.rows.data(), s.rows.size() / kRowBytes);
    w.add(kTileMeta, &s.meta, 1);
    w.add(kTileKeys, s.keys.data(), s.keys.size());
    w.add(kShardRec, two, 2);
    expect("two records", check(w.finish()), "snapshot: the shard record is not one record");
  }
  // every single flipped bit of the two new sections
  {
    Table t;
    CHECK(parse_table(good.data(), good.size(), t).empty());
    for (uint32_t k : {(uint32_t)kTileKeys, (uint32_t)kShardRec})
      for (uint64_t bit = t.ent[k].off * 8; bit < (t.ent[k].off + t.ent[k].bytes) * 8; ++bit) {
        std::vector<uint8_t> b = good;
        b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
        expect("flipped bit", check(b), "snapshot: a section's checksum does not match");
      }
  }
  // every truncation
  for (size_t n = 0; n < good.size(); ++n) {
    const std::vector<uint8_t> cut(good.begin(), good.begin() + n);
    if (check(cut).empty()) { std::printf("FAIL truncation to %zu accepted\n", n); ++g_fail; }
  }
  // the messages of the new bits are distinct and none is the fallback
  for (uint32_t a = 0; a < kENumErr; ++a) {
    CHECK(std::string(message(a)) != "snapshot: unknown error");
    for (uint32_t b = a + 1; b < kENumErr; ++b) CHECK(std::string(message(a)) != message(b));
  }
  if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
  std::printf("snapshot shard ok\n");
  return 0;
}
