// snapshot.hpp — the stream snapshot (DESIGN.md §3 rule 15): the blob that carries the vehicle
// sessions, the vehicle directory and the tile store out of HBM and back, its checksum and its
// structural rule, shared by the kernels of snapshot.hip, the host check (rm_snapshot_check_host)
// and the host test (tests/cpp/snapshot_test.cpp), the way sess_dist.hpp and tile_text.hpp are.
//
// Layout (little-endian, every section 16-byte aligned, the padding zero, the length a multiple of 16):
//   header   magic u64 | version u32 | sections u32 | total bytes u64 | checksum of header + table u64
//   table    per section: kind u32 | element size u32 | offset u64 | bytes u64 | elements u64 | checksum u64
//   sections in increasing offset, any group absent:
//     user       kUser       opaque bytes
//     directory  kDirOff     u64 x (names + 1): the names' offsets into kDirBytes, in index order
//                kDirBytes   the names end to end (no slots, no hashes: the table is rebuilt on load)
//     sessions   kSessRec    SessRec per non-empty vehicle, by increasing vehicle
//                kSessLon, kSessLat, kSessAcc (f32), kSessTime (f64): the kept points in that order
//     tile rows  kTileRows   TileStoreRow x rows, in store order
//                kTileMeta   TileMeta: the store's running arrival number and the quantisation
//     shard      kTileKeys   u64 per row of kTileRows, rule 16's call << 32 | a, in store order
//     (rule 17)  kShardRec   ShardRec: the saving rank, the rank count, the store's add-call counter
// Checksum of a byte range: sum over its 8-byte words w_i (the last zero-padded) of
// (w_i ^ kSeed) * (2 i + 1) mod 2^64.  An odd factor is invertible, so any single flipped bit
// changes the sum; an integer sum is the same in any order, so blocks may add their parts atomically.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "rm_common.hpp"

namespace rm {
namespace snap {

constexpr uint64_t kMagic = 0x0150414e534d5253ull;   // "SRMSNAP\1"
constexpr uint32_t kVersion = 1;
constexpr uint64_t kSeed = 0x9e3779b97f4a7c15ull;
constexpr uint32_t kMaxName = 4096;   // sv::kMaxId: the longest id the line reader keeps
constexpr uint32_t kRowBytes = 64;    // sizeof(TileStoreRow)

enum Kind : uint32_t { kUser = 1, kDirOff, kDirBytes, kSessRec, kSessLon, kSessLat, kSessAcc, kSessTime, kTileRows, kTileMeta, kTileKeys, kShardRec, kNumKinds };

struct Header {
  uint64_t magic;
  uint32_t version, n_sections;
  uint64_t bytes, table_sum;
};
struct Entry {
  uint32_t kind, elem;
  uint64_t off, bytes, count, sum;
};
struct SessRec {
  uint32_t vehicle, cnt;
  float max_sep;
  uint32_t pad;
  int64_t last_update;
};
struct TileMeta {
  uint64_t arrivals;
  uint32_t quantisation, pad;
};
struct ShardRec {   // (calls < 2^32 - 1: the store numbers no more add calls)
  uint32_t rank, nranks, calls, pad;
};
constexpr uint32_t kMaxRanks = 16;
constexpr uint64_t kPadKey = ~0ull;   // the exchange's padding key (tilestore.hip kTsPadKey): no row has it
static_assert(sizeof(ShardRec) == 16, "snapshot layout");
static_assert(sizeof(Header) == 32 && sizeof(Entry) == 40 && sizeof(SessRec) == 24 && sizeof(TileMeta) == 16, "snapshot layout");

RM_HD uint32_t elem_size(uint32_t kind) {
  switch (kind) {
    case kUser: case kDirBytes: return 1u;
    case kDirOff: case kSessTime: case kTileKeys: return 8u;
    case kSessRec: return (uint32_t)sizeof(SessRec);
    case kSessLon: case kSessLat: case kSessAcc: return 4u;
    case kTileRows: return kRowBytes;
    case kTileMeta: return (uint32_t)sizeof(TileMeta);
    case kShardRec: return (uint32_t)sizeof(ShardRec);
    default: return 0u;
  }
}
RM_HD uint64_t align16(uint64_t x) { return (x + 15ull) & ~15ull; }
RM_HD uint64_t data_start(uint32_t n_sections) { return align16(sizeof(Header) + (uint64_t)n_sections * sizeof(Entry)); }

// one word's part of a checksum
RM_HD uint64_t sum_word(uint64_t w, uint64_t i) { return (w ^ kSeed) * (2ull * i + 1ull); }

// ---- the structural rule's parts that look at elements; bit k of an error word is kMessage[k],
// and the lowest bit set is the one reported, on the host and on the device alike
enum Err : uint32_t {
  kESum = 0, kECntZero, kEVehOrder, kEMaxSep, kECntSum, kETimeNaN, kEOffMono, kEOffRange, kENameLen, kEDupName, kEVehRange,
  kEPadKey, kEShardRank, kEShardRanks, kEShardPad, kEVehTwice,
  kENumErr
};
inline const char* message(uint32_t bit) {
  static const char* const m[kENumErr] = {
      "snapshot: a section's checksum does not match",
      "snapshot: a session record has a cnt of 0",
      "snapshot: session vehicle indices are not strictly increasing",
      "snapshot: a session max_sep is negative or not finite",
      "snapshot: the session records' cnt do not add up to the point count",
      "snapshot: a point time is NaN",
      "snapshot: name offsets are not monotone",
      "snapshot: name offsets do not stay inside the name bytes",
      "snapshot: a name is empty or longer than 4096 bytes",
      "snapshot: two names are equal",
      "snapshot: a vehicle index is not below the session's n_vehicles",
      "snapshot: a tile row's key is the padding key",
      "snapshot: the shard record's rank is not below its nranks",
      "snapshot: the shard record's nranks is 0 or above 16",
      "snapshot: the shard record's padding is not zero",
      "snapshot: a vehicle's session is in two blobs"};
  return bit < kENumErr ? m[bit] : "snapshot: unknown error";
}
inline const char* first_message(uint64_t bits) {
  for (uint32_t k = 0; k < kENumErr; ++k)
    if (bits >> k & 1ull) return message(k);
  return "";
}

// record i of n (n_vehicles: the loading session's, or 0 for "not known")
RM_HD uint32_t rec_bits(const SessRec* r, uint64_t i, uint32_t n_vehicles) {
  uint32_t e = 0u;
  const SessRec x = r[i];
  if (x.cnt == 0u) e |= 1u << kECntZero;
  if (i > 0 && r[i - 1].vehicle >= x.vehicle) e |= 1u << kEVehOrder;
  if (!(x.max_sep >= 0.0f) || !(x.max_sep - x.max_sep == 0.0f)) e |= 1u << kEMaxSep;
  if (n_vehicles && x.vehicle >= n_vehicles) e |= 1u << kEVehRange;
  return e;
}
// name i of n: off has n + 1 entries into n_bytes bytes
RM_HD uint32_t name_bits(const uint64_t* off, uint64_t i, uint64_t n, uint64_t n_bytes) {
  uint32_t e = 0u;
  const uint64_t a = off[i], b = off[i + 1];
  if (b < a) e |= 1u << kEOffMono;
  if ((i == 0 && a != 0) || a > n_bytes || b > n_bytes || (i + 1 == n && b != n_bytes)) e |= 1u << kEOffRange;
  if (b >= a && (b == a || b - a > kMaxName)) e |= 1u << kENameLen;
  return e;
}
RM_HD uint32_t time_bits(double t) { return t == t ? 0u : 1u << kETimeNaN; }
RM_HD uint32_t key_bits(uint64_t key) { return key == kPadKey ? 1u << kEPadKey : 0u; }
RM_HD uint32_t shard_bits(const ShardRec& x) {
  uint32_t e = 0u;
  if (x.rank >= x.nranks) e |= 1u << kEShardRank;
  if (x.nranks == 0u || x.nranks > kMaxRanks) e |= 1u << kEShardRanks;
  if (x.pad != 0u) e |= 1u << kEShardPad;
  return e;
}

// ---- host only from here
inline uint64_t checksum(const void* p, uint64_t bytes) {
  const uint8_t* s = (const uint8_t*)p;
  uint64_t sum = 0, i = 0;
  for (; (i + 1) * 8 <= bytes; ++i) {
    uint64_t w;
    std::memcpy(&w, s + i * 8, 8);
    sum += sum_word(w, i);
  }
  if (i * 8 < bytes) {
    uint64_t w = 0;
    std::memcpy(&w, s + i * 8, bytes - i * 8);
    sum += sum_word(w, i);
  }
  return sum;
}

// the checksum of header and table: the header with its own table_sum as zero, then the entries
inline uint64_t table_checksum(const Header& h, const Entry* e) {
  Header z = h;
  z.table_sum = 0;
  std::vector<uint8_t> b(sizeof(Header) + (size_t)h.n_sections * sizeof(Entry));
  std::memcpy(b.data(), &z, sizeof z);
  if (h.n_sections) std::memcpy(b.data() + sizeof z, e, (size_t)h.n_sections * sizeof(Entry));
  return checksum(b.data(), b.size());
}

// the host-checked table of a blob: ent[kind] (bytes of an absent kind: count 0, off 0) and has[kind]
struct Table {
  Header h{};
  Entry ent[kNumKinds] = {};
  bool has[kNumKinds] = {};
  uint64_t names() const { return has[kDirOff] ? ent[kDirOff].count - 1 : 0; }
  uint64_t vehicles() const { return ent[kSessRec].count; }
  uint64_t points() const { return ent[kSessTime].count; }
  uint64_t rows() const { return ent[kTileRows].count; }
};

// header and table alone (nothing here reads a section's elements but the zero padding): "" or the reason
inline std::string parse_table(const void* blob, uint64_t len, Table& t) {
  const uint8_t* s = (const uint8_t*)blob;
  if (!blob || len < sizeof(Header)) return "snapshot: shorter than its header";
  std::memcpy(&t.h, s, sizeof(Header));
  if (t.h.magic != kMagic) return "snapshot: bad magic";
  if (t.h.version != kVersion) return "snapshot: unknown format version";
  if (t.h.bytes != len) return "snapshot: its length differs from the header's";
  if (len % 16) return "snapshot: its length is not a multiple of 16";
  if (t.h.n_sections >= kNumKinds) return "snapshot: too many sections";
  const uint64_t d0 = data_start(t.h.n_sections);
  if (d0 > len) return "snapshot: the section table runs past the end";
  std::vector<Entry> e(t.h.n_sections);
  if (t.h.n_sections) std::memcpy(e.data(), s + sizeof(Header), (size_t)t.h.n_sections * sizeof(Entry));
  if (table_checksum(t.h, e.data()) != t.h.table_sum) return "snapshot: the checksum of header and table does not match";
  uint64_t at = sizeof(Header) + (uint64_t)t.h.n_sections * sizeof(Entry);   // end of what came before
  for (const Entry& x : e) {
    if (x.kind == 0 || x.kind >= kNumKinds) return "snapshot: unknown section kind";
    if (t.has[x.kind]) return "snapshot: a section kind appears twice";
    if (x.off % 16) return "snapshot: a section is misaligned";
    if (x.off > len || x.bytes > len - x.off) return "snapshot: a section runs past the end";
    if (x.off < at) return "snapshot: sections overlap";
    if (x.elem != elem_size(x.kind) || x.count > x.bytes || x.count * x.elem != x.bytes)
      return "snapshot: a section's count times size is not its bytes";
    if (x.off != align16(at)) return "snapshot: a gap between sections";
    for (uint64_t q = at; q < x.off; ++q)
      if (s[q]) return "snapshot: padding is not zero";
    at = x.off + x.bytes;
    t.has[x.kind] = true;
    t.ent[x.kind] = x;
  }
  for (uint64_t q = at; q < len; ++q)
    if (s[q]) return "snapshot: padding is not zero";
  if (len != align16(at)) return "snapshot: bytes behind the last section";
  // the groups come whole
  if (t.has[kDirOff] != t.has[kDirBytes]) return "snapshot: the directory sections are incomplete";
  const bool sess = t.has[kSessRec];
  for (uint32_t k : {(uint32_t)kSessLon, (uint32_t)kSessLat, (uint32_t)kSessAcc, (uint32_t)kSessTime})
    if (t.has[k] != sess) return "snapshot: the session sections are incomplete";
  if (t.has[kTileRows] != t.has[kTileMeta]) return "snapshot: the tile sections are incomplete";
  if (sess) {
    const uint64_t n = t.ent[kSessTime].count;
    if (t.ent[kSessLon].count != n || t.ent[kSessLat].count != n || t.ent[kSessAcc].count != n)
      return "snapshot: the point sections differ in count";
    if (n >= 0xffffffffull || t.ent[kSessRec].count >= 0x7fffffffull) return "snapshot: too many points or vehicles";
    if (t.ent[kSessRec].count > n) return message(kECntZero);
    if (t.ent[kSessRec].count == 0 && n != 0) return message(kECntSum);
  }
  if (t.has[kDirOff]) {
    if (t.ent[kDirOff].count == 0) return "snapshot: the name offsets are empty";
    if (t.ent[kDirOff].count - 1 >= 0x40000000ull || t.ent[kDirBytes].bytes >= (1ull << 32)) return "snapshot: too many names";
    if (t.ent[kDirOff].count == 1 && t.ent[kDirBytes].bytes) return message(kEOffRange);
  }
  if (t.has[kTileMeta]) {
    if (t.ent[kTileMeta].count != 1) return "snapshot: the tile store's numbers are not one record";
    if (t.ent[kTileRows].count >= 0x7fffffffull) return "snapshot: too many tile rows";
  }
  // rule 17: the keys and the shard record come together, beside tile rows, a key per row
  if (t.has[kTileKeys] && !t.has[kShardRec]) return "snapshot: tile keys without a shard record";
  if (t.has[kShardRec] && !t.has[kTileKeys]) return "snapshot: a shard record without tile keys";
  if (t.has[kShardRec]) {
    if (!t.has[kTileRows]) return "snapshot: tile keys and a shard record without tile rows";
    if (t.ent[kShardRec].count != 1) return "snapshot: the shard record is not one record";
    if (t.ent[kTileKeys].count != t.ent[kTileRows].count) return "snapshot: the tile keys' count is not the row count";
  }
  return "";
}

inline TileMeta tile_meta(const void* blob, const Table& t) {
  TileMeta m{};
  if (t.has[kTileMeta]) std::memcpy(&m, (const uint8_t*)blob + t.ent[kTileMeta].off, sizeof m);
  return m;
}

inline ShardRec shard_rec(const void* blob, const Table& t) {   // (no record: all zero, nranks 0)
  ShardRec r{};
  if (t.has[kShardRec]) std::memcpy(&r, (const uint8_t*)blob + t.ent[kShardRec].off, sizeof r);
  return r;
}

// what depends on the loading objects (0: that object is not loaded)
inline std::string check_targets(const void* blob, const Table& t, uint32_t n_vehicles, uint32_t max_vehicles, uint32_t quantisation) {
  if (max_vehicles && t.names() > max_vehicles) return "snapshot: more names than the directory's max_vehicles";
  if (quantisation && t.has[kTileMeta] && tile_meta(blob, t).quantisation != quantisation)
    return "snapshot: its quantisation is not the tile store's";
  (void)n_vehicles;   // (element-wise: rec_bits)
  return "";
}

// The whole rule on the host: header, table, checksums, elements.  info: version, bytes, names,
// vehicles, points, rows, quantisation, user offset, user bytes; shard (null: not wanted): the
// shard record's rank, nranks and calls (all 0 in a blob without one).
inline std::string check_host(const void* blob, uint64_t len, uint64_t info[9], uint32_t n_vehicles = 0, uint64_t shard[3] = nullptr) {
  Table t;
  std::string why = parse_table(blob, len, t);
  if (!why.empty()) return why;
  const uint8_t* s = (const uint8_t*)blob;
  uint64_t bits = 0;
  for (uint32_t k = 1; k < kNumKinds; ++k)
    if (t.has[k] && checksum(s + t.ent[k].off, t.ent[k].bytes) != t.ent[k].sum) bits |= 1ull << kESum;
  if (t.has[kSessRec] && !(bits & 1ull)) {
    const SessRec* r = (const SessRec*)(s + t.ent[kSessRec].off);
    const double* tm = (const double*)(s + t.ent[kSessTime].off);
    uint64_t total = 0;
    for (uint64_t i = 0; i < t.vehicles(); ++i) { bits |= rec_bits(r, i, n_vehicles); total += r[i].cnt; }
    if (total != t.points()) bits |= 1ull << kECntSum;
    for (uint64_t i = 0; i < t.points(); ++i) bits |= time_bits(tm[i]);
  }
  if (t.has[kDirOff] && !(bits & 1ull)) {
    const uint64_t* off = (const uint64_t*)(s + t.ent[kDirOff].off);
    const char* nb = (const char*)(s + t.ent[kDirBytes].off);
    const uint64_t n = t.names(), B = t.ent[kDirBytes].bytes;
    for (uint64_t i = 0; i < n; ++i) bits |= name_bits(off, i, n, B);
    if (!(bits & (1ull << kEOffMono | 1ull << kEOffRange))) {
      std::unordered_set<std::string> seen;
      for (uint64_t i = 0; i < n; ++i)
        if (!seen.emplace(nb + off[i], (size_t)(off[i + 1] - off[i])).second) bits |= 1ull << kEDupName;
    }
  }
  if (t.has[kShardRec] && !(bits & 1ull)) {
    const uint64_t* key = (const uint64_t*)(s + t.ent[kTileKeys].off);
    for (uint64_t i = 0; i < t.rows(); ++i) bits |= key_bits(key[i]);
    bits |= shard_bits(shard_rec(blob, t));
  }
  if (bits) return first_message(bits);
  if (shard) {
    const ShardRec r = shard_rec(blob, t);
    shard[0] = r.rank; shard[1] = r.nranks; shard[2] = r.calls;
  }
  if (info) {
    info[0] = t.h.version; info[1] = len; info[2] = t.names(); info[3] = t.vehicles(); info[4] = t.points();
    info[5] = t.rows(); info[6] = tile_meta(blob, t).quantisation;
    info[7] = t.has[kUser] ? t.ent[kUser].off : 0; info[8] = t.has[kUser] ? t.ent[kUser].bytes : 0;
  }
  return "";
}

// lays a blob out: add() the sections in kind order, then finish() (host writer; save() uses
// layout() for the device buffer and seal() once the sections' checksums are in place)
struct Writer {
  std::vector<Entry> ent;
  std::vector<const void*> src;
  void add(uint32_t kind, const void* p, uint64_t count) {
    Entry e{};
    e.kind = kind; e.elem = elem_size(kind); e.count = count; e.bytes = count * e.elem;
    ent.push_back(e);
    src.push_back(p);
  }
  uint64_t layout() {   // the offsets; returns the blob's length
    uint64_t at = data_start((uint32_t)ent.size());
    for (Entry& e : ent) { e.off = at; at = align16(at + e.bytes); }
    return at;
  }
  // header and table into blob[0 .. data_start): the entries' sums as they stand
  void seal(void* blob, uint64_t len) const {
    Header h{};
    h.magic = kMagic; h.version = kVersion; h.n_sections = (uint32_t)ent.size(); h.bytes = len;
    h.table_sum = table_checksum(h, ent.data());
    std::memcpy(blob, &h, sizeof h);
    if (!ent.empty()) std::memcpy((uint8_t*)blob + sizeof h, ent.data(), ent.size() * sizeof(Entry));
  }
  std::vector<uint8_t> finish() {
    const uint64_t len = layout();
    std::vector<uint8_t> b(len, 0);
    for (size_t k = 0; k < ent.size(); ++k) {
      if (ent[k].bytes) std::memcpy(b.data() + ent[k].off, src[k], ent[k].bytes);
      ent[k].sum = checksum(b.data() + ent[k].off, ent[k].bytes);
    }
    seal(b.data(), len);
    return b;
  }
};

}  // namespace snap
}  // namespace rm
