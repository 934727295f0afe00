// The text routines of the tile store (reporter_amd/csrc/tile_text.hpp) on the host: the same
// code the kernels of tilestore.hip run.  For every decimal digit count and both edges of each,
// the length functions must equal the bytes written, the bytes must equal snprintf's, and nothing
// may be written outside [offset, offset + length) of a guarded buffer.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tile_text.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);             \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

constexpr size_t kGuard = 64, kBuf = 1024;
constexpr unsigned char kFill = 0xA5;

// run `put` at every offset 0..16 of a guarded buffer; the bytes written must be `want` and
// every other byte must keep the fill
template <class F>
static void guarded(const std::string& want, uint32_t said_len, F put) {
  CHECK(said_len == want.size());
  for (size_t off = 0; off <= 16; ++off) {
    std::vector<unsigned char> b(kGuard + kBuf + kGuard, kFill);
    char* p = (char*)b.data() + kGuard + off;
    const uint32_t n = put(p);
    CHECK(n == want.size());
    CHECK(std::memcmp(p, want.data(), want.size()) == 0);
    for (size_t i = 0; i < b.size(); ++i) {
      const bool inside = i >= kGuard + off && i < kGuard + off + want.size();
      if (!inside) CHECK(b[i] == kFill);
    }
  }
}

static TileText make_text(const char* source, const char* mode, uint64_t q) {
  TileText t;
  std::memset(&t, 0, sizeof t);
  t.quantisation = q;
  t.source_len = (uint32_t)std::strlen(source);
  t.mode_len = (uint32_t)std::strlen(mode);
  std::memcpy(t.source, source, t.source_len);
  std::memcpy(t.mode, mode, t.mode_len);
  return t;
}

static std::string row_want(const TileStoreRow& r, const char* source, const char* mode) {
  char buf[512];
  char nxt[32] = "";
  if (r.next_id != kTtInvalidId) std::snprintf(nxt, sizeof nxt, "%" PRIu64, r.next_id);
  std::snprintf(buf, sizeof buf, "\n%" PRIu64 ",%s,%d,1,%d,%d,%" PRId64 ",%" PRId64 ",%s,%s", r.id, nxt, r.duration, r.length,
                r.queue, r.start, r.end, source, mode);
  return buf;
}

static std::string name_want(uint64_t bucket, uint32_t tile, uint64_t q) {
  char buf[128];
  std::snprintf(buf, sizeof buf, "%" PRIu64 "_%" PRIu64 "/%u/%u", bucket * q, bucket * q + q - 1, tile & 7u, (tile >> 3) & 0x3FFFFFu);
  return buf;
}

int main() {
  CHECK(std::strlen(tt_header()) == kTtHeaderLen);
  // ---- the values: 0, both edges of every digit count, 2^63 - 1, the invalid id
  std::vector<uint64_t> vals = {0ull, 0x7fffffffffffffffull, kTtInvalidId, kTtInvalidId - 1, kTtInvalidId + 1, 0xffffffffffffffffull};
  uint64_t p = 1;
  for (int k = 1; k <= 19; ++k) {
    p *= 10ull;                // 10^k
    vals.push_back(p - 1);     // k digits
    vals.push_back(p);         // k + 1 digits
  }
  for (uint64_t v : vals) {
    char buf[32];
    const int n = std::snprintf(buf, sizeof buf, "%" PRIu64, v);
    CHECK((int)tt_digits(v) == n);
    guarded(buf, tt_digits(v), [&](char* q) { return tt_put_u64(q, v); });
  }
  const std::vector<int64_t> ivals = {0, 1, -1, 9, 10, 2147483647ll, -2147483648ll, 999999999ll, 1000000000ll,
                                      9007199254740992ll, -9007199254740992ll, INT64_MAX, INT64_MIN};
  for (int64_t v : ivals) {
    char buf[32];
    const int n = std::snprintf(buf, sizeof buf, "%" PRId64, v);
    CHECK((int)tt_len_i64(v) == n);
    guarded(buf, tt_len_i64(v), [&](char* q) { return tt_put_i64(q, v); });
  }
  // ---- rows: every value as the id and as the next_id, the i32 extremes in the three i32 columns
  const std::string s64(64, 's'), m16(16, 'M');
  const char* sources[] = {"s", s64.c_str()};
  const char* modes[] = {"AUTO", m16.c_str()};
  const int32_t i32s[] = {0, 1, 9, 10, 999999999, 1000000000, 2147483647, (int32_t)(-2147483647 - 1), -1};
  uint64_t rows = 0;
  for (int si = 0; si < 2; ++si) {
    const TileText t = make_text(sources[si], modes[si], si ? 60 : 3600);
    for (size_t a = 0; a < vals.size(); ++a) {
      for (int32_t x : i32s) {
        TileStoreRow r;
        std::memset(&r, 0, sizeof r);
        r.id = vals[a];
        r.next_id = vals[(a * 7 + 3) % vals.size()];
        if (x & 1) r.next_id = kTtInvalidId;
        r.duration = x; r.length = (int32_t)(x ^ 0x55); r.queue = x;
        r.start = (int64_t)(vals[a] >> 11); r.end = r.start + 1;
        const std::string want = row_want(r, sources[si], modes[si]);
        CHECK(want.size() <= kTtMaxRow);
        guarded(want, tt_row_len(r, t), [&](char* q) { return tt_put_row(q, r, t); });
        // the piece a row adds to the blob, in its four settings
        r.bucket = (vals[a] >> 11) / t.quantisation;   // bucket * q < 2^53
        r.tile = (uint32_t)(vals[a] & 0x1FFFFFFull);
        const std::string name = name_want(r.bucket, r.tile, t.quantisation);
        CHECK(name.size() <= kTtMaxName);
        guarded(name, tt_name_len(r.bucket, r.tile, t), [&](char* q) { return tt_put_name(q, r.bucket, r.tile, t); });
        for (int f = 0; f < 8; ++f) {
          const bool file_first = f & 1, blob_first = (f & 2) && file_first, blob_last = f & 4;
          std::string piece;
          if (file_first) {
            if (!blob_first) piece += '\0';
            piece += name;
            piece += '\0';
            piece += tt_header();
          }
          piece += want;
          if (blob_last) piece += '\0';
          CHECK(piece.size() <= kTtMaxPiece);
          guarded(piece, tt_piece_len(r, t, file_first, blob_first, blob_last),
                  [&](char* q) { return tt_put_piece(q, r, t, file_first, blob_first, blob_last); });
        }
        ++rows;
      }
    }
  }
  // ---- Math.round(max - min) as an int: ties up, just below a tie down, saturation
  CHECK(tt_duration(1.0, 1.5) == 1 && tt_duration(1.0, 2.5) == 2 && tt_duration(1.0, 3.5) == 3);
  CHECK(tt_duration(0.0, 0.49999999999999994) == 0 && tt_duration(0.0, 2.4999999999999996) == 2);
  CHECK(tt_duration(3599.25, 3600.75) == 2);
  CHECK(tt_duration(1.0, 1.0 + 3e9) == 2147483647);
  CHECK(tt_duration(1.0, 2147483647.5) == 2147483647 && tt_duration(1.0, 2147483647.0) == 2147483646);
  CHECK(tt_valid(1.0, 2.0, 1, 0) && !tt_valid(0.0, 2.0, 1, 0) && !tt_valid(2.0, 2.0, 1, 0) && !tt_valid(1.0, 2.0, 0, 0) &&
        !tt_valid(1.0, 2.0, 1, -1));
  if (g_fail) return 1;
  std::printf("tile text ok (%zu values, %" PRIu64 " rows)\n", vals.size(), rows);
  return 0;
}
