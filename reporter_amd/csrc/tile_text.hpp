// tile_text.hpp — the text of the streaming anonymiser's tile files (DESIGN.md §3 rule 13;
// reference Segment.java:55-74, AnonymisingProcessor.java:177-187): decimal digit counts, the
// integer writers, the length and the bytes of one CSV row and of one file name.  Everything is
// __host__ __device__ and free of HIP types, so the host program tests/cpp/tile_text_test.cpp runs
// exactly the code the kernels of tilestore.hip run.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TT_HD __host__ __device__ __forceinline__
#else
#define TT_HD static inline
#endif

namespace rm {

constexpr uint64_t kTtInvalidId = 0x3fffffffffffull;   // Segment.java:16: printed as an empty field
constexpr uint32_t kTtMaxSource = 64, kTtMaxMode = 16;

// what every row of a flush shares; passed to the kernels by value
struct TileText {
  uint64_t quantisation;
  uint32_t source_len, mode_len;
  char source[kTtMaxSource];
  char mode[kTtMaxMode];   // upper-cased at creation (AnonymisingProcessor.java:81)
};

// one row of the store: a segment in one of the time buckets it touches, with the values its
// line prints already worked out
struct TileStoreRow {
  uint64_t id, next_id;
  int64_t start, end;                 // floor(min), ceil(max)
  int32_t duration, length, queue;    // Math.round(max - min) as Double.intValue leaves it
  uint32_t tile;                      // id & 0x1FFFFFF
  uint64_t bucket;                    // time_range_start / quantisation
  uint64_t arrival;                   // running number of the segment that made the row
};
static_assert(sizeof(TileStoreRow) == 64, "TileStoreRow is four dwordx4");

// longest texts (signs allowed for, although no stored row has one)
constexpr uint32_t kTtMaxRow = 1 + 19 + 1 + 19 + 1 + 11 + 1 + 2 + 11 + 1 + 11 + 1 + 20 + 1 + 20 + 1 + kTtMaxSource + 1 + kTtMaxMode;
constexpr uint32_t kTtMaxName = 20 + 1 + 20 + 1 + 1 + 1 + 7;

TT_HD const char* tt_header() {   // Segment.java:55-57
  return "segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,source,"
         "vehicle_type";
}
constexpr uint32_t kTtHeaderLen = 117;

// decimal digits of v (1 for 0): nineteen comparisons, no loop and no branch
TT_HD uint32_t tt_digits(uint64_t v) {
  uint32_t n = 1;
  uint64_t p = 10;
  for (int i = 0; i < 19; ++i) {
    n += v >= p ? 1u : 0u;
    p *= 10ull;   // (the product after 10^19 is not used)
  }
  return n;
}
TT_HD uint32_t tt_len_i64(int64_t v) {
  return v < 0 ? 1u + tt_digits(0ull - (uint64_t)v) : tt_digits((uint64_t)v);
}

// the decimal text of v at p; returns its length (== tt_digits(v))
TT_HD uint32_t tt_put_u64(char* p, uint64_t v) {
  const uint32_t n = tt_digits(v);
  for (uint32_t i = n; i-- > 0u;) {
    p[i] = (char)('0' + (uint32_t)(v % 10ull));
    v /= 10ull;
  }
  return n;
}
TT_HD uint32_t tt_put_i64(char* p, int64_t v) {
  if (v >= 0) return tt_put_u64(p, (uint64_t)v);
  *p = '-';
  return 1u + tt_put_u64(p + 1, 0ull - (uint64_t)v);
}

// Segment.valid() (Segment.java:38-40)
TT_HD bool tt_valid(double mn, double mx, int32_t length, int32_t queue) {
  return mn > 0 && mx > 0 && mx > mn && length > 0 && queue >= 0;
}

// new Double(Math.round(max - min)).intValue() (Segment.java:65-66) for 0 <= d < 2^53: the
// nearest integer, ties up, saturated at Integer.MAX_VALUE.  d - floor(d) is exact, so a value
// just below x.5 stays below it (no d + 0.5 that could round up).
TT_HD int32_t tt_duration(double mn, double mx) {
  const double d = mx - mn;
  const double fl = __builtin_floor(d);
  const double r = fl + ((d - fl) >= 0.5 ? 1.0 : 0.0);
  if (!(r < 2147483647.0)) return 2147483647;
  if (!(r > -2147483648.0)) return (int32_t)(-2147483647 - 1);
  return (int32_t)r;
}

// bytes of one row: "\n<id>,<next_id or empty>,<duration>,1,<length>,<queue>,<start>,<end>,<source>,<mode>"
TT_HD uint32_t tt_row_len(const TileStoreRow& r, const TileText& t) {
  return 11u + tt_digits(r.id) + (r.next_id == kTtInvalidId ? 0u : tt_digits(r.next_id)) + tt_len_i64(r.duration) +
         tt_len_i64(r.length) + tt_len_i64(r.queue) + tt_len_i64(r.start) + tt_len_i64(r.end) + t.source_len + t.mode_len;
}

TT_HD uint32_t tt_put_row(char* p, const TileStoreRow& r, const TileText& t) {
  char* const p0 = p;
  *p++ = '\n';
  p += tt_put_u64(p, r.id);
  *p++ = ',';
  if (r.next_id != kTtInvalidId) p += tt_put_u64(p, r.next_id);
  *p++ = ',';
  p += tt_put_i64(p, r.duration);
  *p++ = ','; *p++ = '1'; *p++ = ',';
  p += tt_put_i64(p, r.length);
  *p++ = ',';
  p += tt_put_i64(p, r.queue);
  *p++ = ',';
  p += tt_put_i64(p, r.start);
  *p++ = ',';
  p += tt_put_i64(p, r.end);
  *p++ = ',';
  for (uint32_t i = 0; i < t.source_len; ++i) *p++ = t.source[i];
  *p++ = ',';
  for (uint32_t i = 0; i < t.mode_len; ++i) *p++ = t.mode[i];
  return (uint32_t)(p - p0);
}

// "<start>_<start + q - 1>/<level>/<tile index>" (AnonymisingProcessor.java:185-187)
TT_HD uint32_t tt_name_len(uint64_t bucket, uint32_t tile, const TileText& t) {
  const uint64_t s = bucket * t.quantisation;
  return tt_digits(s) + 1u + tt_digits(s + t.quantisation - 1ull) + 1u + 1u + 1u + tt_digits((tile >> 3) & 0x3FFFFFu);
}
TT_HD uint32_t tt_put_name(char* p, uint64_t bucket, uint32_t tile, const TileText& t) {
  char* const p0 = p;
  const uint64_t s = bucket * t.quantisation;
  p += tt_put_u64(p, s);
  *p++ = '_';
  p += tt_put_u64(p, s + t.quantisation - 1ull);
  *p++ = '/';
  p += tt_put_u64(p, tile & 7u);
  *p++ = '/';
  p += tt_put_u64(p, (tile >> 3) & 0x3FFFFFu);
  return (uint32_t)(p - p0);
}

// What the kept row k of a flush adds to the reply blob ("name\0body\0" per file, files in order).
// The first kept row of a file carries the previous file's closing \0 (not before the first
// file), the file's name, a \0 and the header; the very last row carries the final \0.
TT_HD uint32_t tt_piece_len(const TileStoreRow& r, const TileText& t, bool file_first, bool blob_first, bool blob_last) {
  uint32_t n = tt_row_len(r, t);
  if (file_first) n += (blob_first ? 0u : 1u) + tt_name_len(r.bucket, r.tile, t) + 1u + kTtHeaderLen;
  return n + (blob_last ? 1u : 0u);
}
TT_HD uint32_t tt_put_piece(char* p, const TileStoreRow& r, const TileText& t, bool file_first, bool blob_first, bool blob_last) {
  char* const p0 = p;
  if (file_first) {
    if (!blob_first) *p++ = 0;
    p += tt_put_name(p, r.bucket, r.tile, t);
    *p++ = 0;
    const char* h = tt_header();
    for (uint32_t i = 0; i < kTtHeaderLen; ++i) *p++ = h[i];
  }
  p += tt_put_row(p, r, t);
  if (blob_last) *p++ = 0;
  return (uint32_t)(p - p0);
}
constexpr uint32_t kTtMaxPiece = kTtMaxRow + 1 + kTtMaxName + 1 + kTtHeaderLen + 1;

}  // namespace rm
