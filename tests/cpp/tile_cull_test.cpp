// The keep rule of the privacy cull (reporter_amd/csrc/tile_cull.hpp tile_run_kept) on the host:
// the same code the kernels of stages.hip and tilestore.hip run.  Every layout of up to 3 files x
// up to 4 runs x run sizes 1-3, at privacy 1-3, is judged run by run and compared with the
// reference's loop over the rows of each file, restated as oracle/tiles_oracle.py privacy_cull
// states it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tile_cull.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);             \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

// simple_reporter.py:221-239 over one file's sorted rows (a row is its run's number: rows of one
// run are equal in (id, next_id), rows of different runs are not): bit r of the result is set iff
// run r survives
static uint32_t reference_cull(const std::vector<uint32_t>& sizes, uint32_t privacy) {
  std::vector<uint32_t> segments;
  for (uint32_t r = 0; r < sizes.size(); ++r) segments.insert(segments.end(), sizes[r], r);
  size_t start = 0, i = 0;
  while (i < segments.size()) {
    if (segments[start] != segments[i] || i == segments.size() - 1) {
      if (i == segments.size() - 1) i += 1;
      if (i - start < privacy) {
        segments.erase(segments.begin() + start, segments.begin() + i);
        i = start;
      } else {
        start = i;
      }
    }
    i += 1;
  }
  std::vector<uint32_t> left(sizes.size(), 0);
  for (uint32_t r : segments) ++left[r];
  uint32_t keep = 0;
  for (uint32_t r = 0; r < sizes.size(); ++r) {
    CHECK(left[r] == 0 || left[r] == sizes[r]);   // a run goes or stays whole
    if (left[r]) keep |= 1u << r;
  }
  return keep;
}

int main() {
  // one file's layouts: 1-4 runs of 1-3 rows, and what the reference keeps of each
  std::vector<std::vector<uint32_t>> layouts;
  for (uint32_t runs = 1; runs <= 4; ++runs) {
    uint32_t combos = 1;
    for (uint32_t r = 0; r < runs; ++r) combos *= 3;
    for (uint32_t c = 0; c < combos; ++c) {
      std::vector<uint32_t> s(runs);
      for (uint32_t r = 0, x = c; r < runs; ++r, x /= 3) s[r] = 1 + x % 3;
      layouts.push_back(s);
    }
  }
  const uint32_t nl = (uint32_t)layouts.size();
  CHECK(nl == 3 + 9 + 27 + 81);
  std::vector<uint32_t> want[4];
  for (uint32_t p = 1; p <= 3; ++p)
    for (const auto& s : layouts) want[p].push_back(reference_cull(s, p));

  // the shapes the rule exists for: a final one-row run after a short run (both go), after a
  // long run (both stay), and a file whose only run is one row
  uint64_t after_short = 0, after_long = 0, lone_row = 0, cases = 0, judged = 0;
  for (uint32_t files = 1; files <= 3; ++files) {
    uint32_t pick[3] = {0, 0, 0};
    for (;;) {
      // the runs of every file end to end, as the kernels see them
      uint32_t gpos[13], file_of[12], first_run[3], G = 0;
      gpos[0] = 0;
      for (uint32_t f = 0; f < files; ++f) {
        first_run[f] = G;
        for (uint32_t sz : layouts[pick[f]]) { file_of[G] = f; gpos[G + 1] = gpos[G] + sz; ++G; }
      }
      auto size = [&](uint32_t x) { return gpos[x + 1] - gpos[x]; };
      auto same_file = [&](uint32_t x, uint32_t y) { return file_of[x] == file_of[y]; };
      for (uint32_t p = 1; p <= 3; ++p) {
        ++cases;
        for (uint32_t g = 0; g < G; ++g) {
          const bool got = tile_run_kept(g, G, size, same_file, p);
          const uint32_t f = file_of[g];
          const bool ref = (want[p][pick[f]] >> (g - first_run[f])) & 1u;
          CHECK(got == ref);
          ++judged;
        }
        for (uint32_t f = 0; f < files; ++f) {
          const std::vector<uint32_t>& s = layouts[pick[f]];
          const size_t n = s.size();
          if (n == 1 && s[0] == 1) ++lone_row;
          if (n >= 2 && s[n - 1] == 1 && s[n - 2] + 1 < p) ++after_short;
          if (n >= 2 && s[n - 1] == 1 && s[n - 2] >= p) ++after_long;
        }
      }
      uint32_t f = 0;
      while (f < files && ++pick[f] == nl) pick[f++] = 0;
      if (f == files) break;
    }
  }
  CHECK(cases == 3ull * (120ull + 120ull * 120ull + 120ull * 120ull * 120ull));
  CHECK(after_short > 0);
  CHECK(after_long > 0);
  CHECK(lone_row > 0);
  // the three shapes by hand, at privacy 2 (and 3 for the short run): {1, 1} stays whole,
  // {1, 1} goes whole at 3, {2, 1} stays whole, {1} goes
  CHECK(reference_cull({1, 1}, 2) == 3u);
  CHECK(reference_cull({1, 1}, 3) == 0u);
  CHECK(reference_cull({2, 1}, 2) == 3u);
  CHECK(reference_cull({1}, 2) == 0u);
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("tile cull ok: %llu layouts x privacy, %llu runs judged\n", (unsigned long long)cases, (unsigned long long)judged);
  return 0;
}
