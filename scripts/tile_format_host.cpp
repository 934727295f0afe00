// Host baseline of scripts/tilestore_probe.py: the rows of a flush formatted one by one with
// snprintf, the way rm_runner_tiles' format_row (stages.hip) does it -- the loop that the tile
// store's device text replaces.
//
//   tile_format_host <segments.bin> <rows> <quantisation> <source> <mode>
//
// segments.bin holds rm_tile_segment records (40 bytes).  Formats `rows` rows (the segments taken
// in turn, each with Math.round, floor and ceil as a row needs them) into one growing string and
// prints {"rows":..,"bytes":..,"ms":..}.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Seg {
  uint64_t id, next_id;
  double t0, t1;
  int32_t length, queue;
};
static_assert(sizeof(Seg) == 40, "rm_tile_segment");

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<Seg> segs;
  Seg s;
  while (std::fread(&s, sizeof s, 1, f) == 1) segs.push_back(s);
  std::fclose(f);
  const uint64_t rows = std::strtoull(argv[2], nullptr, 10);
  const std::string source = argv[4], mode = argv[5];
  if (segs.empty()) return 2;
  std::string blob;
  blob.reserve(rows * 64);
  const auto t0 = std::chrono::steady_clock::now();
  char buf[256];
  for (uint64_t k = 0; k < rows; ++k) {
    const Seg& g = segs[k % segs.size()];
    const double d = g.t1 - g.t0, fl = std::floor(d);
    const long long dur = (long long)fl + (d - fl >= 0.5 ? 1 : 0);
    int n;
    if (g.next_id == 0x3fffffffffffull)
      n = std::snprintf(buf, sizeof buf, "\n%" PRIu64 ",,%lld,1,%d,%d,%lld,%lld,", g.id, dur, g.length, g.queue,
                        (long long)std::floor(g.t0), (long long)std::ceil(g.t1));
    else
      n = std::snprintf(buf, sizeof buf, "\n%" PRIu64 ",%" PRIu64 ",%lld,1,%d,%d,%lld,%lld,", g.id, g.next_id, dur, g.length,
                        g.queue, (long long)std::floor(g.t0), (long long)std::ceil(g.t1));
    blob.append(buf, (size_t)n);
    blob += source;
    blob += ',';
    blob += mode;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"rows\": %" PRIu64 ", \"bytes\": %zu, \"ms\": %.3f}\n", rows, blob.size(), ms);
  return 0;
}
