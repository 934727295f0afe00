// zlib's own inflate over a directory of one-member .gz files on T host threads: the baseline the
// device inflate (DESIGN.md §3 rule 20, §5) is compared with.  Not the code under test.
//
//   zlib_inflate_bench <dir> [threads=16] [repeats=5]
//
// The files are read into memory first; a repeat is the wall time from the first thread's start to
// the last one's end, files handed out largest first from one counter.  Prints one JSON line.
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <string>
#include <thread>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: zlib_inflate_bench <dir> [threads] [repeats]\n"); return 2; }
  const int threads = argc > 2 ? std::max(1, std::atoi(argv[2])) : 16;
  const int repeats = argc > 3 ? std::max(1, std::atoi(argv[3])) : 5;
  std::vector<std::vector<uint8_t>> in;
  DIR* d = opendir(argv[1]);
  if (!d) { std::perror(argv[1]); return 2; }
  while (dirent* e = readdir(d)) {
    const std::string name = e->d_name;
    if (name.size() < 3 || name.substr(name.size() - 3) != ".gz") continue;
    FILE* f = std::fopen((std::string(argv[1]) + "/" + name).c_str(), "rb");
    if (!f) continue;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> b((size_t)n);
    if (n && std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) { std::fclose(f); return 2; }
    std::fclose(f);
    in.push_back(std::move(b));
  }
  closedir(d);
  std::sort(in.begin(), in.end(), [](const auto& a, const auto& b) { return a.size() > b.size(); });
  std::vector<std::vector<uint8_t>> out(in.size());
  uint64_t bytes_in = 0, bytes_out = 0;
  for (size_t i = 0; i < in.size(); ++i) {
    const auto& z = in[i];
    if (z.size() < 18) return 2;
    const uint32_t isize = (uint32_t)z[z.size() - 4] | ((uint32_t)z[z.size() - 3] << 8) | ((uint32_t)z[z.size() - 2] << 16) | ((uint32_t)z[z.size() - 1] << 24);
    out[i].resize(isize + 1u);
    bytes_in += z.size();
    bytes_out += isize;
  }
  std::vector<double> ms;
  std::atomic<int> bad{0};
  for (int r = 0; r < repeats + 1; ++r) {   // (the first run touches the output pages and is dropped)
    std::atomic<size_t> next{0};
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
      pool.emplace_back([&] {
        for (size_t i; (i = next.fetch_add(1)) < in.size();) {
          z_stream s{};
          if (inflateInit2(&s, 31) != Z_OK) { ++bad; return; }
          s.next_in = in[i].data();
          s.avail_in = (uInt)in[i].size();
          s.next_out = out[i].data();
          s.avail_out = (uInt)out[i].size();
          if (inflate(&s, Z_FINISH) != Z_STREAM_END || s.total_out + 1 != out[i].size()) ++bad;
          inflateEnd(&s);
        }
      });
    for (auto& t : pool) t.join();
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r) ms.push_back(dt);
  }
  if (bad) { std::fprintf(stderr, "%d files did not inflate\n", (int)bad); return 1; }
  std::printf("{\"files\": %zu, \"threads\": %d, \"bytes_in\": %llu, \"bytes_out\": %llu, \"zlib\": \"%s\", \"ms\": [", in.size(), threads,
              (unsigned long long)bytes_in, (unsigned long long)bytes_out, zlibVersion());
  for (size_t i = 0; i < ms.size(); ++i) std::printf("%s%.3f", i ? ", " : "", ms[i]);
  std::printf("]}\n");
  return 0;
}
