// inflate.hip — rule 20 on the device: k_inflate decodes one gzip chunk per wave with the shared
// core (inflate_core.hpp), k_text_gather puts the inflated chunks end to end.  Streams of one
// chunk depend on each other bit by bit, so the parallelism is across chunks.
//
// Per wave in LDS: a 32 KiB window ring and the core's work area (two code sets with their
// first-level lookups, the code-length scratch): 36.4 KiB, four waves to a CU's 160 KiB.  Every
// lane runs the decoder on the same values; a literal is one ring write, a match is copied by all
// lanes (lane i takes byte i; for distance < length the source index wraps modulo the distance).
// A filled half of the ring goes to the chunk's slot in 16-byte stores and into the member's
// CRC-32 (64 slices, combined by x^(8n) mod P).  Past the slot's end the wave goes on decoding and
// counting without storing, so a chunk's true size is known after one pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>

#include "dev_util.hpp"
#include "host_pool.hpp"
#include "inflate.hpp"
#include "inflate_core.hpp"
#include "inflate_ring.hpp"

namespace rm {

namespace {

// one wave per chunk, in the order given (descending compressed size, so that the tail is short)
__global__ void __launch_bounds__(64) k_inflate(uint32_t n, const uint32_t* __restrict__ order,
                                                const InflateItem* __restrict__ item, InflateOut* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[inf::kRing];
  __shared__ inf::Work work;
  if (blockIdx.x >= n) return;
  const uint32_t c = order[blockIdx.x];
  const InflateItem it = item[c];
  inf::RingSink s;
  s.ring = ring;
  s.out = it.out;
  s.cap = it.cap;
  s.ln = threadIdx.x & 63u;
  uint32_t members = 0;
  const uint32_t status = inf::inflate_ring_chunk(it.in, it.in_len, work, s, members);
  if (s.ln == 0) {
    InflateOut o;
    o.count = s.pos;
    o.status = status;
    o.members = members;
    o.last = s.last_byte();
    o.pad = 0;
    res[c] = o;
  }
}

// chunk blockIdx.x's bytes [piece * blockIdx.y, ...) to their place in dst, then the '\n' a chunk
// lacks (tail 1)
__global__ void __launch_bounds__(256) k_text_gather(const GatherItem* __restrict__ item, uint64_t piece, uint8_t* __restrict__ dst) {
  const GatherItem g = item[blockIdx.x];
  const uint64_t a = piece * blockIdx.y;
  uint8_t* d = dst + g.dst_off;
  if (g.tail && blockIdx.y == 0 && threadIdx.x == 0) d[g.len] = '\n';
  if (a >= g.len) return;
  const uint64_t b = a + piece < g.len ? a + piece : g.len;
  for (uint64_t k = a + threadIdx.x; k < b; k += 256u) d[k] = g.src[k];
}

}  // namespace

void inflate_host(uint32_t n, const char* const* data, const uint64_t* len, InflateResult& out) {
  if (n && (!data || !len)) throw std::runtime_error("inflate: chunks are NULL");
  out = InflateResult();
  out.status.assign(n, 0);
  out.members.assign(n, 0);
  out.off.assign(n + 1ull, 0);
  std::vector<std::vector<uint8_t>> bytes(n);
  HostPool& pool = HostPool::get();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(pool.size(), n));
  std::atomic<uint32_t> next{0};
  pool.run(nt, [&](size_t) {
    for (uint32_t c; (c = next.fetch_add(1)) < n;) {
      if (len[c] && !data[c]) { out.status[c] = inf::kHeader; continue; }
      out.status[c] = inf::inflate_host_chunk((const uint8_t*)data[c], len[c], bytes[c], out.members[c]);
      if (out.status[c] != inf::kOk) std::vector<uint8_t>().swap(bytes[c]);
    }
  });
  for (uint32_t c = 0; c < n; ++c) out.off[c + 1] = out.off[c] + bytes[c].size();
  out.blob.resize(out.off[n]);
  for (uint32_t c = 0; c < n; ++c)
    if (!bytes[c].empty()) std::memcpy(out.blob.data() + out.off[c], bytes[c].data(), bytes[c].size());
}

uint32_t inflate_device_min_chunks() {
  if (const char* e = std::getenv("RM_INFLATE_DEVICE_MIN_CHUNKS")) {
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    if (end != e && v >= 0 && v <= 0x7fffffffl) return (uint32_t)v;
  }
  return kInflateDeviceMinChunks;
}

void InflateJob::run(uint32_t n, const char* const* data, const uint64_t* len, const uint8_t* use, hipStream_t st, PartTimer& timer) {
  second_pass = 0;
  bytes_in = 0;
  item.assign(n, InflateItem{nullptr, 0, nullptr, 0});
  res.assign(n, InflateOut{0, 0, 0, 0, 0});
  // ---- the compressed bytes, each chunk at a multiple of 16; slots from the trailers
  std::vector<uint32_t> order;
  std::vector<uint64_t> in_off(n, 0), slot_off(n, 0);
  uint64_t in_all = 0, slot_all = 0;
  for (uint32_t c = 0; c < n; ++c) {
    if (use && !use[c]) continue;
    if (len[c] && !data[c]) throw std::runtime_error("inflate: chunk is NULL");
    order.push_back(c);
    in_off[c] = in_all;
    slot_off[c] = slot_all;
    item[c].in_len = len[c];
    item[c].cap = inf::isize_hint((const uint8_t*)data[c], len[c]);
    in_all += (len[c] + 15ull) & ~15ull;
    slot_all += (item[c].cap + 15ull) & ~15ull;
    bytes_in += len[c];
  }
  if (order.empty()) return;
  if (slot_all > inf::kMaxOut) {
    // the trailers promise more than a call may hold: some of them lie (a valid call's would not).
    // No slot is taken on trust then: every wave counts, and the second pass stores into exact slots
    for (uint32_t c : order) { item[c].cap = 0; slot_off[c] = 0; }
    slot_all = 0;
  }
  if (in.cap() < in_all + 16) in.reserve(in_all + 16);
  if (slots.cap() < slot_all + 16) slots.reserve(slot_all + 16);
  if (d_item.cap() < n) { d_item.reserve(n); d_res.reserve(n); d_order.reserve(n); }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
  timer.tic(3, st);
  for (uint32_t c : order) {
    if (len[c]) RM_HIP(hipMemcpyAsync(in + in_off[c], data[c], len[c], hipMemcpyHostToDevice, st));
    item[c].in = in + in_off[c];
    item[c].out = slots + slot_off[c];
  }
  timer.toc(st);
  auto launch = [&](uint32_t m) {
    RM_HIP(hipMemcpyAsync(d_item, item.data(), n * sizeof(InflateItem), hipMemcpyHostToDevice, st));
    RM_HIP(hipMemcpyAsync(d_order, order.data(), m * 4ull, hipMemcpyHostToDevice, st));
    timer.tic(0, st);
    hipLaunchKernelGGL(k_inflate, dim3(m), dim3(64), 0, st, m, d_order, d_item, d_res);
    RM_HIP(hipGetLastError());
    timer.toc(st);
    RM_HIP(hipStreamSynchronize(st));
    // (the waves wrote the launched chunks' entries only)
    std::vector<InflateOut> got(n);
    RM_HIP(hipMemcpy(got.data(), d_res, n * sizeof(InflateOut), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < m; ++k) res[order[k]] = got[order[k]];
  };
  launch((uint32_t)order.size());
  // ---- chunks that outgrew their slot (several members: the last trailer undercounts) once more
  std::vector<uint32_t> more;
  uint64_t extra = 0;
  for (uint32_t c : order)
    if (res[c].status == inf::kOk && res[c].count > item[c].cap) {
      more.push_back(c);
      extra += (res[c].count + 15ull) & ~15ull;
    }
  if (more.empty()) return;
  if (extra > inf::kMaxOut) throw std::runtime_error(std::string("gzip: ") + inf::status_text(inf::kTooLarge));
  if (again.cap() < extra + 16) again.reserve(extra + 16);
  uint64_t at = 0;
  for (uint32_t c : more) {
    item[c].out = again + at;
    item[c].cap = res[c].count;
    at += (res[c].count + 15ull) & ~15ull;
  }
  order = more;
  launch((uint32_t)more.size());
  for (uint32_t c : more)
    if (res[c].status != inf::kOk || res[c].count != item[c].cap) throw std::runtime_error("inflate: the second pass disagrees with the first");
  second_pass = more.size();
}

void InflateJob::gather(const std::vector<GatherItem>& g, uint8_t* dst, hipStream_t st, PartTimer& timer) {
  if (g.empty()) return;
  uint64_t longest = 0;
  for (const GatherItem& x : g) longest = std::max(longest, x.len);
  if (d_gather.cap() < g.size()) d_gather.reserve(g.size());
  RM_HIP(hipMemcpyAsync(d_gather, g.data(), g.size() * sizeof(GatherItem), hipMemcpyHostToDevice, st));
  const uint64_t piece = std::max<uint64_t>(inf::kHalf, (longest + 65534ull) / 65535ull);
  const uint32_t rows = (uint32_t)((longest + piece - 1) / piece);
  timer.tic(2, st);
  hipLaunchKernelGGL(k_text_gather, dim3((uint32_t)g.size(), std::max(rows, 1u)), dim3(256), 0, st, d_gather.get(), piece, dst);
  RM_HIP(hipGetLastError());
  timer.toc(st);
  RM_HIP(hipStreamSynchronize(st));   // (g's upload is read from pageable memory until then)
}

void inflate_device(int device, uint32_t n, const char* const* data, const uint64_t* len, InflateResult& out) {
  if (n && (!data || !len)) throw std::runtime_error("inflate: chunks are NULL");
  out = InflateResult();
  out.status.assign(n, 0);
  out.members.assign(n, 0);
  out.off.assign(n + 1ull, 0);
  if (n == 0) return;
  RM_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  InflateJob job;
  PartTimer timer;
  job.run(n, data, len, nullptr, st, timer);
  out.second_pass = job.second_pass;
  // ---- end to end, then down
  std::vector<GatherItem> g;
  for (uint32_t c = 0; c < n; ++c) {
    out.status[c] = job.res[c].status;
    out.members[c] = job.res[c].members;
    const uint64_t m = job.res[c].status == inf::kOk ? job.res[c].count : 0;
    out.off[c + 1] = out.off[c] + m;
    if (m) g.push_back(GatherItem{job.item[c].out, m, out.off[c], 0, 0});
  }
  if (out.off[n] > inf::kMaxOut) throw std::runtime_error(std::string("gzip: ") + inf::status_text(inf::kTooLarge));
  if (out.off[n]) {
    DevBuf<uint8_t> flat(out.off[n]);
    job.gather(g, flat, st, timer);
    out.blob.resize(out.off[n]);
    RM_HIP(hipMemcpy(out.blob.data(), flat, out.off[n], hipMemcpyDeviceToHost));
  }
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  timer.harvest(ms);
  std::copy(ms, ms + 3, out.ms);
}

}  // namespace rm
