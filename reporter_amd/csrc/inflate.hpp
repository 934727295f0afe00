// inflate.hpp — rule 20's two decoders (inflate.hip): the host pool running inflate_core.hpp per
// chunk, and k_inflate running it a wave per chunk, its output left on the device for
// k_text_gather to put end to end (Matcher::parse_text, rm_inflate).
#pragma once
#include <stdint.h>

#include <vector>

#include "dev_util.hpp"

namespace rm {

// RM_INFLATE_DEVICE_MIN_CHUNKS (default kInflateDeviceMinChunks): a parse call with fewer gzip
// chunks inflates them on the host pool and uploads plain text
constexpr uint32_t kInflateDeviceMinChunks = 1024;
uint32_t inflate_device_min_chunks();

struct InflateResult {
  std::vector<uint32_t> status, members;   // per chunk (rule 20's status words)
  std::vector<uint64_t> off;               // n + 1: chunk c's bytes are blob[off[c], off[c + 1]); none for a bad chunk
  std::vector<uint8_t> blob;
  uint64_t second_pass = 0;                // chunks whose slot was too small (device only)
  double ms[3] = {0.0, 0.0, 0.0};          // inflate (with the CRC, computed at the ring flush), crc (0), gather
};

// no GPU: the chunks divided over HostPool
void inflate_host(uint32_t n, const char* const* data, const uint64_t* len, InflateResult& out);
// on `device`: upload, k_inflate (twice for chunks of several members), k_text_gather, download
void inflate_device(int device, uint32_t n, const char* const* data, const uint64_t* len, InflateResult& out);

// one chunk of a k_inflate launch, and what the wave reports of it
struct InflateItem {
  const uint8_t* in;
  uint64_t in_len;
  uint8_t* out;        // 16-byte aligned
  uint64_t cap;        // bytes of out that may be written
};
struct InflateOut {
  uint64_t count;      // the chunk's inflated bytes (up to the first error), stored or not
  uint32_t status, members;
  uint32_t last;       // the last byte produced (0 for none)
  uint32_t pad;
};
struct GatherItem {
  const uint8_t* src;
  uint64_t len, dst_off;
  uint32_t tail, pad;  // tail 1: a '\n' goes after the bytes
};

// Chunks inflated on the device and left there.  run: the chunks with use[c] != 0 (null: all) are
// uploaded and decoded on st (synchronised before it returns); res[c] and item[c].out then hold
// every used chunk's status, size, last byte and bytes.  gather: the items' bytes to dst + dst_off.
// timer parts: 0 inflate, 2 gather, 3 the compressed upload.
struct InflateJob {
  DevBuf<uint8_t> in, slots, again;
  DevBuf<InflateItem> d_item;
  DevBuf<InflateOut> d_res;
  DevBuf<uint32_t> d_order;
  DevBuf<GatherItem> d_gather;
  std::vector<InflateItem> item;
  std::vector<InflateOut> res;
  uint64_t second_pass = 0, bytes_in = 0;
  void run(uint32_t n, const char* const* data, const uint64_t* len, const uint8_t* use, hipStream_t st, PartTimer& timer);
  void gather(const std::vector<GatherItem>& g, uint8_t* dst, hipStream_t st, PartTimer& timer);
};

}  // namespace rm
