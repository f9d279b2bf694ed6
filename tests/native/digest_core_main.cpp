// Stand-alone driver of ozone_amd/csrc/digest_core.hpp for tests/test_digest_core.py (built with a plain g++ under
// AddressSanitizer + UBSan and run as a program).  Prints, one record per line:
//   abc <algo> <hex digest of "abc">
//   digest <algo> <len> <hex digest of pattern(len)>          pattern byte i = (i * 131 + (i >> 8) * 29 + 7) & 0xff
//   pad <algo> <total_len> <nblocks> <hex of the padded block(s)>   tail byte j = (j * 37 + 11) & 0xff, j < total_len % 64
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ozone_amd/csrc/digest_core.hpp"

namespace dg = ozec::digest;

static void hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}

template <int A>
static void run(const char *name) {
  uint8_t out[32];
  dg::digest_bytes<A>(reinterpret_cast<const uint8_t *>("abc"), 3, out);
  std::printf("abc %s ", name);
  hex(out, dg::Traits<A>::kDigestLen);
  std::printf("\n");
  const size_t lens[] = {1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 1000};
  for (size_t len : lens) {
    std::vector<uint8_t> v(len);  // exactly len bytes: a read past the message is an ASan report
    for (size_t i = 0; i < len; ++i) v[i] = static_cast<uint8_t>(i * 131 + (i >> 8) * 29 + 7);
    dg::digest_bytes<A>(v.data(), len, out);
    std::printf("digest %s %zu ", name, len);
    hex(out, dg::Traits<A>::kDigestLen);
    std::printf("\n");
  }
  const uint64_t totals[] = {uint64_t{1} << 29, (uint64_t{1} << 29) + 3, (uint64_t{1} << 32) + 5, (uint64_t{1} << 32) + 61};
  for (uint64_t total : totals) {
    uint8_t tail[64] = {0};
    for (uint64_t j = 0; j < (total & 63); ++j) tail[j] = static_cast<uint8_t>(j * 37 + 11);
    uint32_t t[16], b[2][16];
    std::memcpy(t, tail, 64);
    const int n = dg::final_blocks<A>(total, t, b[0], b[1]);
    std::printf("pad %s %llu %d ", name, static_cast<unsigned long long>(total), n);
    for (int k = 0; k < n; ++k) {
      uint8_t raw[64];
      std::memcpy(raw, b[k], 64);
      hex(raw, 64);
    }
    std::printf("\n");
  }
}

int main() {
  run<dg::kSha256>("sha256");
  run<dg::kMd5>("md5");
  return 0;
}
