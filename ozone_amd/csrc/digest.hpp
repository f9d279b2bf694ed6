// Launch-side interface of the SHA-256 / MD5 window-digest kernels in digest.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ozec {

// Per-window digest job over equally sized cells: cell c at base + c * cell_stride, `len` bytes each, windows of bpc
// bytes (the last of len - (nwin - 1) * bpc, at least 1).  Any byte address and any cell_stride >= len.
struct DigestArgs {
  const uint8_t *base;
  int64_t cell_stride;
  int64_t ncells;
  int64_t len;
  int64_t bpc;
  int64_t nwin;  // ceil(len / bpc)
  // compute mode (expected == null): out[c][w][digest_len], dense, the bytes of MessageDigest.digest()
  uint8_t *out;
  // verify mode: compare with expected[c][w][digest_len] and atomicMin the window index into mismatch[c], which the
  // caller pre-fills with INT32_MAX and finishes with launch_finish_mismatch (kernels.hpp)
  const uint8_t *expected;
  int32_t *mismatch;
};

// algo: digest::kSha256 / digest::kMd5 (digest_core.hpp)
hipError_t launch_digest_windows(int algo, const DigestArgs &a, hipStream_t stream);

}  // namespace ozec
