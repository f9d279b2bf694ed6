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

// Per-window digest job over stripes (the fused encode / reconstruct / stripe-queue forms): logical cell (s, j), digest
// unit j of `nunits` per stripe, lies at buf[unit[j].buf] + unit[j].off + s * stripe_stride[unit[j].buf]; `len` bytes
// each, windows as in DigestArgs.  The lane of (s, j, w) is (s * nunits + j) * nwin + w, so one launch covers data and
// coded units in two allocations.  The unit table travels in the kernel arguments: no device allocation per call.
constexpr int kDigestMaxUnits = 64 + 16;  // OZEC_MAX_K + OZEC_MAX_ROWS
struct DigestUnit {
  int64_t off;      // byte offset of the unit in stripe 0 from its buffer's base
  uint8_t buf;      // 0 / 1: which of the two buffers
  uint8_t verify;   // 0: compute -> out[s][slot][w][digest_len]; 1: compare with expected[s][slot][w][digest_len]
  uint16_t slot;    // compute: index among the out_units digests a stripe writes; verify: the stripe-unit number, which
                    // also indexes `expected` and goes into the mismatch report
  uint32_t pad_;
};
struct DigestStripeArgs {
  const uint8_t *buf[2];
  int64_t stripe_stride[2];
  int64_t nstripes;
  int64_t len;
  int64_t bpc;
  int64_t nwin;
  int32_t nunits;
  int32_t out_units;  // units per stripe in `out`
  int32_t exp_units;  // units per stripe in `expected` (k + p)
  uint8_t *out;
  const uint8_t *expected;
  // verify lanes atomicMin slot * nwin + w into mismatch[s]; pre-filled with INT32_MAX, finished by
  // launch_finish_mismatch, as ozec_reconstruct_crc_batch
  int32_t *mismatch;
  DigestUnit unit[kDigestMaxUnits];
};

hipError_t launch_digest_stripes(int algo, const DigestStripeArgs &a, hipStream_t stream);

}  // namespace ozec
