// gfx950 kernels for per-window SHA-256 / MD5 (ChecksumType SHA256 / MD5, Checksum.java:43-57,76-81).
//
// A Merkle-Damgard digest is serial within a window, so the parallelism is one LANE per (cell, window): unit
// u = c * nwin + w.  Neighbouring lanes read addresses bpc bytes apart -- unlike the CRC kernels, where a wave walks
// one window.  A single very large window is one lane's serial work; nothing here parallelises inside a window.
//
// Fetch, simple form (digest_windows; SHA-256, and MD5 windows under 256 bytes): each lane loads its own next 64-byte
// block (4 x 16 B through an align-1 copy, as the CRC kernels' UA form) before it compresses the current one, into the
// other of two register sets, so no copy sits between a load and its use.  Cooperative form (digest_windows_coop; MD5):
// the wave fetches 256-byte segments of its 64 windows with coalesced loads and hands them to the lanes through LDS.
// Whole blocks lie inside the window; the 0-63 tail bytes are read with 4-byte loads that end at or before the window's
// end and at most three single-byte loads, so nothing outside [cell, cell + len) is touched.
//
// Stripes (digest_stripes, digest_stripes_coop; DigestStripeArgs): the same two forms over the units of coded stripes,
// which lie in two buffers and are computed or verified unit by unit, all in one launch -- a digest launch lasts at
// least one lane's walk over one window, so the stripe paths make one per batch.
#include "device.hpp"
#include "digest.hpp"
#include "digest_core.hpp"

namespace ozec {
namespace {

namespace dg = digest;

// the window's last r = 0..63 bytes at p as 16 words in memory order, zero after them
__device__ __forceinline__ void load_tail(const uint8_t *p, uint32_t r, uint32_t (&t)[16]) {
  const uint32_t wi = r >> 2, nb = r & 3;
  uint32_t part = 0;
#pragma unroll
  for (uint32_t b = 0; b < 3; ++b)
    if (b < nb) part |= static_cast<uint32_t>(p[4 * wi + b]) << (8 * b);
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    uint32_t v = i == wi ? part : 0u;
    if (i < wi) __builtin_memcpy(&v, p + 4 * i, 4);
    t[i] = v;
  }
}

// Blocks [i0, nb) of the window at `win` (N bytes, nb whole blocks) into the state, then the padding: o = the digest's
// words in memory order.  Shared by the cell kernels (digest_rest) and the stripe kernels (digest_stripes*).
template <int A>
__device__ __forceinline__ void digest_blocks(uint32_t *st, const uint8_t *win, int64_t i0, int64_t nb, int64_t N,
                                              uint32_t (&o)[dg::Traits<A>::kStateWords]) {
  // Two register sets: the loads of the next block are issued before the compress of the current one and land in the
  // other set, so no copy sits between a load and its use.  Three things keep hipcc from undoing that (read from the
  // ISA): the loads are unconditional -- past the last whole block the cursor stays on it and the surplus load
  // re-reads it -- because a load under a branch is waited for with vmcnt(0) at every compress; no compress sits
  // under a branch, because the loads of a conditionally used set are sunk down to the use; and a scheduling barrier
  // follows each group of loads, because the scheduler otherwise moves them next to their use to shorten live ranges.
  uint32_t xa[16] = {0}, xb[16];
  const int64_t lastb = nb > 0 ? nb - 1 : 0;
  if (i0 < nb) __builtin_memcpy(xa, win + (i0 << 6), 64);
  int64_t i = i0;
  for (; i + 1 < nb; i += 2) {
    __builtin_memcpy(xb, win + ((i + 1) << 6), 64);
    __builtin_amdgcn_sched_barrier(0);
    dg::compress<A>(st, xa);
    __builtin_memcpy(xa, win + (std::min(i + 2, lastb) << 6), 64);
    __builtin_amdgcn_sched_barrier(0);
    dg::compress<A>(st, xb);
  }
  // What is left goes through one more copy of the block function: the last whole block of an odd count (in xa: the
  // clamped cursor loaded it), then the one or two padded blocks.
  uint32_t t[16], b0[16], b1[16];
  load_tail(win + (nb << 6), static_cast<uint32_t>(N & 63), t);
  const int nfin = dg::final_blocks<A>(static_cast<uint64_t>(N), t, b0, b1);
#pragma unroll 1
  for (int k = i < nb ? 0 : 1; k <= nfin; ++k) {
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = k == 0 ? xa[j] : k == 1 ? b0[j] : b1[j];
    dg::compress<A>(st, m);
  }
  dg::digest_words<A>(st, o);
}

// o differs from the stored digest at e
template <int A>
__device__ __forceinline__ bool digest_differs(const uint32_t (&o)[dg::Traits<A>::kStateWords], const uint8_t *e) {
  constexpr int SW = dg::Traits<A>::kStateWords;
  uint32_t x[SW];
  __builtin_memcpy(x, e, dg::Traits<A>::kDigestLen);
  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < SW; ++j) diff |= x[j] ^ o[j];
  return diff != 0;
}

template <int A>
__device__ __forceinline__ void digest_store(const uint32_t (&o)[dg::Traits<A>::kStateWords], uint8_t *dst) {
#pragma unroll
  for (int j = 0; j < dg::Traits<A>::kStateWords; j += 4) {
    const uint4 v = make_uint4(o[j], o[j + 1], o[j + 2], o[j + 3]);
    __builtin_memcpy(dst + 4 * j, &v, 16);
    store_data_hold(v);
  }
}

// digest_blocks, then the result of unit u = (c, w): the digest stored, or compared with the expected one
template <int A, bool VERIFY>
__device__ __forceinline__ void digest_rest(const DigestArgs &a, uint32_t *st, const uint8_t *win, int64_t i0, int64_t nb,
                                            int64_t N, int64_t u, int64_t c, int64_t w) {
  constexpr int DL = dg::Traits<A>::kDigestLen;
  uint32_t o[dg::Traits<A>::kStateWords];
  digest_blocks<A>(st, win, i0, nb, N, o);
  if constexpr (VERIFY) {
    if (digest_differs<A>(o, a.expected + u * DL)) atomicMin(a.mismatch + c, static_cast<int32_t>(w));
  } else {
    digest_store<A>(o, a.out + u * DL);
  }
}

// Simple form: every lane fetches its own blocks.
template <int A, bool VERIFY>
__global__ __launch_bounds__(kBlock) void digest_windows(const DigestArgs a) {
  const int64_t units = a.ncells * a.nwin;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; u < units;
       u += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t c = u / a.nwin;
    const int64_t w = u - c * a.nwin;
    const int64_t N = w == a.nwin - 1 ? a.len - w * a.bpc : a.bpc;
    const uint8_t *win = a.base + c * a.cell_stride + w * a.bpc;
    uint32_t st[dg::Traits<A>::kStateWords];
    dg::init<A>(st);
    digest_rest<A, VERIFY>(a, st, win, 0, N >> 6, N, u, c, w);
  }
}

// Wave-cooperative form: the wave fetches the next 256 bytes (4 blocks) of each of its 64 windows with 16 coalesced
// loads -- 16 lanes x 16 B cover one window's segment, 4 windows per instruction -- into registers while it works on
// the current step, writes them to its own stage in LDS, and every lane reads its window's row back, one block
// (4 x ds_read_b128) per compress.  Rows are padded by one access width (16 B), so the 16 lanes of a ds_read_b128 group
// (MI355X: rows r, r + 1, ... modulo 16 all distinct within a group) fall on 16 different 16-B slots of the bank row.
// A wave takes as many such steps as its shortest window has whole segments (none if a lane of it has no unit); the
// blocks after them, the tail bytes and the padding go the simple form's way (digest_rest).  The stage is private to
// the wave, whose lanes run in lockstep: no block barrier.
constexpr int kCoopRow = 256 + 16;
constexpr int kCoopWave = 64 * kCoopRow + 64 * 8;  // 64 rows, then the 64 window offsets

// step s of the wave's 64 windows into g, 4 windows per load; unconditional, as in digest_rest (the caller clamps s)
// (the stage holds the windows' offsets from `base`, not their addresses: an address read back from LDS is a generic
// pointer, loaded through flat_load, which counts on the LDS counter too and so is waited for at every ds_read)
__device__ __forceinline__ void coop_fetch(uint4 (&g)[16], const uint8_t *base, const int64_t *offs, int sub, int col,
                                           int s) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
    const u32x4u v = *reinterpret_cast<const u32x4u *>(base + offs[4 * j + sub] + (static_cast<int64_t>(s) << 8) + col);
    g[j] = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

template <int A, bool VERIFY>
__global__ __launch_bounds__(kBlock) void digest_windows_coop(const DigestArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[(kBlock / 64) * kCoopWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t *stage = s_mem + wave * kCoopWave;
  int64_t *offs = reinterpret_cast<int64_t *>(stage + 64 * kCoopRow);
  const int64_t units = a.ncells * a.nwin;
  for (int64_t u0 = (static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave) * 64; u0 < units;
       u0 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t u = u0 + lane;
    const bool live = u < units;
    const int64_t c = live ? u / a.nwin : 0;
    const int64_t w = live ? u - c * a.nwin : 0;
    const int64_t N = !live ? 0 : w == a.nwin - 1 ? a.len - w * a.bpc : a.bpc;
    const int64_t woff = c * a.cell_stride + w * a.bpc;
    const uint8_t *win = a.base + woff;
    const int64_t nb = N >> 6;
    // steps the whole wave takes together: the minimum over its lanes of whole 256-byte segments
    int steps = static_cast<int>(std::min<int64_t>(nb >> 2, 0x7fffffff));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) steps = std::min(steps, __shfl_xor(steps, m, 64));
    steps = __builtin_amdgcn_readfirstlane(steps);
    uint32_t st[dg::Traits<A>::kStateWords];
    dg::init<A>(st);
    if (steps > 0) {
      __builtin_amdgcn_wave_barrier();  // the previous unit's reads of `offs` are done
      offs[lane] = woff;
      __builtin_amdgcn_wave_barrier();
      const int sub = lane >> 4, col = (lane & 15) * 16;
      uint4 g[16];
      coop_fetch(g, a.base, offs, sub, col, 0);
      for (int s = 0; s < steps; ++s) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 16; ++j) *reinterpret_cast<uint4 *>(stage + (4 * j + sub) * kCoopRow + col) = g[j];
        coop_fetch(g, a.base, offs, sub, col, std::min(s + 1, steps - 1));
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int b = 0; b < 4; ++b) {
          uint32_t m[16];
          __builtin_memcpy(m, stage + lane * kCoopRow + b * 64, 64);
          dg::compress<A>(st, m);
        }
      }
    }
    if (live) digest_rest<A, VERIFY>(a, st, win, static_cast<int64_t>(steps) << 2, nb, N, u, c, w);
  }
}

// ---- stripes: cells of two buffers, per-unit roles (DigestStripeArgs) ------------------------------------------------
// The same two fetch forms over lanes (s, j, w) = (s * nunits + j) * nwin + w.  A wave's 64 windows lie in data and
// coded units, several stripes and two allocations, so a window is named by its address, not by an offset from one
// base.  The addresses are kept as integers and turned into pointers of the global address space where they are used:
// that keeps every load a global_load (an address that went through LDS or a select would otherwise be a generic
// pointer and load through flat_load, see coop_fetch).
typedef const __attribute__((address_space(1))) uint8_t *gptr_t;

struct StripeLane {
  int64_t s, w, N;
  uint64_t addr;  // of the window's first byte
  DigestUnit un;
};

__device__ __forceinline__ StripeLane stripe_lane(const DigestStripeArgs &a, int64_t u) {
  StripeLane l;
  const int64_t c = u / a.nwin;
  l.w = u - c * a.nwin;
  l.s = c / a.nunits;
  l.un = a.unit[c - l.s * a.nunits];
  l.N = l.w == a.nwin - 1 ? a.len - l.w * a.bpc : a.bpc;
  const uint64_t b0 = reinterpret_cast<uint64_t>(a.buf[0]), b1 = reinterpret_cast<uint64_t>(a.buf[1]);
  l.addr = (l.un.buf ? b1 : b0) + static_cast<uint64_t>(l.un.off + l.s * (l.un.buf ? a.stripe_stride[1] : a.stripe_stride[0]) +
                                                        l.w * a.bpc);
  return l;
}

// the lane's digest: stored (compute units) or compared (verify units: the smallest slot * nwin + w per stripe)
template <int A>
__device__ __forceinline__ void stripe_result(const DigestStripeArgs &a, const StripeLane &l,
                                              const uint32_t (&o)[dg::Traits<A>::kStateWords]) {
  constexpr int DL = dg::Traits<A>::kDigestLen;
  if (l.un.verify) {
    const int64_t e = (l.s * a.exp_units + l.un.slot) * a.nwin + l.w;
    if (digest_differs<A>(o, a.expected + e * DL))
      atomicMin(a.mismatch + l.s, static_cast<int32_t>(l.un.slot * a.nwin + l.w));
  } else {
    digest_store<A>(o, a.out + ((l.s * a.out_units + l.un.slot) * a.nwin + l.w) * DL);
  }
}

template <int A>
__global__ __launch_bounds__(kBlock) void digest_stripes(const DigestStripeArgs a) {
  const int64_t units = a.nstripes * a.nunits * a.nwin;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; u < units;
       u += static_cast<int64_t>(gridDim.x) * kBlock) {
    const StripeLane l = stripe_lane(a, u);
    const uint8_t *win = (const uint8_t *)reinterpret_cast<gptr_t>(l.addr);
    uint32_t st[dg::Traits<A>::kStateWords], o[dg::Traits<A>::kStateWords];
    dg::init<A>(st);
    digest_blocks<A>(st, win, 0, l.N >> 6, l.N, o);
    stripe_result<A>(a, l, o);
  }
}

// coop_fetch with the stage holding the windows' addresses
__device__ __forceinline__ void coop_fetch_addr(uint4 (&g)[16], const uint64_t *addrs, int sub, int col, int s) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
    typedef const __attribute__((address_space(1))) u32x4u *vptr_t;
    const u32x4u v = *reinterpret_cast<vptr_t>(addrs[4 * j + sub] + (static_cast<uint64_t>(s) << 8) + col);
    g[j] = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

template <int A>
__global__ __launch_bounds__(kBlock) void digest_stripes_coop(const DigestStripeArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[(kBlock / 64) * kCoopWave];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t *stage = s_mem + wave * kCoopWave;
  uint64_t *addrs = reinterpret_cast<uint64_t *>(stage + 64 * kCoopRow);
  const int64_t units = a.nstripes * a.nunits * a.nwin;
  for (int64_t u0 = (static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + wave) * 64; u0 < units;
       u0 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const bool live = u0 + lane < units;
    StripeLane l = stripe_lane(a, live ? u0 + lane : u0);  // a dead lane names a window it never reads: no steps then
    if (!live) l.N = 0;
    const int64_t nb = l.N >> 6;
    int steps = static_cast<int>(std::min<int64_t>(nb >> 2, 0x7fffffff));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) steps = std::min(steps, __shfl_xor(steps, m, 64));
    steps = __builtin_amdgcn_readfirstlane(steps);
    uint32_t st[dg::Traits<A>::kStateWords];
    dg::init<A>(st);
    if (steps > 0) {
      __builtin_amdgcn_wave_barrier();  // the previous unit's reads of `addrs` are done
      addrs[lane] = l.addr;
      __builtin_amdgcn_wave_barrier();
      const int sub = lane >> 4, col = (lane & 15) * 16;
      uint4 g[16];
      coop_fetch_addr(g, addrs, sub, col, 0);
      for (int s = 0; s < steps; ++s) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 16; ++j) *reinterpret_cast<uint4 *>(stage + (4 * j + sub) * kCoopRow + col) = g[j];
        coop_fetch_addr(g, addrs, sub, col, std::min(s + 1, steps - 1));
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int b = 0; b < 4; ++b) {
          uint32_t m[16];
          __builtin_memcpy(m, stage + lane * kCoopRow + b * 64, 64);
          dg::compress<A>(st, m);
        }
      }
    }
    if (live) {
      const uint8_t *win = (const uint8_t *)reinterpret_cast<gptr_t>(l.addr);
      uint32_t o[dg::Traits<A>::kStateWords];
      digest_blocks<A>(st, win, static_cast<int64_t>(steps) << 2, nb, l.N, o);
      stripe_result<A>(a, l, o);
    }
  }
}

// Which form a launch takes, from the A/B on 3,072 cells of 1 MiB (profiles/digest/): MD5, whose bound is the
// fetch path, gains 11-12 % at 16 KiB windows and 36 % at 1 MiB windows from the cooperative form; SHA-256 is bound by
// VALU issue and was 4 % slower with it (two waves per SIMD instead of three), so its cooperative instantiation is not
// built.  Windows under 256 bytes have no whole segment.
template <int A>
constexpr bool kCoop = A == dg::kMd5;

template <int A>
hipError_t launch(const DigestArgs &a, hipStream_t st) {
  const int64_t units = a.ncells * a.nwin;
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>((units + kBlock - 1) / kBlock, int64_t{1} << 22)));
  if constexpr (kCoop<A>) {
    if (a.bpc >= 256) {
      if (a.expected) hipLaunchKernelGGL((digest_windows_coop<A, true>), grid, dim3(kBlock), 0, st, a);
      else hipLaunchKernelGGL((digest_windows_coop<A, false>), grid, dim3(kBlock), 0, st, a);
      return hipGetLastError();
    }
  }
  if (a.expected) hipLaunchKernelGGL((digest_windows<A, true>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((digest_windows<A, false>), grid, dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

template <int A>
hipError_t launch_stripes(const DigestStripeArgs &a, hipStream_t st) {
  const int64_t units = a.nstripes * a.nunits * a.nwin;
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>((units + kBlock - 1) / kBlock, int64_t{1} << 22)));
  if constexpr (kCoop<A>) {
    if (a.bpc >= 256) {
      hipLaunchKernelGGL((digest_stripes_coop<A>), grid, dim3(kBlock), 0, st, a);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((digest_stripes<A>), grid, dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_digest_stripes(int algo, const DigestStripeArgs &a, hipStream_t stream) {
  if (a.nstripes <= 0 || a.nunits <= 0 || a.nwin <= 0) return hipSuccess;
  return algo == dg::kSha256 ? launch_stripes<dg::kSha256>(a, stream) : launch_stripes<dg::kMd5>(a, stream);
}

hipError_t launch_digest_windows(int algo, const DigestArgs &a, hipStream_t stream) {
  if (a.ncells <= 0 || a.nwin <= 0) return hipSuccess;
  return algo == dg::kSha256 ? launch<dg::kSha256>(a, stream) : launch<dg::kMd5>(a, stream);
}

}  // namespace ozec
