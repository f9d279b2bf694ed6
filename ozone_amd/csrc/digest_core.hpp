// SHA-256 (FIPS 180-4) and MD5 (RFC 1321) block functions and final-block padding, shared by the host and the gfx950
// kernels (digest.hip).  Depends on nothing else in the library and compiles with a plain C++ compiler.
//
// A 64-byte block is passed as 16 uint32 words in MEMORY order: word i holds bytes 4i..4i+3 of the block as a
// little-endian load gives them.  MD5 uses them as they are, SHA-256 swaps each word to big-endian itself.  The digest
// bytes (MessageDigest.digest(), Checksum.java:76-81) are the state words stored big-endian (SHA-256) or little-endian
// (MD5): digest_words.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OZEC_DIGEST_HD __host__ __device__ __forceinline__
#else
#define OZEC_DIGEST_HD inline
#endif
#if defined(__clang__)
#define OZEC_DIGEST_UNROLL _Pragma("unroll")
#else
#define OZEC_DIGEST_UNROLL
#endif

namespace ozec {
namespace digest {

enum Algo { kSha256 = 0, kMd5 = 1 };

template <int A>
struct Traits;
template <>
struct Traits<kSha256> {
  static constexpr int kStateWords = 8;
  static constexpr int kDigestLen = 32;
};
template <>
struct Traits<kMd5> {
  static constexpr int kStateWords = 4;
  static constexpr int kDigestLen = 16;
};

// ---- bit primitives: on gfx950 v_alignbit_b32 / v_bitop3_b32 / v_perm_b32 through the builtins, plain C++ elsewhere
OZEC_DIGEST_HD uint32_t rotr(uint32_t x, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, n);
#else
  return (x >> n) | (x << (32 - n));
#endif
}
OZEC_DIGEST_HD uint32_t rotl(uint32_t x, int n) { return rotr(x, 32 - n); }
OZEC_DIGEST_HD uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// three-input bit function with truth table T, bit (4a + 2b + c) of T the result for input bits a, b, c
// (a = 0xF0, b = 0xCC, c = 0xAA): 0x96 a ^ b ^ c, 0xCA a ? b : c, 0xE8 majority, 0xE4 c ? a : b, 0x39 b ^ (a | ~c)
template <int T>
OZEC_DIGEST_HD uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
  return __builtin_amdgcn_bitop3_b32(a, b, c, T);
#else
  uint32_t r = 0;
  if (T & 0x01) r |= ~a & ~b & ~c;
  if (T & 0x02) r |= ~a & ~b & c;
  if (T & 0x04) r |= ~a & b & ~c;
  if (T & 0x08) r |= ~a & b & c;
  if (T & 0x10) r |= a & ~b & ~c;
  if (T & 0x20) r |= a & ~b & c;
  if (T & 0x40) r |= a & b & ~c;
  if (T & 0x80) r |= a & b & c;
  return r;
#endif
}
OZEC_DIGEST_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return bitop3<0x96>(a, b, c); }

// ---- SHA-256 ---------------------------------------------------------------------------------------------------
constexpr uint32_t kSha256K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

OZEC_DIGEST_HD void sha256_init(uint32_t s[8]) {
  s[0] = 0x6a09e667u, s[1] = 0xbb67ae85u, s[2] = 0x3c6ef372u, s[3] = 0xa54ff53au;
  s[4] = 0x510e527fu, s[5] = 0x9b05688cu, s[6] = 0x1f83d9abu, s[7] = 0x5be0cd19u;
}

// one block into the state: 64 rounds fully unrolled over a ring of 16 schedule words
OZEC_DIGEST_HD void sha256_compress(uint32_t s[8], const uint32_t m[16]) {
  uint32_t w[16];
OZEC_DIGEST_UNROLL
  for (int i = 0; i < 16; ++i) w[i] = bswap(m[i]);
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
OZEC_DIGEST_UNROLL
  for (int i = 0; i < 64; ++i) {
    if (i >= 16) {
      const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      w[i & 15] += xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3) + w[(i - 7) & 15] +
                   xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
    }
    const uint32_t t1 = h + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + bitop3<0xCA>(e, f, g) + kSha256K[i] + w[i & 15];
    const uint32_t t2 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + bitop3<0xE8>(a, b, c);
    h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
  }
  s[0] += a, s[1] += b, s[2] += c, s[3] += d, s[4] += e, s[5] += f, s[6] += g, s[7] += h;
}

// ---- MD5 -------------------------------------------------------------------------------------------------------
constexpr uint32_t kMd5K[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af,
    0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa,
    0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8,
    0x676f02d9, 0x8d2a4c8a, 0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
    0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97,
    0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1,
    0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
constexpr int kMd5S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};

OZEC_DIGEST_HD void md5_init(uint32_t s[4]) {
  s[0] = 0x67452301u, s[1] = 0xefcdab89u, s[2] = 0x98badcfeu, s[3] = 0x10325476u;
}

OZEC_DIGEST_HD void md5_compress(uint32_t s[4], const uint32_t m[16]) {
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
OZEC_DIGEST_UNROLL
  for (int i = 0; i < 64; ++i) {
    uint32_t f;
    int g;
    if (i < 16) {
      f = bitop3<0xCA>(b, c, d), g = i;  // F = (b & c) | (~b & d)
    } else if (i < 32) {
      f = bitop3<0xE4>(b, c, d), g = (5 * i + 1) & 15;  // G = (b & d) | (c & ~d)
    } else if (i < 48) {
      f = xor3(b, c, d), g = (3 * i + 5) & 15;  // H
    } else {
      f = bitop3<0x39>(b, c, d), g = (7 * i) & 15;  // I = c ^ (b | ~d)
    }
    const uint32_t t = a + f + kMd5K[i] + m[g];
    a = d, d = c, c = b, b = b + rotl(t, kMd5S[i >> 4][i & 3]);
  }
  s[0] += a, s[1] += b, s[2] += c, s[3] += d;
}

// ---- algorithm-generic front ---------------------------------------------------------------------------------------
template <int A>
OZEC_DIGEST_HD void init(uint32_t *s) {
  if (A == kSha256)
    sha256_init(s);
  else
    md5_init(s);
}
template <int A>
OZEC_DIGEST_HD void compress(uint32_t *s, const uint32_t m[16]) {
  if (A == kSha256)
    sha256_compress(s, m);
  else
    md5_compress(s, m);
}

// The padded end of a message of total_len bytes (a 64-bit count): `tail` holds its last total_len % 64 bytes in memory
// order with every byte after them zero.  Appends 0x80, zeros and the bit length -- big-endian for SHA-256, little-endian
// for MD5 -- and returns the number of blocks produced: 1 (b0; tails up to 55 bytes) or 2 (b0, b1).
template <int A>
OZEC_DIGEST_HD int final_blocks(uint64_t total_len, const uint32_t tail[16], uint32_t b0[16], uint32_t b1[16]) {
  const uint32_t r = static_cast<uint32_t>(total_len & 63);
  const uint32_t mark = 0x80u << (8 * (r & 3));
OZEC_DIGEST_UNROLL
  for (int i = 0; i < 16; ++i) {
    b0[i] = tail[i] | (static_cast<uint32_t>(i) == (r >> 2) ? mark : 0u);
    b1[i] = 0;
  }
  const uint64_t bits = total_len << 3;
  const uint32_t lo = static_cast<uint32_t>(bits), hi = static_cast<uint32_t>(bits >> 32);
  const uint32_t w14 = A == kSha256 ? bswap(hi) : lo, w15 = A == kSha256 ? bswap(lo) : hi;
  if (r < 56) {
    b0[14] = w14, b0[15] = w15;
    return 1;
  }
  b1[14] = w14, b1[15] = w15;
  return 2;
}

// state -> digest bytes as 32-bit words in memory order
template <int A>
OZEC_DIGEST_HD void digest_words(const uint32_t *s, uint32_t *out) {
OZEC_DIGEST_UNROLL
  for (int i = 0; i < Traits<A>::kStateWords; ++i) out[i] = A == kSha256 ? bswap(s[i]) : s[i];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// whole message on the host (little-endian hosts: the words are loaded with memcpy): out gets Traits<A>::kDigestLen bytes
template <int A>
inline void digest_bytes(const uint8_t *data, uint64_t len, uint8_t *out) {
  uint32_t s[8], m[16], b0[16], b1[16], o[8];
  init<A>(s);
  uint64_t off = 0;
  for (; off + 64 <= len; off += 64) {
    memcpy(m, data + off, 64);
    compress<A>(s, m);
  }
  memset(m, 0, sizeof m);
  if (len > off) memcpy(m, data + off, static_cast<size_t>(len - off));
  const int n = final_blocks<A>(len, m, b0, b1);
  compress<A>(s, b0);
  if (n == 2) compress<A>(s, b1);
  digest_words<A>(s, o);
  memcpy(out, o, Traits<A>::kDigestLen);
}
#endif

}  // namespace digest
}  // namespace ozec
