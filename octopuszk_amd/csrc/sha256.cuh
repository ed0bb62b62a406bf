// SHA-256 (FIPS 180-4) for one lane: a streaming absorb / finish over a 64-byte block buffer that the caller owns.
// The transcripts of a batch of PLONK proofs are hashed with it, one lane per proof (plonk_verify.cuh, DESIGN.md
// section 38); it compiles for the host too (tests/native/sha256_hostcheck.cpp).  Stands alone.
//
// The eight state words, the sixteen words of the message schedule and the eight working variables live in registers:
// the 64 rounds are unrolled, so that every index of the rolling schedule w[i & 15] is a constant (a runtime-indexed
// W[] would go to scratch).  The block buffer is addressed at run time (the fill level moves with the message), so on
// the device it belongs in LDS: 16 words per lane, the lanes SHA256_LDS_STRIDE = 17 words apart, an odd stride, so
// that the lanes of a wave that touch the same word of their blocks hit distinct banks (points_mul.hip keeps its
// schedules at stride 33 for the same reason).
//
// The buffer holds the block's bytes big-endian in words; below the fill level a word is complete, the word the fill
// level lies in has zero bytes behind it, and the words above are not read before they are written.  Input arrives as
// bytes, as big-endian words at any byte offset (absorb_be32: a shift and at most two words touched), or as the memory
// image of little-endian words (absorb_le_words: the 32-byte elements and compressed points of the transcripts).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if !defined(OZK_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OZK_HD __host__ __device__ __forceinline__
#else
#define OZK_HD inline
#endif
#endif

namespace ozk {

constexpr int SHA256_LDS_STRIDE = 17;   // words between the block buffers of neighbouring lanes in LDS

OZK_HD uint32_t sha256_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
OZK_HD uint32_t sha256_bswap(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

struct Sha256 {
  uint32_t h[8];
  uint32_t* buf;       // 16 words of the caller's
  uint32_t fill;       // bytes of the current block that are in buf: 0 .. 63
  uint32_t blocks;     // blocks compressed so far

  OZK_HD void init(uint32_t* block16) {
    buf = block16;
    fill = 0;
    blocks = 0;
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  }

  OZK_HD void compress() {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = buf[i];
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
      if (i >= 16) {
        const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
        w[i & 15] += (sha256_rotr(x, 7) ^ sha256_rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] +
                     (sha256_rotr(y, 17) ^ sha256_rotr(y, 19) ^ (y >> 10));
      }
      const uint32_t t1 = hh + (sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                          K[i] + w[i & 15];
      const uint32_t t2 = (sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
    h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    blocks++;
    fill = 0;
  }

  OZK_HD void absorb_byte(uint32_t byte) {
    const uint32_t wi = fill >> 2, at = fill & 3;
    if (at == 0) buf[wi] = byte << 24;
    else buf[wi] |= byte << (24 - 8 * at);
    if (++fill == 64) compress();
  }

  // four bytes, the most significant first
  OZK_HD void absorb_be32(uint32_t v) {
    const uint32_t wi = fill >> 2, at = fill & 3;
    if (at == 0) {
      buf[wi] = v;
      fill += 4;
      if (fill == 64) compress();
      return;
    }
    buf[wi] |= v >> (8 * at);
    const uint32_t rest = v << (32 - 8 * at);
    if (wi == 15) {
      compress();
      buf[0] = rest;
      fill = at;
    } else {
      buf[wi + 1] = rest;
      fill += 4;
    }
  }

  // the memory image of n little-endian 32-bit words (4 n bytes in the order they lie in memory)
  OZK_HD void absorb_le_words(const uint32_t* words, int n) {
    for (int i = 0; i < n; i++) absorb_be32(sha256_bswap(words[i]));
  }

  OZK_HD void absorb(const void* ptr, size_t len) {
    const uint8_t* p = (const uint8_t*)ptr;
    for (size_t i = 0; i < len; i++) absorb_byte(p[i]);
  }

  // a digest's 32 bytes, from its eight big-endian words (chained hashes: D1 into gamma's message and so on)
  OZK_HD void absorb_digest(const uint32_t (&d)[8]) {
#pragma unroll 1
    for (int i = 0; i < 8; i++) absorb_be32(d[i]);
  }

  // Padding and the last block or two; digest[i] holds bytes 4 i .. 4 i + 3 of the hash, big-endian.
  OZK_HD void finish(uint32_t (&digest)[8]) {
    const uint64_t bits = ((uint64_t)blocks * 64 + fill) * 8;
    absorb_byte(0x80);
    if (fill > 56) {
      for (uint32_t i = (fill + 3) >> 2; i < 16; i++) buf[i] = 0;
      compress();
    }
    for (uint32_t i = (fill + 3) >> 2; i < 14; i++) buf[i] = 0;
    buf[14] = (uint32_t)(bits >> 32);
    buf[15] = (uint32_t)bits;
    compress();
#pragma unroll
    for (int i = 0; i < 8; i++) digest[i] = h[i];
  }
};

// the digest as 32 bytes
OZK_HD void sha256_digest_bytes(const uint32_t (&d)[8], uint8_t* out32) {
  for (int i = 0; i < 8; i++) {
    out32[4 * i] = (uint8_t)(d[i] >> 24);
    out32[4 * i + 1] = (uint8_t)(d[i] >> 16);
    out32[4 * i + 2] = (uint8_t)(d[i] >> 8);
    out32[4 * i + 3] = (uint8_t)d[i];
  }
}

}  // namespace ozk
