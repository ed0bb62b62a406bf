// GLV endomorphism for BN254 (j = 0): phi(x, y) = (beta x, y) = lambda * (x, y) on the order-r
// subgroups of G1 (beta = BETA_G1) and of the twist G2 (beta = BETA_G2 = BETA_G1^2, same lambda).
// A scalar k (reduced mod r) splits as k = k1 + k2 * lambda (mod r) with |k1|, |k2| < 2^127, so
//     sum k_i P_i = sum |k1_i| (+-P_i) + sum |k2_i| (+-phi(P_i)):
// twice the points, half the scalar length — the same number of bucket additions, but HALF the
// windows: half the bucket-to-window-sum work and a Horner chain of 112 instead of 240 dependent
// doublings (the serial tail that dominates a single MSM's latency).
// Decomposition (lattice basis from the extended Euclid on (r, lambda); constants generated and
// cross-checked by tools/gen_glv.py; model and bound test in tests/test_glv.py):
//     c1 = floor(k * G1C / 2^256),  c2 = floor(k * G2C / 2^256)      (G1C ~ 2^256 b2 / r, G2C ~ 2^256 |b1| / r)
//     k1 = k - c1 * A1 - c2 * A2,   k2 = c1 * B1ABS - c2 * B2
// The reference has no counterpart (its windows cover all 254 bits, VariableBaseMSM.java:137-143);
// the group element computed is the same.
#pragma once
#include "curve.cuh"

namespace ozk {

struct GlvConsts {
  static constexpr u32 R32[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};      // r
  static constexpr u32 G1C[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u};
  static constexpr u32 G2C[5] = {0x391eb18du, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u};
  static constexpr u32 A1[2] = {0x94d213e3u, 0x89d32568u};
  static constexpr u32 A2[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};
  static constexpr u32 B1ABS[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};
  static constexpr u32 B2[2] = {0x94d213e3u, 0x89d32568u};
  // beta in Montgomery form (R = 2^261), 9 x 29-bit limbs
  static constexpr u32 BETA_G1[9] = {0xa337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu, 0x176f16du, 0xeed93bau, 0x14291140u, 0xc0afeu};
  static constexpr u32 BETA_G2[9] = {0x18ccb791u, 0x175b1c3au, 0xb83d6e2u, 0xe8ed071u, 0x1282bee2u, 0x4220e84u, 0x1fe4017fu, 0x15084d4au, 0x169119u};
};

// r[0..NR) = low NR words of a[0..NA) * b[0..NB), row by row (one row per word of b) on a 64-bit multiply-add:
//     t = a[i] * b[j] + r[i + j] + carry  <=  (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
// never overflows, so a row needs no third carry word; the low word of t is the new r[i + j], the high word the
// carry into the next position.  Terms at positions >= NR are not computed.
template <int NA, int NB, int NR>
OZK_HD void mp_mul_lo(const u32* a, const u32* b, u32* r) {
#pragma unroll
  for (int k = 0; k < NR; k++) r[k] = 0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    u32 carry = 0;
#pragma unroll
    for (int i = 0; i < NA; i++) {
      if (i + j < NR) {
        const u64 t = mad64(a[i], b[j], (u64)r[i + j] + carry);
        r[i + j] = (u32)t;
        carry = (u32)(t >> 32);
      }
    }
    if (NA + j < NR) r[NA + j] = carry;   // (no earlier row reaches this word)
  }
}

template <int N>
OZK_HD void mp_sub(u32* a, const u32* b) {  // a -= b (mod 2^(32N))
  u64 br = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const u64 t = (u64)a[i] - b[i] - br;
    a[i] = (u32)t;
    br = (t >> 32) & 1;
  }
}
template <int N>
OZK_HD bool mp_geq(const u32* a, const u32* b) {
  for (int i = N - 1; i >= 0; i--) {
    if (a[i] > b[i]) return true;
    if (a[i] < b[i]) return false;
  }
  return true;
}
template <int N>
OZK_HD void mp_cneg(u32* a, bool neg) {  // two's complement negate when neg, by selects: a = (a ^ m) + (m & 1), m = -neg
  const u32 m = 0u - (u32)neg;
  u64 c = m & 1u;
#pragma unroll
  for (int i = 0; i < N; i++) {
    c += (u64)(a[i] ^ m);
    a[i] = (u32)c;
    c >>= 32;
  }
}

// k <- k mod r for ANY 256-bit k, without a branch.  With k7, r7 the top words, q' = floor(k7 / (r7 + 1)) is
// floor(k / r) or one less: k >= k7 2^224 and r < (r7 + 1) 2^224 give q' <= k / r, and k / r < (k7 + 1) / r7 <=
// (q' + 1)(1 + 1 / r7) < q' + 2 because q' + 1 <= 6 < r7.  So k - q' r is in [0, 2r): one conditional subtraction.
OZK_HD void reduce_mod_r(u32 (&k)[8]) {
  const u32 q = k[7] / (GlvConsts::R32[7] + 1u);   // 0 .. 5 (a division by a constant: multiply-high and shift)
  u64 m = 0;
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {   // k -= q r
    m = mad64(q, GlvConsts::R32[i], m);
    const u64 t = (u64)k[i] - (u32)m - br;
    k[i] = (u32)t;
    br = (u32)(t >> 32) & 1u;
    m >>= 32;
  }
  u32 d[8];
  br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {   // d = k - r
    const u64 t = (u64)k[i] - GlvConsts::R32[i] - br;
    d[i] = (u32)t;
    br = (u32)(t >> 32) & 1u;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = br ? k[i] : d[i];
}

// k: any 256-bit value (reduced mod r first).  Outputs |k1|, |k2| as 4 words each (< 2^128) + signs.
// Sizes: c1 <= k G1C / 2^256 < r G1C / 2^256 <= B2 < 2^64 and c2 < |B1| < 2^127, so c1 has 2 words and c2 has 4
// (words 8-9 and 8-11 of the two products, carries out of the low words included; the words above are zero).
// k1 and k2 are below 2^127 in magnitude (tests/test_glv.py), so they are computed modulo 2^128 in two's complement:
// bit 127 is the sign, and no product word at or above 2^128 is formed.
OZK_HD void glv_decompose(const u32 (&k_in)[8], u32 (&k1)[4], bool& neg1, u32 (&k2)[4], bool& neg2) {
  u32 k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_in[i];
  reduce_mod_r(k);
  u32 p1[10], p2[12];
  mp_mul_lo<8, 3, 10>(k, GlvConsts::G1C, p1);
  mp_mul_lo<8, 5, 12>(k, GlvConsts::G2C, p2);
  const u32* c1 = p1 + 8;  // 2 words
  const u32* c2 = p2 + 8;  // 4 words
  u32 t1[4], t2[4], s1[4], s2[4];
  mp_mul_lo<2, 2, 4>(c1, GlvConsts::A1, t1);
  mp_mul_lo<4, 4, 4>(c2, GlvConsts::A2, t2);
#pragma unroll
  for (int i = 0; i < 4; i++) s1[i] = k[i];
  mp_sub<4>(s1, t1);
  mp_sub<4>(s1, t2);                                  // k1 = k - c1 a1 - c2 a2
  mp_mul_lo<2, 4, 4>(c1, GlvConsts::B1ABS, s2);
  mp_mul_lo<4, 2, 4>(c2, GlvConsts::B2, t2);
  mp_sub<4>(s2, t2);                                  // k2 = c1 |b1| - c2 b2
  neg1 = (s1[3] >> 31) != 0;
  neg2 = (s2[3] >> 31) != 0;
  mp_cneg<4>(s1, neg1);
  mp_cneg<4>(s2, neg2);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    k1[i] = s1[i];
    k2[i] = s2[i];
  }
}

// beta of the GLV endomorphism for this curve's base field (G2: beta^2, acting on both Fq2 components)
template <class CV>
OZK_HD Fe<FqParams, 16> glv_beta() {
  if constexpr (CurveIO<CV>::CW == 16) return fe_const<FqParams, 16>(GlvConsts::BETA_G2);
  else return fe_const<FqParams, 16>(GlvConsts::BETA_G1);
}
// phi(q) = (beta x, y) of an affine point with canonical coordinates, canonical again; O = (0, 0) stays O
template <class CV>
OZK_HD Aff<typename CV::EA> glv_image(const Aff<typename CV::EA>& q) {
  Aff<typename CV::EA> q2;
  q2.x = typename CV::EA(canonical(scale(q.x, glv_beta<CV>())));
  q2.y = q.y;
  return q2;
}

}  // namespace ozk
