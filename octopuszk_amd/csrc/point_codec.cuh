// Compressed BN254 points: an x coordinate plus a sign bit, 32 bytes for G1 and 64 for G2, and the
// square roots in Fq and Fq2 that turn them back into points.  One point per lane, registers only.
//
//   G1  x little-endian (x < q < 2^254); bit 7 of byte 31 Y_LARGER (canonical y > q - y), bit 6 INFINITY
//   G2  x.c0 | x.c1, each as above; the two flags in byte 63; Y_LARGER decided on y.c1 unless it is 0, then on y.c0
//
// Decoding is strict and returns a code per point: 0 ok, 1 a coordinate >= q, 2 bad infinity encoding (or Y_LARGER on
// a point with y = 0), 3 no curve point has this x.  Proofs get no subgroup check here: [r]B = O stays in
// bv_g2_wellformed (batch_verify.cuh).  The points of a proving key are decoded straight into the
// prepared records of the variable-base MSM (codec_g1_decode_prepared / codec_g2_decode_prepared: what
// k_convert_bases of msm_var.cuh makes of the decoded wire point, without the wire point), and those of G2 can be
// checked for [r]P = O there: code 4.
//
// Bounds: every element that crosses a function boundary is a CdFq / CdF2 (< 2p); whatever is compared or stored is
// first made canonical, as integer words out of from_mont.  The header compiles for the host too
// (tests/native/codec_hostcheck.cpp), the kernels at the end only in point_codec.hip.
#pragma once
#include "fq2.cuh"
#include "glv.cuh"
#include "pairing_consts_gen.h"

namespace ozk {

using CdFq = Fe<FqParams, 32>;
using CdF2 = Fe2<32>;

constexpr int CODEC_OK = 0, CODEC_E_RANGE = 1, CODEC_E_INFINITY = 2, CODEC_E_NO_POINT = 3;
constexpr int CODEC_E_SUBGROUP = 4;   // only from the subgroup check of decoded key points (k_codec_subgroup_g2)
constexpr u32 CODEC_Y_LARGER = 0x80000000u, CODEC_INFINITY = 0x40000000u;   // in the top word of the encoding

constexpr u32 CODEC_Q_WORDS[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                                  0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
// (q + 1) / 4, 252 bits: 63 windows of 4
constexpr u32 CODEC_SQRT_EXP[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                                   0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
constexpr int CODEC_SQRT_WINDOWS = 63;
// 1 / 2 and 3 in Montgomery form
constexpr u32 CODEC_HALF[9] = {0x16fce4b4u, 0xa904407u,  0xa626a11u, 0x12109375u, 0x1014a498u,
                               0x100ec0c7u, 0x93e16a4u,  0x9c376eeu, 0x1f1642u};
constexpr u32 CODEC_THREE[9] = {0x766463u,   0x1c54760au, 0x8f6927au,  0x3e40c4du, 0x1fea4f2bu,
                                0x17c6c26au, 0x157fe417u, 0xf8056f9u,  0x2958a2u};

// ---------------------------------------------------------------------------------------------- square roots
// q = 3 (mod 4): the only candidate for a root of a is a^((q+1)/4), whose square is a or -a.  Fixed 4-bit windows
// over the constant exponent: 14 products for the table a^2 .. a^15, then 4 squarings and one product per window
// (252 + 77 against the 251 + 108 of square-and-multiply).  The table entry is picked with selects on the window
// digit, which is the same in every lane: no branch on data, no indexed register array.
OZK_HD bool fq_sqrt(const CdFq& a, CdFq& root) {
  CdFq t[16];
  t[0] = CdFq(fe_one<FqParams>());
  t[1] = a;
#pragma unroll
  for (int j = 2; j < 16; j++) t[j] = CdFq(mul(t[j - 1], a));
  CdFq r = t[0];
#pragma unroll 1
  for (int w = CODEC_SQRT_WINDOWS - 1; w >= 0; w--) {
#pragma unroll
    for (int s = 0; s < 4; s++) r = CdFq(sqr(r));
    const u32 d = (CODEC_SQRT_EXP[w >> 3] >> (4 * (w & 7))) & 15u;
    CdFq m = t[0];
#pragma unroll
    for (int j = 1; j < 16; j++) m = select_el(d == (u32)j, t[j], m);
    r = CdFq(mul(r, m));
  }
  root = r;
  return is_zero(sub(CdFq(sqr(r)), a));
}

OZK_HD bool codec_words_zero(const u32 (&w)[8]) {
  u32 o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= w[i];
  return o == 0;
}
// w < q
OZK_HD bool codec_canonical(const u32 (&w)[8]) {
  bool lt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    lt = decided ? lt : w[i] < CODEC_Q_WORDS[i];
    decided = decided || w[i] != CODEC_Q_WORDS[i];
  }
  return lt;
}
// y > q - y for a canonical y, i.e. 2 y > q
OZK_HD bool larger(const u32 (&y)[8]) {
  bool gt = false, decided = false;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    const u32 d = (y[i] << 1) | (i ? y[i - 1] >> 31 : 0u);
    gt = decided ? gt : d > CODEC_Q_WORDS[i];
    decided = decided || d != CODEC_Q_WORDS[i];
  }
  return gt;   // y < q < 2^254: bit 256 of 2 y is clear
}
// q - y for a canonical y != 0
OZK_HD void codec_negate(u32 (&y)[8]) {
  u32 borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u64 d = (u64)CODEC_Q_WORDS[i] - y[i] - borrow;
    y[i] = (u32)d;
    borrow = (u32)(d >> 63);
  }
}
// the order of Y_LARGER on Fq2: c1 decides unless it is zero
OZK_HD bool larger2(const u32 (&y0)[8], const u32 (&y1)[8]) { return codec_words_zero(y1) ? larger(y0) : larger(y1); }

// A root of a in Fq2 = Fq[u] / (u^2 + 1), by the norm ("complex") method with two Fq roots and one inversion.
// a = a0 + a1 u is a square exactly when n = a0^2 + a1^2 is one in Fq.  With alpha^2 = n and
// delta = (a0 + alpha) / 2, the candidate c = delta^((q+1)/4) squares to delta or to -delta:
//   c^2 =  delta:  root = c + t u,  t = a1 / (2 c)      (c^2 - t^2 = delta - (alpha - a0) / 2 = a0)
//   c^2 = -delta:  root = t + c u                        (t^2 - c^2 = (a0 - alpha) / 2 + delta = a0)
// so the second candidate never has to be recomputed for the other sign of alpha.  a1 = 0 takes delta = a0
// (alpha = +-a0 would make delta 0 or a0 by chance): root c for a square a0, else c u, purely imaginary.  a1 != 0
// gives delta != 0, so the inversion is of a non-zero value; a = 0 gives c = t = 0.
// Of the two roots the one that is not `larger2` is returned, so that the result is a function of a alone.
OZK_HD bool fq2_sqrt(const CdF2& a, CdF2& root) {
  const bool real = is_zero(a.c1);
  const CdFq n = CdFq(reduce_to<32>(add(sqr(a.c0), sqr(a.c1))));
  CdFq alpha;
  const bool square = fq_sqrt(n, alpha);
  const CdFq half = CdFq(fe_const<FqParams, 16>(CODEC_HALF));
  const CdFq delta = select_el(real, a.c0, CdFq(mul(add(a.c0, alpha), half)));
  CdFq c;
  const bool direct = fq_sqrt(delta, c);
  const CdFq t = CdFq(mul(a.c1, inv(dbl(c))));
  const CdFq r0 = select_el(direct, c, t), r1 = select_el(direct, t, c);
  u32 w0[8], w1[8];
  from_mont(r0, w0);
  from_mont(r1, w1);
  const bool flip = larger2(w0, w1);
  root.c0 = select_el(flip, CdFq(reduce_to<32>(neg(r0))), r0);
  root.c1 = select_el(flip, CdFq(reduce_to<32>(neg(r1))), r1);
  return square;
}

// ---------------------------------------------------------------------------------------------- points
// A decoded point: affine, canonical integer words; inf: the point O (also what a failed decoding leaves)
struct CodecG1 {
  u32 x[8], y[8];
  bool inf;
};
struct CodecG2 {
  u32 x[2][8], y[2][8];
  bool inf;
};

OZK_HD CdFq codec_fq(const u32 (&w)[8]) { return CdFq(to_mont<FqParams>(w)); }

// the code of an encoding from what was found: infinity flag (0 or 2), x >= q (1), no root (3), y = 0 with Y_LARGER (2)
OZK_HD int codec_code(bool infinity, bool ylarger, bool x_zero, bool x_canonical, bool on, bool y_zero) {
  if (infinity) return (!x_zero || ylarger) ? CODEC_E_INFINITY : CODEC_OK;
  if (!x_canonical) return CODEC_E_RANGE;
  if (!on) return CODEC_E_NO_POINT;
  return (y_zero && ylarger) ? CODEC_E_INFINITY : CODEC_OK;
}

// in: 8 words.  The checks in the order of the codes' precedence: infinity flag (0 or 2), x >= q (1), x^3 + 3 not
// a square (3), y = 0 with Y_LARGER (2).
OZK_HD int codec_g1_decode(const u32* in, CodecG1& p) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = in[i];
  const bool ylarger = (w[7] & CODEC_Y_LARGER) != 0, infinity = (w[7] & CODEC_INFINITY) != 0;
  w[7] &= ~(CODEC_Y_LARGER | CODEC_INFINITY);
  const CdFq X = codec_fq(w);
  const CdFq rhs = CdFq(reduce_to<32>(add(mul(CdFq(sqr(X)), X), fe_const<FqParams, 16>(CODEC_THREE))));
  CdFq Y;
  const bool on = fq_sqrt(rhs, Y);
  from_mont(Y, p.y);
  const bool y0 = codec_words_zero(p.y);
  if (larger(p.y) != ylarger) codec_negate(p.y);
  const int code = codec_code(infinity, ylarger, codec_words_zero(w), codec_canonical(w), on, y0);
#pragma unroll
  for (int i = 0; i < 8; i++) p.x[i] = w[i];
  p.inf = infinity || code != CODEC_OK;
  return code;
}

// in: 16 words, x.c0 | x.c1, flags in the top word of x.c1.  Same order of checks; the curve is the twist
// y^2 = x^3 + 3 / (9 + u).
OZK_HD int codec_g2_decode(const u32* in, CodecG2& p) {
  u32 w0[8], w1[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    w0[i] = in[i];
    w1[i] = in[8 + i];
  }
  const bool ylarger = (w1[7] & CODEC_Y_LARGER) != 0, infinity = (w1[7] & CODEC_INFINITY) != 0;
  w1[7] &= ~(CODEC_Y_LARGER | CODEC_INFINITY);
  CdF2 X, b;
  X.c0 = codec_fq(w0);
  X.c1 = codec_fq(w1);
  b.c0 = CdFq(fe_const<FqParams, 16>(pc::TWIST_B[0]));
  b.c1 = CdFq(fe_const<FqParams, 16>(pc::TWIST_B[1]));
  const CdF2 rhs = reduce_to<32>(add(mul(sqr(X), X), b));
  CdF2 Y;
  const bool on = fq2_sqrt(rhs, Y);   // the root that is not larger2
  from_mont(Y.c0, p.y[0]);
  from_mont(Y.c1, p.y[1]);
  const bool y0 = codec_words_zero(p.y[0]) && codec_words_zero(p.y[1]);
  if (ylarger) {
    if (!codec_words_zero(p.y[0])) codec_negate(p.y[0]);
    if (!codec_words_zero(p.y[1])) codec_negate(p.y[1]);
  }
  const int code = codec_code(infinity, ylarger, codec_words_zero(w0) && codec_words_zero(w1),
                              codec_canonical(w0) && codec_canonical(w1), on, y0);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p.x[0][i] = w0[i];
    p.x[1][i] = w1[i];
  }
  p.inf = infinity || code != CODEC_OK;
  return code;
}

// ---------------------------------------------------------------------------------------------- prepared records
// A compressed point straight into the two records k_convert_bases (msm_var.cuh) makes of the decoded point: q = (x, y),
// q2 = (beta x, y), canonical Montgomery; O and every point whose code is not 0 become the (0, 0) marker in both.
// x enters Montgomery form once and stays; y stays there from the square root on.  The only canonical integer taken
// is the one Y_LARGER is decided on (G2: inside fq2_sqrt), and the root is negated in the Montgomery domain.
OZK_HD int codec_g1_decode_prepared(const u32* in, Aff<G1Cfg::EA>& q, Aff<G1Cfg::EA>& q2) {
  using EA = G1Cfg::EA;
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = in[i];
  const bool ylarger = (w[7] & CODEC_Y_LARGER) != 0, infinity = (w[7] & CODEC_INFINITY) != 0;
  w[7] &= ~(CODEC_Y_LARGER | CODEC_INFINITY);
  const CdFq X = codec_fq(w);
  const CdFq rhs = CdFq(reduce_to<32>(add(mul(CdFq(sqr(X)), X), fe_const<FqParams, 16>(CODEC_THREE))));
  CdFq Y;
  const bool on = fq_sqrt(rhs, Y);
  u32 yw[8];
  from_mont(Y, yw);
  const int code = codec_code(infinity, ylarger, codec_words_zero(w), codec_canonical(w), on, codec_words_zero(yw));
  const bool inf = infinity || code != CODEC_OK;
  const Fe<FqParams, 16> zero = fe_zero<FqParams>();
  const Fe<FqParams, 16> y = select_el(larger(yw) != ylarger, canonical(neg(Y)), canonical(Y));   // -0 = 0
  q.x = EA(select_el(inf, zero, canonical(X)));
  q.y = EA(select_el(inf, zero, y));
  q2 = glv_image<G1Cfg>(q);
  return code;
}

OZK_HD int codec_g2_decode_prepared(const u32* in, Aff<G2Cfg::EA>& q, Aff<G2Cfg::EA>& q2) {
  using EA = G2Cfg::EA;
  u32 w0[8], w1[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    w0[i] = in[i];
    w1[i] = in[8 + i];
  }
  const bool ylarger = (w1[7] & CODEC_Y_LARGER) != 0, infinity = (w1[7] & CODEC_INFINITY) != 0;
  w1[7] &= ~(CODEC_Y_LARGER | CODEC_INFINITY);
  CdF2 X, b;
  X.c0 = codec_fq(w0);
  X.c1 = codec_fq(w1);
  b.c0 = CdFq(fe_const<FqParams, 16>(pc::TWIST_B[0]));
  b.c1 = CdFq(fe_const<FqParams, 16>(pc::TWIST_B[1]));
  const CdF2 rhs = reduce_to<32>(add(mul(sqr(X), X), b));
  CdF2 Y;
  const bool on = fq2_sqrt(rhs, Y);   // the root that is not larger2
  const int code = codec_code(infinity, ylarger, codec_words_zero(w0) && codec_words_zero(w1),
                              codec_canonical(w0) && codec_canonical(w1), on, is_zero(Y));
  const bool inf = infinity || code != CODEC_OK;
  const Fe2<16> zero = el_zero(Y);
  const Fe2<16> y = select_el(ylarger, canonical(neg(Y)), canonical(Y));
  q.x = EA(select_el(inf, zero, canonical(X)));
  q.y = EA(select_el(inf, zero, y));
  q2 = glv_image<G2Cfg>(q);
  return code;
}

// one canonical value as a wire coordinate of S words (8: wire-in, 16: wire-out with the upper half zero);
// `keep` false writes `other` (0 or 1) instead
OZK_HD void codec_store_coord(const u32 (&w)[8], bool keep, u32 other, int S, u32* out) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = keep ? w[i] : (i == 0 ? other : 0u);
  for (int i = 8; i < S; i++) out[i] = 0;
}
// X | Y | Z with Z = 1; O is (0, 1, 0), the affine form of infinity everywhere else in the library
OZK_HD void codec_g1_store(const CodecG1& p, int S, u32* out) {
  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  codec_store_coord(p.x, !p.inf, 0, S, out);
  codec_store_coord(p.y, !p.inf, 1, S, out + S);
  codec_store_coord(zero, false, p.inf ? 0u : 1u, S, out + 2 * S);
}
// X.c0 | X.c1 | Y.c0 | Y.c1 | Z.c0 | Z.c1; O is ((0, 0), (1, 0), (0, 0))
OZK_HD void codec_g2_store(const CodecG2& p, int S, u32* out) {
  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  codec_store_coord(p.x[0], !p.inf, 0, S, out);
  codec_store_coord(p.x[1], !p.inf, 0, S, out + S);
  codec_store_coord(p.y[0], !p.inf, 1, S, out + 2 * S);
  codec_store_coord(p.y[1], !p.inf, 0, S, out + 3 * S);
  codec_store_coord(zero, false, p.inf ? 0u : 1u, S, out + 4 * S);
  codec_store_coord(zero, false, 0, S, out + 5 * S);
}

OZK_HD CdFq codec_load_coord(const u32* p) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = p[i];
  return codec_fq(w);   // any 256-bit value, taken mod q
}

// p: X | Y | Z, S words per coordinate, any Z (Jacobian); out: 8 words.  Z = 0 gives the infinity encoding;
// inv(0) = 0 makes x and y zero there, so nothing branches.
OZK_HD void codec_g1_encode(const u32* p, int S, u32* out) {
  const CdFq X = codec_load_coord(p), Y = codec_load_coord(p + S), Z = codec_load_coord(p + 2 * S);
  const bool inf = is_zero(Z);
  const CdFq zi = inv(Z), zi2 = CdFq(sqr(zi));
  u32 x[8], y[8];
  from_mont(CdFq(mul(X, zi2)), x);
  from_mont(CdFq(mul(Y, CdFq(mul(zi2, zi)))), y);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = x[i];
  out[7] |= inf ? CODEC_INFINITY : (larger(y) ? CODEC_Y_LARGER : 0u);
}
// p: X.c0 | X.c1 | Y.c0 | Y.c1 | Z.c0 | Z.c1; out: 16 words
OZK_HD void codec_g2_encode(const u32* p, int S, u32* out) {
  CdF2 X, Y, Z;
  X.c0 = codec_load_coord(p);
  X.c1 = codec_load_coord(p + S);
  Y.c0 = codec_load_coord(p + 2 * S);
  Y.c1 = codec_load_coord(p + 3 * S);
  Z.c0 = codec_load_coord(p + 4 * S);
  Z.c1 = codec_load_coord(p + 5 * S);
  const bool inf = is_zero(Z);
  const CdF2 zi = inv(Z), zi2 = sqr(zi);
  const CdF2 x = mul(X, zi2), y = mul(Y, mul(zi2, zi));
  u32 x0[8], x1[8], y0[8], y1[8];
  from_mont(x.c0, x0);
  from_mont(x.c1, x1);
  from_mont(y.c0, y0);
  from_mont(y.c1, y1);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[i] = x0[i];
    out[8 + i] = x1[i];
  }
  out[15] |= inf ? CODEC_INFINITY : (larger2(y0, y1) ? CODEC_Y_LARGER : 0u);
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- kernels
// One point per lane, one wave per workgroup.  G1 and G2 work never share a wave: the typed kernels are
// instantiated per group, and the proof kernel gives the two groups separate ranges of the grid.

template <int TYPE>   // 1: G1, 2: G2
__global__ __launch_bounds__(64) void k_codec_decompress(const u32* __restrict__ in, int n, int S,
                                                         u32* __restrict__ out, int32_t* __restrict__ codes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (TYPE == 1) {
    CodecG1 p;
    codes[i] = codec_g1_decode(in + 8L * i, p);
    codec_g1_store(p, S, out + 3L * S * i);
  } else {
    CodecG2 p;
    codes[i] = codec_g2_decode(in + 16L * i, p);
    codec_g2_store(p, S, out + 6L * S * i);
  }
}

// n compressed points into the 2 n prepared records of the GLV plan: record i = (x, y), record n + i = (beta x, y)
template <int TYPE>
__global__ __launch_bounds__(64) void k_codec_decompress_prepared(const u32* __restrict__ in, int n,
                                                                  u32* __restrict__ aff, int32_t* __restrict__ codes) {
  using CV = std::conditional_t<TYPE == 1, G1Cfg, G2Cfg>;
  using IO = CurveIO<CV>;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Aff<typename CV::EA> q, q2;
  if constexpr (TYPE == 1)
    codes[i] = codec_g1_decode_prepared(in + 8L * i, q, q2);
  else
    codes[i] = codec_g2_decode_prepared(in + 16L * i, q, q2);
  IO::store_aff(q, aff + (size_t)i * IO::AFF_WORDS);
  IO::store_aff(q2, aff + (size_t)(n + i) * IO::AFF_WORDS);
}

// The order-r check of the G2 records k_codec_decompress_prepared has just written (affine Montgomery already): a
// finite point with [r]P != O gets code 4 and the (0, 0) marker in both records.  A kernel of its own, so that the
// decoder keeps its registers.
__global__ __launch_bounds__(64) void k_codec_subgroup_g2(u32* __restrict__ aff, int n, int32_t* __restrict__ codes) {
  using IO = CurveIO<G2Cfg>;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Aff<G2Cfg::EA> q = IO::load_aff(aff + (size_t)i * IO::AFF_WORDS);
  if (is_inf(q) || is_inf(scalar_mul<G2Cfg>(q, GlvConsts::R32, 8))) return;
  codes[i] = CODEC_E_SUBGROUP;
  for (int k = 0; k < IO::AFF_WORDS; k++) {
    aff[(size_t)i * IO::AFF_WORDS + k] = 0;
    aff[(size_t)(n + i) * IO::AFF_WORDS + k] = 0;
  }
}

template <int TYPE>
__global__ __launch_bounds__(64) void k_codec_compress(const u32* __restrict__ in, int n, int S,
                                                       u32* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (TYPE == 1)
    codec_g1_encode(in + 3L * S * i, S, out + 8L * i);
  else
    codec_g2_encode(in + 6L * S * i, S, out + 16L * i);
}

// K proofs of 32 words (A 8 | B 16 | C 8) into K records of 192 words (A 48 | B 96 | C 48, wire-out).  Blocks
// [0, g1_blocks): lane t decodes A (t even) or C (t odd) of proof t / 2; the blocks after them: lane j decodes B of
// proof j.  codes3: three codes per proof, A, B, C.
__global__ __launch_bounds__(64) void k_codec_proofs(const u32* __restrict__ in, int k, int g1_blocks,
                                                     u32* __restrict__ recs, int32_t* __restrict__ codes3) {
  if ((int)blockIdx.x < g1_blocks) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2L * k) return;
    const long i = t >> 1;
    const int c = (int)(t & 1);
    CodecG1 p;
    codes3[3 * i + 2 * c] = codec_g1_decode(in + 32 * i + 24 * c, p);
    codec_g1_store(p, 16, recs + 192 * i + 144 * c);
  } else {
    const long i = (long)(blockIdx.x - g1_blocks) * blockDim.x + threadIdx.x;
    if (i >= k) return;
    CodecG2 p;
    codes3[3 * i + 1] = codec_g2_decode(in + 32 * i + 8, p);
    codec_g2_store(p, 16, recs + 192 * i + 48);
  }
}
// the code of a proof: the first non-zero one of A, B, C
__global__ __launch_bounds__(256) void k_codec_proof_codes(const int32_t* __restrict__ codes3, int k,
                                                           int32_t* __restrict__ codes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int32_t a = codes3[3L * i], b = codes3[3L * i + 1], c = codes3[3L * i + 2];
  codes[i] = a ? a : (b ? b : c);
}
#endif

}  // namespace ozk
