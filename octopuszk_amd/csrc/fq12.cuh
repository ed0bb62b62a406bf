// The pairing tower over fq2.cuh, one element per lane:
//   Fq6  = Fq2[v]/(v^3 - xi),  xi = 9 + u      (algebra/fields/Fp6_3Over2.java)
//   Fq12 = Fq6[w]/(w^2 - v)                    (algebra/fields/Fp12_2Over3Over2.java)
// and the line steps and final exponentiation of the optimal-ate pairing (BNPairing.java).
//
// Bounds: every Fq2 component of an Fq6 / Fq12 is an Fe2<32> (< 2p).  Sums and differences are fed straight into
// the lazily reduced Fq2 product (fq2.cuh mul; lazy_ok checks them at compile time) and brought back under 2p with
// f2n() wherever they are stored or squared, so every formula below type-checks against fp29.cuh's bound proofs.
// All of it compiles for the host too (OZK_HD / OZK_BIG): tests/native/pairing_hostcheck.cpp builds it with g++.
#pragma once
#include "fq2.cuh"
#include "pairing_consts_gen.h"

// The large tower operations are separate functions on the device (one copy of their code each, called from the
// loops of the Miller loop and the final exponentiation) instead of being inlined at every use.
#if defined(__HIPCC__)
#define OZK_BIG __host__ __device__ __noinline__
#else
#define OZK_BIG inline
#endif

namespace ozk {

using F2 = Fe2<32>;

// back under 2p: conditional subtractions up to 128/16 p, one quotient-estimate subtraction above
template <int B>
OZK_HD F2 f2n(const Fe2<B>& a) {
  if constexpr (B <= 32) {
    return a;
  } else if constexpr (B <= 128) {
    return reduce_to<32>(a);
  } else {
    F2 r;
    r.c0 = Fe<FqParams, 32>(reduce_q(a.c0));
    r.c1 = Fe<FqParams, 32>(reduce_q(a.c1));
    return r;
  }
}
OZK_HD F2 f2_const(const u32 (&c)[2][9]) {
  F2 r;
  r.c0 = Fe<FqParams, 32>(fe_const<FqParams, 16>(c[0]));
  r.c1 = Fe<FqParams, 32>(fe_const<FqParams, 16>(c[1]));
  return r;
}
OZK_HD F2 f2_zero() { return F2(el_zero(F2())); }
OZK_HD F2 f2_one() { return F2(el_one(F2())); }
template <int B1, int B2>
OZK_HD F2 f2_add(const Fe2<B1>& a, const Fe2<B2>& b) { return f2n(add(a, b)); }
template <int B1, int B2>
OZK_HD F2 f2_sub(const Fe2<B1>& a, const Fe2<B2>& b) { return f2n(sub(a, b)); }
OZK_HD F2 f2_neg(const F2& a) { return f2n(neg(a)); }
OZK_HD F2 f2_conj(const F2& a) {  // Fp2 FrobeniusMap(1): u^q = -u
  F2 r;
  r.c0 = a.c0;
  r.c1 = Fe<FqParams, 32>(reduce_to<32>(neg(a.c1)));
  return r;
}
// xi a = (9 a0 - a1) + (a0 + 9 a1) u, by additions (Fp6_3Over2.java:32-34 multiplies by the constant)
OZK_HD F2 mul_xi(const F2& a) {
  const auto a9 = add(dbl(dbl(dbl(a))), a);   // < 288/16 p
  F2 r;
  r.c0 = Fe<FqParams, 32>(reduce_q(sub(a9.c0, a.c1)));
  r.c1 = Fe<FqParams, 32>(reduce_q(add(a.c0, a9.c1)));
  return r;
}

// ---------------------------------------------------------------------------------------------- Fq6
struct Fe6 {
  F2 c0, c1, c2;
};
OZK_HD Fe6 f6_zero() { return Fe6{f2_zero(), f2_zero(), f2_zero()}; }
OZK_HD Fe6 f6_one() { return Fe6{f2_one(), f2_zero(), f2_zero()}; }
OZK_HD Fe6 add(const Fe6& a, const Fe6& b) { return Fe6{f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
OZK_HD Fe6 sub(const Fe6& a, const Fe6& b) { return Fe6{f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
OZK_HD Fe6 neg(const Fe6& a) { return Fe6{f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
OZK_HD bool is_zero(const Fe6& a) { return is_zero(a.c0) && is_zero(a.c1) && is_zero(a.c2); }
OZK_HD Fe6 mul_by_v(const Fe6& a) { return Fe6{mul_xi(a.c2), a.c0, a.c1}; }   // Fp12_2Over3Over2.java:33-35
OZK_HD Fe6 mul(const Fe6& a, const F2& k) { return Fe6{mul(a.c0, k), mul(a.c1, k), mul(a.c2, k)}; }
// Fp6_3Over2.java:35-49 (Karatsuba: 6 Fq2 products)
OZK_BIG Fe6 mul(const Fe6& a, const Fe6& b) {
  const F2 c0C0 = mul(a.c0, b.c0), c1C1 = mul(a.c1, b.c1), c2C2 = mul(a.c2, b.c2);
  const F2 t0 = mul(add(a.c1, a.c2), add(b.c1, b.c2));
  const F2 t1 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
  const F2 t2 = mul(add(a.c0, a.c2), add(b.c0, b.c2));
  const F2 c0F = f2n(sub(t0, add(c1C1, c2C2)));
  const F2 c1F = f2n(sub(t1, add(c0C0, c1C1)));
  Fe6 r;
  r.c0 = f2_add(c0C0, mul_xi(c0F));
  r.c1 = f2_add(c1F, mul_xi(c2C2));
  r.c2 = f2n(sub(add(t2, c1C1), add(c0C0, c2C2)));
  return r;
}
// Fp6_3Over2.java:72-87 (CH-SQR2)
OZK_HD Fe6 sqr(const Fe6& a) {
  const F2 s0 = sqr(a.c0);
  const F2 c0c1 = mul(a.c0, a.c1);
  const F2 s1 = f2n(dbl(c0c1));
  const F2 s2 = sqr(f2n(add(sub(a.c0, a.c1), a.c2)));
  const F2 c1c2 = mul(a.c1, a.c2);
  const F2 s3 = f2n(dbl(c1c2));
  const F2 s4 = sqr(a.c2);
  Fe6 r;
  r.c0 = f2_add(s0, mul_xi(s3));
  r.c1 = f2_add(s1, mul_xi(s4));
  r.c2 = f2n(sub(add(add(s1, s2), s3), add(s0, s4)));
  return r;
}
// Fp6_3Over2.java:88-103 (Algorithm 17): one Fq2 inversion (through its norm to the safegcd Fq inversion)
OZK_BIG Fe6 inv(const Fe6& a) {
  const F2 t0 = sqr(a.c0), t1 = sqr(a.c1), t2 = sqr(a.c2);
  const F2 t3 = mul(a.c0, a.c1), t4 = mul(a.c0, a.c2), t5 = mul(a.c1, a.c2);
  const F2 s0 = f2_sub(t0, mul_xi(t5));
  const F2 s1 = f2_sub(mul_xi(t2), t3);
  const F2 s2 = f2_sub(t1, t4);
  const F2 d = f2_add(mul(a.c0, s0), mul_xi(f2_add(mul(a.c2, s1), mul(a.c1, s2))));
  const F2 t6 = inv(d);
  return Fe6{mul(t6, s0), mul(t6, s1), mul(t6, s2)};
}
// Fp6_3Over2.java:104-109
template <int K>
OZK_HD Fe6 frobenius(const Fe6& a) {
  constexpr int k6 = K % 6;
  const F2 x0 = (K & 1) ? f2_conj(a.c0) : a.c0;
  const F2 x1 = (K & 1) ? f2_conj(a.c1) : a.c1;
  const F2 x2 = (K & 1) ? f2_conj(a.c2) : a.c2;
  return Fe6{x0, mul(f2_const(pc::FQ6_FROB_C1[k6]), x1), mul(f2_const(pc::FQ6_FROB_C2[k6]), x2)};
}

// ---------------------------------------------------------------------------------------------- Fq12
struct Fe12 {
  Fe6 c0, c1;
};
OZK_HD Fe12 f12_one() { return Fe12{f6_one(), f6_zero()}; }
OZK_HD bool is_zero(const Fe12& a) { return is_zero(a.c0) && is_zero(a.c1); }
OZK_HD Fe12 conj(const Fe12& a) { return Fe12{a.c0, neg(a.c1)}; }   // Fp12_2Over3Over2.java:92-94 unitaryInverse
// Fp12_2Over3Over2.java:36-45 (Karatsuba: 3 Fq6 products)
OZK_BIG Fe12 mul(const Fe12& a, const Fe12& b) {
  const Fe6 c0C0 = mul(a.c0, b.c0), c1C1 = mul(a.c1, b.c1);
  const Fe6 t = mul(add(a.c0, a.c1), add(b.c0, b.c1));
  return Fe12{add(c0C0, mul_by_v(c1C1)), sub(sub(t, c0C0), c1C1)};
}
// Fp12_2Over3Over2.java:67-76 (complex squaring: 2 Fq6 products)
OZK_BIG Fe12 sqr(const Fe12& a) {
  const Fe6 c0c1 = mul(a.c0, a.c1);
  const Fe6 factor = mul(add(a.c0, a.c1), add(a.c0, mul_by_v(a.c1)));
  return Fe12{sub(sub(factor, c0c1), mul_by_v(c0c1)), add(c0c1, c0c1)};
}
// Fp12_2Over3Over2.java:77-85 (Algorithm 8): the norm to Fq6, one Fq6 inversion
OZK_BIG Fe12 inv(const Fe12& a) {
  const Fe6 t0 = sqr(a.c0), t1 = sqr(a.c1);
  const Fe6 t3 = inv(sub(t0, mul_by_v(t1)));
  return Fe12{mul(a.c0, t3), neg(mul(a.c1, t3))};
}
// Fp12_2Over3Over2.java:86-91
template <int K>
OZK_BIG Fe12 frobenius(const Fe12& a) {
  return Fe12{frobenius<K>(a.c0), mul(frobenius<K>(a.c1), f2_const(pc::FQ12_FROB_C1[K % 12]))};
}
// (x + y s)^2 with s^2 = xi, as Fp12_2Over3Over2.java:105-108 writes it: ((x + y)(x + xi y) - xy - xi xy, 2 xy)
OZK_HD void sqr_pair(const F2& x, const F2& y, F2& t0, F2& t1) {
  const F2 tmp = mul(x, y);
  const F2 f = mul(add(x, y), add(x, mul_xi(y)));
  t0 = f2n(sub(f, add(tmp, mul_xi(tmp))));
  t1 = f2n(dbl(tmp));
}
OZK_HD F2 three_minus_two(const F2& t, const F2& z) {   // 3 t - 2 z = (t - z) + (t - z) + t
  const F2 d = f2_sub(t, z);
  return f2n(add(dbl(d), t));
}
OZK_HD F2 three_plus_two(const F2& t, const F2& z) {    // 3 t + 2 z = (t + z) + (t + z) + t
  const F2 s = f2_add(t, z);
  return f2n(add(dbl(s), t));
}
// Fp12_2Over3Over2.java:95-151 (Granger-Scott): equals sqr() on the cyclotomic subgroup only
OZK_BIG Fe12 cyclotomic_sqr(const Fe12& a) {
  F2 z0 = a.c0.c0, z4 = a.c0.c1, z3 = a.c0.c2;
  F2 z2 = a.c1.c0, z1 = a.c1.c1, z5 = a.c1.c2;
  F2 t0, t1, t2, t3, t4, t5;
  sqr_pair(z0, z1, t0, t1);
  sqr_pair(z2, z3, t2, t3);
  sqr_pair(z4, z5, t4, t5);
  z0 = three_minus_two(t0, z0);
  z1 = three_plus_two(t1, z1);
  z2 = three_plus_two(mul_xi(t5), z2);
  z3 = three_minus_two(t4, z3);
  z4 = three_minus_two(t2, z4);
  z5 = three_plus_two(t3, z5);
  return Fe12{Fe6{z0, z4, z3}, Fe6{z2, z1, z5}};
}
// Fp12_2Over3Over2.java:152-216: a * (x0 + x2 v + x4 v w) with x0 = ell0, x2 = ellVV, x4 = ellVW (13 Fq2 products)
OZK_BIG Fe12 mul_by_024(const Fe12& a, const F2& x0, const F2& x4, const F2& x2) {
  const F2 z0 = a.c0.c0, z1 = a.c0.c1, z2 = a.c0.c2, z3 = a.c1.c0, z4 = a.c1.c1, z5 = a.c1.c2;
  const F2 D0 = mul(z0, x0), D2 = mul(z2, x2), D4 = mul(z4, x4);
  const F2 t2 = f2_add(z0, z4);
  const F2 t1 = f2_add(z0, z2);
  const F2 s0 = f2n(add(add(z1, z3), z5));
  Fe12 r;
  F2 S1 = mul(z1, x2);
  r.c0.c0 = f2_add(mul_xi(f2_add(S1, D4)), D0);
  F2 T3 = mul(z5, x4);
  S1 = f2_add(S1, T3);
  F2 T4 = mul_xi(f2_add(T3, D2));
  T3 = mul(z1, x0);
  S1 = f2_add(S1, T3);
  r.c0.c1 = f2_add(T4, T3);
  T3 = f2n(sub(mul(t1, add(x0, x2)), add(D0, D2)));
  T4 = mul(z3, x4);
  S1 = f2_add(S1, T4);
  r.c0.c2 = f2_add(T3, T4);
  T3 = f2n(sub(mul(add(z2, z4), add(x2, x4)), add(D2, D4)));
  T4 = mul_xi(T3);
  T3 = mul(z3, x0);
  S1 = f2_add(S1, T3);
  r.c1.c0 = f2_add(T4, T3);
  T3 = mul(z5, x2);
  S1 = f2_add(S1, T3);
  T4 = mul_xi(T3);
  T3 = f2n(sub(mul(t2, add(x0, x4)), add(D0, D4)));
  r.c1.c1 = f2_add(T4, T3);
  r.c1.c2 = f2_sub(mul(s0, f2n(add(add(x0, x2), x4))), S1);
  return r;
}
// Fp12_2Over3Over2.java:217-230, exponent a 64-bit word (z = u has 63 bits)
OZK_HD Fe12 cyclotomic_exp(const Fe12& a, u64 e, int bits) {
  Fe12 res = a;   // the top bit: one * a
  for (int i = bits - 2; i >= 0; i--) {
    res = cyclotomic_sqr(res);
    if ((e >> i) & 1) res = mul(res, a);
  }
  return res;
}

// ---------------------------------------------------------------------------------------------- pairing steps
struct Ell {
  F2 ell0, ellVW, ellVV;
};
struct G2Proj {
  F2 X, Y, Z;
};
// BNPairing.java:84-110 (doubling step of the flipped Miller loop, homogeneous projective coordinates)
OZK_BIG Ell doubling_step(G2Proj& cur) {
  const Fe<FqParams, 16> two_inv = fe_const<FqParams, 16>(pc::TWO_INV);
  const F2 X = cur.X, Y = cur.Y, Z = cur.Z;
  const F2 A = scale(mul(X, Y), two_inv);
  const F2 B = sqr(Y);
  const F2 C = sqr(Z);
  const F2 D = f2n(add(dbl(C), C));
  const F2 E = mul(f2_const(pc::TWIST_B), D);
  const F2 Fv = f2n(add(dbl(E), E));
  const F2 G = scale(add(B, Fv), two_inv);
  const F2 H = f2n(sub(sqr(f2_add(Y, Z)), add(B, C)));
  const F2 I = f2_sub(E, B);
  const F2 J = sqr(X);
  const F2 ESq = sqr(E);
  cur.X = mul(A, sub(B, Fv));
  cur.Y = f2n(sub(sqr(G), add(dbl(ESq), ESq)));
  cur.Z = mul(B, H);
  return Ell{mul_xi(I), f2_neg(H), f2n(add(dbl(J), J))};
}
// BNPairing.java:112-136 (mixed addition step with the affine base (x2, y2))
OZK_BIG Ell mixed_addition_step(const F2& x2, const F2& y2, G2Proj& cur) {
  const F2 X1 = cur.X, Y1 = cur.Y, Z1 = cur.Z;
  const F2 D = f2n(sub(X1, mul(x2, Z1)));
  const F2 E = f2n(sub(Y1, mul(y2, Z1)));
  const F2 Fv = sqr(D);
  const F2 G = sqr(E);
  const F2 H = mul(D, Fv);
  const F2 I = mul(X1, Fv);
  const F2 J = f2n(sub(add(H, mul(Z1, G)), dbl(I)));
  cur.X = mul(D, J);
  cur.Y = f2n(sub(mul(E, sub(I, J)), mul(H, Y1)));
  cur.Z = mul(Z1, H);
  return Ell{mul_xi(f2n(sub(mul(E, x2), mul(D, y2)))), D, f2_neg(E)};
}
// BNPairing.java:138-143 on an affine point (Z = 1 stays 1 under the Frobenius)
OZK_HD void mul_by_q(F2& x, F2& y) {
  x = mul(f2_const(pc::Q_X_MUL_TWIST), f2_conj(x));
  y = mul(f2_const(pc::Q_Y_MUL_TWIST), f2_conj(y));
}
// one line of the Miller loop: f * (ell0 + ellVV xP v + ellVW yP v w)   (BNPairing.java:257)
OZK_HD Fe12 apply_line(const Fe12& f, const Ell& c, const Fe<FqParams, 32>& px, const Fe<FqParams, 32>& py) {
  const F2 vw = scale(c.ellVW, Fe<FqParams, 16>(reduce_to<16>(py)));
  const F2 vv = scale(c.ellVV, Fe<FqParams, 16>(reduce_to<16>(px)));
  return mul_by_024(f, c.ell0, vw, vv);
}

// BNPairing.java:145-151 (z is positive: the result is conjugated)
OZK_HD Fe12 exp_by_neg_z(const Fe12& a) {
  const Fe12 r = cyclotomic_exp(a, pc::FINAL_EXP_Z, pc::FINAL_EXP_Z_BITS);
  return pc::FINAL_EXP_Z_NEGATIVE ? r : conj(r);
}
// BNPairing.java:153-171: elt^((q^6 - 1)(q^2 + 1))
OZK_BIG Fe12 final_exp_first_chunk(const Fe12& elt) {
  const Fe12 C = mul(conj(elt), inv(elt));
  return mul(frobenius<2>(C), C);
}
// BNPairing.java:173-234.  The three exp_by_neg_z run as one loop (one copy of the exponentiation's code):
// pass 0 gives A = elt^-z, B = A^2, D = A^6; pass 1 E = D^-z, F = E^2; pass 2 G = F^-z.
OZK_BIG Fe12 final_exp_last_chunk(const Fe12& elt) {
  Fe12 x = elt, B, E, K;
  for (int pass = 0; pass < 3; pass++) {
    x = exp_by_neg_z(x);
    if (pass == 0) {
      B = cyclotomic_sqr(x);
      x = mul(cyclotomic_sqr(B), B);     // D
      K = conj(x);                       // H = conj(D), kept as the first factor of K
    } else if (pass == 1) {
      E = x;
      K = mul(K, E);                     // H E
      x = cyclotomic_sqr(x);             // F
    }
  }
  K = mul(conj(x), K);                   // K = I E H = conj(G) E conj(D)
  const Fe12 L = mul(K, B);
  const Fe12 N = mul(mul(K, E), elt);    // M elt
  const Fe12 P = mul(frobenius<1>(L), N);
  const Fe12 Rr = mul(frobenius<2>(K), P);
  const Fe12 U = frobenius<3>(mul(conj(elt), L));
  return mul(U, Rr);
}
OZK_BIG Fe12 final_exponentiation(const Fe12& f) { return final_exp_last_chunk(final_exp_first_chunk(f)); }

// ---------------------------------------------------------------------------------------------- storage
// raw Montgomery limbs (the loop-carried bounds), 9 words per Fq; STRIDE apart (lane-interleaved arrays)
constexpr int FE12_WORDS = 108;
constexpr int ELL_WORDS = 54;
OZK_HD void store_f2(const F2& a, u32* p, long stride) {
  for (int i = 0; i < 9; i++) {
    p[i * stride] = a.c0.l[i];
    p[(9 + i) * stride] = a.c1.l[i];
  }
}
OZK_HD F2 load_f2(const u32* p, long stride) {
  F2 a;
  for (int i = 0; i < 9; i++) {
    a.c0.l[i] = p[i * stride];
    a.c1.l[i] = p[(9 + i) * stride];
  }
  return a;
}
OZK_HD void store_f12(const Fe12& a, u32* p, long stride) {
  const F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int k = 0; k < 6; k++) store_f2(*c[k], p + 18 * k * stride, stride);
}
OZK_HD Fe12 load_f12(const u32* p, long stride) {
  Fe12 a;
  F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int k = 0; k < 6; k++) *c[k] = load_f2(p + 18 * k * stride, stride);
  return a;
}
// GT wire format: twelve 32-byte little-endian canonical Fq values, c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1
OZK_HD void f12_to_wire(const Fe12& a, u32* out) {
  const F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int k = 0; k < 6; k++) {
    u32 w[8];
    from_mont(c[k]->c0, w);
    for (int i = 0; i < 8; i++) out[16 * k + i] = w[i];
    from_mont(c[k]->c1, w);
    for (int i = 0; i < 8; i++) out[16 * k + 8 + i] = w[i];
  }
}
OZK_HD Fe12 f12_from_wire(const u32* in) {
  Fe12 a;
  F2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int k = 0; k < 6; k++) {
    u32 w[8];
    for (int i = 0; i < 8; i++) w[i] = in[16 * k + i];
    c[k]->c0 = Fe<FqParams, 32>(to_mont<FqParams>(w));
    for (int i = 0; i < 8; i++) w[i] = in[16 * k + 8 + i];
    c[k]->c1 = Fe<FqParams, 32>(to_mont<FqParams>(w));
  }
  return a;
}
OZK_HD bool f12_eq(const Fe12& a, const Fe12& b) {
  const F2* x[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  const F2* y[6] = {&b.c0.c0, &b.c0.c1, &b.c0.c2, &b.c1.c0, &b.c1.c1, &b.c1.c2};
  bool e = true;
  for (int k = 0; k < 6; k++) e = e && is_zero(sub(*x[k], *y[k]));
  return e;
}

}  // namespace ozk
