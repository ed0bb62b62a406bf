// TEST INFRASTRUCTURE: compiles the pairing tower and steps (fq12.cuh) for the HOST with g++, so the Fq6 / Fq12
// arithmetic, the Miller loop and the final exponentiation (and their compile-time bound proofs) are checked against
// tests/pairing_ref.py without a GPU.  Not linked into the product library.
//
// Fq12 values cross this interface as 96 words (the GT wire order, little-endian canonical); Fq6 as the first 48.
// hi != 0 loads every Fq component as its Montgomery value plus p: the top of the Fe2<32> bound every Fq6 / Fq12
// operation takes.
#include "../../octopuszk_amd/csrc/fq12.cuh"
#include <string.h>
using namespace ozk;

static Fe<FqParams, 32> ld(const u32* w, int hi) {
  u32 t[8];
  memcpy(t, w, 32);
  const auto x = canonical(to_mont<FqParams>(t));
  if (!hi) return x;
  return Fe<FqParams, 32>(add(x, fe_const<FqParams, 16>(FqParams::P)));
}
static F2 ld2(const u32* w, int hi) {
  F2 r;
  r.c0 = ld(w, hi);
  r.c1 = ld(w + 8, hi);
  return r;
}
static void st2(const F2& a, u32* w) {
  from_mont(a.c0, *(u32(*)[8])w);
  from_mont(a.c1, *(u32(*)[8])(w + 8));
}
static Fe6 ld6(const u32* w, int hi) { return Fe6{ld2(w, hi), ld2(w + 16, hi), ld2(w + 32, hi)}; }
static void st6(const Fe6& a, u32* w) {
  st2(a.c0, w);
  st2(a.c1, w + 16);
  st2(a.c2, w + 32);
}
static Fe12 ld12(const u32* w, int hi) { return Fe12{ld6(w, hi), ld6(w + 48, hi)}; }
static void st12(const Fe12& a, u32* w) {
  st6(a.c0, w);
  st6(a.c1, w + 48);
}

static void g1_affine(const u32* p, Fe<FqParams, 32>& x, Fe<FqParams, 32>& y) {
  const auto X = ld(p, 0), Y = ld(p + 8, 0), Z = ld(p + 16, 0);
  if (is_zero(Z)) {
    x = fe_zero<FqParams>();
    y = fe_one<FqParams>();
    return;
  }
  const Fe<FqParams, 32> zi = inv(Z), z2 = Fe<FqParams, 32>(sqr(zi));
  x = Fe<FqParams, 32>(mul(X, z2));
  y = Fe<FqParams, 32>(mul(Y, Fe<FqParams, 32>(mul(z2, zi))));
}
static void g2_affine(const u32* q, F2& x, F2& y) {
  const F2 X = ld2(q, 0), Y = ld2(q + 16, 0), Z = ld2(q + 32, 0);
  if (is_zero(Z)) {
    x = f2_zero();
    y = f2_one();
    return;
  }
  const F2 zi = inv(Z), z2 = sqr(zi);
  x = mul(X, z2);
  y = mul(Y, mul(z2, zi));
}
// the device's k_g2_prepare / miller (pairing.hip), step for step
static void steps(const u32* q, Ell* out) {
  F2 x, y;
  g2_affine(q, x, y);
  G2Proj cur{x, y, f2_one()};
  F2 bx = x, by = y;
  for (int s = 0; s < pc::ATE_STEPS; s++) {
    const int kind = pc::ATE_STEP_KIND[s];
    if (kind == 0) {
      out[s] = doubling_step(cur);
    } else {
      if (kind >= 2) {
        mul_by_q(bx, by);
        if (kind == 3) by = f2_neg(by);
      }
      out[s] = mixed_addition_step(bx, by, cur);
    }
  }
}
static Fe12 miller(const u32* p, const u32* q) {
  Fe<FqParams, 32> px, py;
  g1_affine(p, px, py);
  Ell c[pc::ATE_STEPS];
  steps(q, c);
  Fe12 f = f12_one();
  for (int s = 0; s < pc::ATE_STEPS; s++) {
    if (pc::ATE_STEP_KIND[s] == 0) f = sqr(f);
    f = apply_line(f, c[s], px, py);
  }
  return f;
}

extern "C" {

// Fq6: 0 mul, 1 sqr, 2 inv, 3..5 Frobenius 1..3, 6 mul_by_v
void pc_f6_op(int op, int hi, const u32* a, const u32* b, u32* out) {
  const Fe6 x = ld6(a, hi), y = ld6(b, hi);
  Fe6 r = f6_zero();
  switch (op) {
    case 0: r = mul(x, y); break;
    case 1: r = sqr(x); break;
    case 2: r = inv(x); break;
    case 3: r = frobenius<1>(x); break;
    case 4: r = frobenius<2>(x); break;
    case 5: r = frobenius<3>(x); break;
    case 6: r = mul_by_v(x); break;
  }
  st6(r, out);
}
// Fq12: 0 mul, 1 sqr, 2 inv, 3..5 Frobenius 1..3, 6 cyclotomic_sqr, 7 conj, 8 final exponentiation,
// 9 its first chunk, 10 exp_by_neg_z, 11 equality (out[0])
void pc_f12_op(int op, int hi, const u32* a, const u32* b, u32* out) {
  const Fe12 x = ld12(a, hi), y = ld12(b, hi);
  Fe12 r = f12_one();
  switch (op) {
    case 0: r = mul(x, y); break;
    case 1: r = sqr(x); break;
    case 2: r = inv(x); break;
    case 3: r = frobenius<1>(x); break;
    case 4: r = frobenius<2>(x); break;
    case 5: r = frobenius<3>(x); break;
    case 6: r = cyclotomic_sqr(x); break;
    case 7: r = conj(x); break;
    case 8: r = final_exponentiation(x); break;
    case 9: r = final_exp_first_chunk(x); break;
    case 10: r = exp_by_neg_z(x); break;
    case 11: memset(out, 0, 96 * 4); out[0] = f12_eq(x, y); return;
  }
  st12(r, out);
}
// a * (ell0, ellVW, ellVV) as mulBy024 takes them; ell = 3 x 16 words
void pc_mul_by_024(int hi, const u32* a, const u32* ell, u32* out) {
  st12(mul_by_024(ld12(a, hi), ld2(ell, hi), ld2(ell + 16, hi), ld2(ell + 32, hi)), out);
}
// precomputeG2 of a wire-in G2 point: 102 x (ell0, ellVW, ellVV), 48 words each
void pc_prepare(const u32* q, u32* out) {
  Ell c[pc::ATE_STEPS];
  steps(q, c);
  for (int s = 0; s < pc::ATE_STEPS; s++) {
    st2(c[s].ell0, out + 48 * s);
    st2(c[s].ellVW, out + 48 * s + 16);
    st2(c[s].ellVV, out + 48 * s + 32);
  }
}
// wire-in P (24 words), Q (48 words): the Miller value (final = 0) or the reduced pairing (final = 1)
void pc_pairing(int final_exp, const u32* p, const u32* q, u32* out) {
  const Fe12 f = miller(p, q);
  st12(final_exp ? final_exponentiation(f) : f, out);
}

}  // extern "C"
