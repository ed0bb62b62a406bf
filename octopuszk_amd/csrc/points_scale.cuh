// n points, each multiplied by the SAME scalar: out_i = [k] P_i.  What a phase-2 key contribution
// does to delta_abc_g1 and query_h, and, with k = r - 1 on one point, the subgroup test of a new delta_g2.
//
// The scalar is shared, so it is recoded ONCE on the host into a digit schedule that travels as a kernel argument:
// the ladder's control flow is the same in every lane, and lanes part only in the exceptional branches of the group
// law (an input at infinity, an accumulator that meets +- the addend).
//
//   G1  k = k1 + k2 lambda (mod r), |k1|, |k2| < 2^128 (glv_decompose), and the pair in joint sparse form: one column
//       (d1, d2) in {-1, 0, 1}^2 per doubling, about half of them zero.  A non-zero column adds ONE affine point out of
//       P, phi(P) = (beta x, y), P + phi(P) = -phi^2(P) = (beta^2 x, -y) and T = P - phi(P), or its negative.  T is the
//       only one that costs anything: one affine addition with one inversion, (beta - 1) x != 0 because no point of
//       y^2 = x^3 + 3 over Fq has x = 0 (3 is not a square; tests/test_ceremony_cpu.py).
//   G2  the eigenvalue lambda holds on the order-r subgroup only and this must be exact on the whole twist (it IS the
//       subgroup test), so: the joint sparse form of (k, 0), which is the non-adjacent form of k, over P alone.
//
// Every addition is jac_madd (complete: P == Q doubles, P == -Q gives O) and jac_dbl is exact for every point, so
// the result is [k] P for any point of the curve and any k.  The result is normalised with the safegcd inversion and
// written as wire-in, Z = 1; O as ozk_points_decompress_dev writes it.
// The header compiles for the host too (tests/native/ceremony_hostcheck.cpp), the kernel only in points_scale.hip.
#pragma once
#include "fq2.cuh"
#include "glv.cuh"

namespace ozk {

// 4 bits per ladder step, step i in bits [4 (i & 7), +4) of word i >> 3, step len - 1 first
constexpr int SCALE_MAX_STEPS = 256;
constexpr u32 SCALE_D1 = 1, SCALE_N1 = 2, SCALE_D2 = 4, SCALE_N2 = 8;   // d1 != 0, d1 < 0, d2 != 0, d2 < 0
struct ScaleSchedule {
  u32 w[SCALE_MAX_STEPS / 8];
  int32_t len;
};
// (any schedule: a struct with SCALE_MAX_STEPS / 8 words behind .w and a .len; points_mul.cuh keeps its words in LDS)
template <class S>
OZK_HD u32 scale_step(const S& s, int i) { return (s.w[i >> 3] >> (4 * (i & 7))) & 15u; }

// ---------------------------------------------------------------------------------------------- recoding
// (on the host for ozk_points_scale_dev, on the device for the per-twiddle schedules of ec_fft.cuh and the per-point
// ones of points_mul.cuh)
// Joint sparse form (Solinas 2001) of two non-negative integers below 2^256, least significant column first, each
// column's signs flipped where its integer is to be subtracted (neg1 / neg2).  u = a mods 4 for an odd a, negated
// when a = +-3 (mod 8) and b = 2 (mod 4): then (a - u) / 2 is odd exactly when b / 2 is, so that non-zero columns
// pair up.  sum u_i 2^i = a whatever the choice of sign, which is all the ladder needs.
template <class S>
OZK_HD void scale_jsf(const u32 (&a_in)[8], bool neg1, const u32 (&b_in)[8], bool neg2, S& s) {
  u32 v[2][9];
  for (int i = 0; i < 8; i++) {
    v[0][i] = a_in[i];
    v[1][i] = b_in[i];
  }
  v[0][8] = v[1][8] = 0;
  const bool neg[2] = {neg1, neg2};
  for (int i = 0; i < SCALE_MAX_STEPS / 8; i++) s.w[i] = 0;
  int len = 0;
  for (;; len++) {
    u32 any = 0;
    for (int i = 0; i < 9; i++) any |= v[0][i] | v[1][i];
    if (!any || len == SCALE_MAX_STEPS) break;
    int u[2];
    for (int j = 0; j < 2; j++) {
      const u32 a = v[j][0], b = v[1 - j][0];
      u[j] = (a & 1) ? 2 - (int)(a & 3) : 0;
      if (u[j] && ((a & 7) == 3 || (a & 7) == 5) && (b & 3) == 2) u[j] = -u[j];
    }
    u32 code = 0;
    for (int j = 0; j < 2; j++) {
      if (u[j] > 0) v[j][0] &= ~1u;   // odd: a - 1
      if (u[j] < 0)                   // a + 1
        for (int i = 0; i < 9 && ++v[j][i] == 0; i++) {}
      for (int i = 0; i < 9; i++) v[j][i] = (v[j][i] >> 1) | (i < 8 ? v[j][i + 1] << 31 : 0u);
      if (u[j]) code |= (SCALE_D1 | (((u[j] < 0) != neg[j]) ? SCALE_N1 : 0u)) << (2 * j);
    }
    s.w[len >> 3] |= code << (4 * (len & 7));
  }
  s.len = len;
}
// k < r (the caller's check).  G1: the GLV halves jointly; G2: k alone.
template <class S>
OZK_HD void scale_recode(const u32 (&k)[8], bool glv, S& s) {
  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!glv) return scale_jsf(k, false, zero, false, s);
  u32 h1[4], h2[4], k1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, k2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool neg1, neg2;
  glv_decompose(k, h1, neg1, h2, neg2);
  for (int i = 0; i < 4; i++) {
    k1[i] = h1[i];
    k2[i] = h2[i];
  }
  scale_jsf(k1, neg1, k2, neg2, s);
}
OZK_HD bool scale_scalar_ok(const u32 (&k)[8]) { return !mp_geq<8>(k, GlvConsts::R32); }

// ---------------------------------------------------------------------------------------------- one point
// [k] q for the schedule of k.  GLV (G1 only) reads both digits of a step, otherwise the second is never set.
template <class CV, bool GLV, class S>
OZK_HD Jac<CV> scale_ladder(const Aff<typename CV::EA>& q, const S& s) {
  using EA = typename CV::EA;
  Jac<CV> acc = jac_infinity<CV>();
  if (is_inf(q)) return acc;
  EA bx = q.x, b2x = q.x, tx = q.x, ty = q.y;
  if constexpr (GLV) {
    bx = EA(canonical(scale(q.x, glv_beta<CV>())));
    b2x = EA(canonical(scale(bx, glv_beta<CV>())));
    // T = q + (beta x, -y): slope -2 y / (beta x - x)
    const auto sl = mul(dbl(neg(q.y)), inv(sub(bx, q.x)));
    tx = EA(canonical(sub(sqr(sl), add(q.x, bx))));
    ty = EA(canonical(sub(mul(sl, sub(q.x, tx)), q.y)));
  }
#pragma unroll 1
  for (int i = s.len - 1; i >= 0; i--) {
    acc = jac_dbl<CV>(acc);
    const u32 c = scale_step(s, i);   // the same in every lane for a shared schedule; a lane's own in points_mul.cuh
    if (c == 0) continue;
    Aff<EA> a;
    bool negate = (c & SCALE_N1) != 0;
    a.x = q.x;
    a.y = q.y;
    if constexpr (GLV) {
      const bool d1 = (c & SCALE_D1) != 0, d2 = (c & SCALE_D2) != 0;
      const bool n1 = (c & SCALE_N1) != 0, n2 = (c & SCALE_N2) != 0;
      const bool same = d1 && d2 && n1 == n2, diff = d1 && d2 && n1 != n2;
      //   (+-1, 0) +-(x, y)      (0, +-1) +-(beta x, y)      +-(1, 1) -+(beta^2 x, y)      +-(1, -1) +-T
      a.x = select_el(same, b2x, select_el(diff, tx, select_el(d1, q.x, bx)));
      a.y = select_el(diff, ty, q.y);
      negate = same ? !n1 : (d1 ? n1 : n2);
    }
    if (negate) a.y = EA(canonical(neg(a.y)));
    acc = jac_madd<CV>(acc, a);
  }
  return acc;
}

// in: one wire-in point, out: [k] of it as wire-in with Z = 1 (O: (0, 1, 0) / ((0, 0), (1, 0), (0, 0))).  The point
// is read whole before anything is written, so out may be in.
template <class CV, bool GLV, class S>
OZK_HD void scale_point(const u32* in, const S& s, u32* out) {
  using IO = CurveIO<CV>;
  IO::template write<WireIn>(scale_ladder<CV, GLV>(IO::aff_from_wire(in), s), out);
}

#if defined(__HIPCC__)
// One point per lane, one wave per workgroup (as the codec kernels).  in and out may be the same buffer: no
// __restrict__, and a lane touches its own record only.
template <int TYPE>   // 1: G1, 2: G2
__global__ __launch_bounds__(64) void k_points_scale(const u32* in, int n, ScaleSchedule s, u32* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (TYPE == 1)
    scale_point<G1Cfg, true>(in + 24L * i, s, out + 24L * i);
  else
    scale_point<G2Cfg, false>(in + 48L * i, s, out + 48L * i);
}
#endif

}  // namespace ozk
