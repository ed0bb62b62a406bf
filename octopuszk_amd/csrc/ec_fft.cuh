// Point kernels of the setup from a powers-of-tau string: a radix-2 FFT whose values are curve points
// and whose twiddles are Fr scalars, a sparse matrix times a vector of points, and a pointwise sum of two vectors.
//
// The transform is decimation in time over a bit-reversed copy, in place, one butterfly per lane:
//     (a, b) -> (a + [w] b, a - [w] b)
// A pass of half-size h has B = n / 2h blocks and h twiddles w = omega^(j B), j < h.  Butterfly t of a pass is
// (j, k) = (t / B, t % B): neighbouring lanes are the SAME offset j of different blocks k, so that while B >= 64 all
// lanes of a wave share their twiddle and run its digit schedule in lockstep, as k_points_scale does for its one
// scalar.  In the last six passes (B < 64) a wave holds 64 / B twiddles: the same code, now with lanes idle in the
// additions their own schedule skips.  The schedules (ScaleSchedule of points_scale.cuh, 132 bytes) are recoded once
// per call on the device: `last` holds n / 2 of them for c omega^j (the last pass), `inner` n / 4 for omega^(2 j)
// (every other pass reads it at stride B / 2).  c = 1 for the forward transform; the inverse uses omega^-1 and
// c = 1 / n, folded into the last pass: out = [c] a +- [c omega^-j] b, where [c] a is one more ladder of a schedule the
// whole pass shares.  A butterfly whose twiddle is 1 (j = 0, c = 1) runs no ladder.
//
//   G1  GLV halves in joint sparse form: exact on all of E(Fq), which IS the order-r group (cofactor 1).
//   G2  the non-adjacent form of the twiddle, no endomorphism: exact on the whole twist, so the G2 instance assumes
//       nothing about its input.
// Additions are jac_madd / jac_dbl (complete); a butterfly normalises its two results with ONE shared inversion.
// Every function here compiles for the host too (tests/native/ecfft_hostcheck.cpp); the kernels only under hipcc.
#pragma once
#include "points_scale.cuh"

namespace ozk {

// ---------------------------------------------------------------------------------------------- points
// a and -b (negate_b) or b, normalised with one inversion between them
template <class CV>
OZK_HD void ec_write2(const Jac<CV>& a, const Jac<CV>& b, bool negate_b, u32* oa, u32* ob) {
  using IO = CurveIO<CV>;
  const bool ia = is_inf(a), ib = is_inf(b);
  if (ia || ib) {
    IO::template write<WireIn>(a, oa);
    if (ib) return IO::template write_inf<WireIn>(ob);
    return IO::template write_jac<WireIn>(b, inv(b.Z), negate_b, ob);
  }
  const auto za = reduce_to<32>(a.Z), zb = reduce_to<32>(b.Z);
  const auto ti = inv(mul(za, zb));
  IO::template write_jac<WireIn>(a, mul(ti, zb), false, oa);
  IO::template write_jac<WireIn>(b, mul(ti, za), negate_b, ob);
}
template <class CV>
OZK_HD Aff<typename CV::EA> ec_to_affine(const Jac<CV>& r) {   // canonical; O as (0, 0)
  using IO = CurveIO<CV>;
  using EA = typename CV::EA;
  Aff<EA> q = IO::aff_infinity();
  if (is_inf(r)) return q;
  q = IO::jac_to_aff(r, inv(r.Z));
  q.x = EA(canonical(q.x));
  q.y = EA(canonical(q.y));
  return q;
}
template <class EA>
OZK_HD Aff<EA> ec_neg(const Aff<EA>& q) {   // -O = O: canonical(-0) = 0
  Aff<EA> m;
  m.x = q.x;
  m.y = EA(canonical(neg(q.y)));
  return m;
}

// out = a + b or a - b
template <class CV>
OZK_HD void points_add_one(const u32* pa, const u32* pb, bool negate_b, u32* out) {
  using IO = CurveIO<CV>;
  const auto a = IO::aff_from_wire(pa);
  auto b = IO::aff_from_wire(pb);
  if (negate_b) b = ec_neg(b);
  IO::template write<WireIn>(jac_madd<CV>(from_affine<CV>(a), b), out);
}

// ---------------------------------------------------------------------------------------------- twiddles
struct EcFftTwiddle {   // plain little-endian words, below r
  u32 base[8], k[8];
};
// k base^i mod r as 8 plain words
OZK_HD void ecfft_twiddle(const EcFftTwiddle& c, u32 i, u32 (&out)[8]) {
  using F = Fe<FrParams, 32>;
  F acc = F(to_mont<FrParams>(c.k)), b = F(to_mont<FrParams>(c.base));
  for (u32 e = i; e; e >>= 1) {
    if (e & 1) acc = F(mul(acc, b));
    b = F(sqr(b));
  }
  from_mont(acc, out);
}
// schedule i of a table: the recoding of k base^i, jointly over the GLV halves (G1) or alone (G2)
OZK_HD void ecfft_schedule(const EcFftTwiddle& c, u32 i, bool glv, ScaleSchedule& s) {
  u32 w[8];
  ecfft_twiddle(c, i, w);
  scale_recode(w, glv, s);
}

// ---------------------------------------------------------------------------------------------- one butterfly
// oa = [sa] a + [sb] b, ob = [sa] a - [sb] b; a null schedule stands for the factor 1.  pa / pb are read whole before
// oa / ob are written, so the butterfly may run in place.
template <class CV, bool GLV>
OZK_HD void ecfft_butterfly(const u32* pa, const u32* pb, const ScaleSchedule* sa, const ScaleSchedule* sb, u32* oa,
                            u32* ob) {
  auto a = CurveIO<CV>::aff_from_wire(pa);
  const auto b = CurveIO<CV>::aff_from_wire(pb);
  if (sa) a = ec_to_affine<CV>(scale_ladder<CV, GLV>(a, *sa));
  const Jac<CV> v = sb ? scale_ladder<CV, GLV>(b, *sb) : from_affine<CV>(b);
  const Jac<CV> sum = jac_madd<CV>(v, a);
  const Jac<CV> dif = jac_madd<CV>(v, ec_neg(a));   // v - a = -(a - v)
  ec_write2<CV>(sum, dif, true, oa, ob);
}

// ---------------------------------------------------------------------------------------------- sparse product
OZK_HD bool words_are(const u32* w, const u32 (&v)[8]) {
  u32 d = 0;
  for (int i = 0; i < 8; i++) d |= w[i] ^ v[i];
  return d == 0;
}
// acc + [c] P: c null or 1 adds P, c = r - 1 subtracts it, c = 0 (and every multiple of r below 2^256) adds nothing;
// any other c runs a per-lane double-and-add over its bits (scalar_mul), exact on the whole curve
template <class CV>
OZK_HD Jac<CV> sparse_term(const Jac<CV>& acc, const u32* p, const u32* c) {
  auto q = CurveIO<CV>::aff_from_wire(p);
  if (c) {
    u32 k[8];
    for (int i = 0; i < 8; i++) k[i] = c[i];
    reduce_mod_r(k);
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    u32 m1[8];
    for (int i = 0; i < 8; i++) m1[i] = GlvConsts::R32[i];
    m1[0] -= 1;   // r is odd
    if (words_are(k, m1)) {
      q = ec_neg(q);
    } else if (!words_are(k, one)) {
      const Jac<CV> v = is_inf(q) ? jac_infinity<CV>() : scalar_mul<CV>(q, k, 8);
      q = ec_to_affine<CV>(v);
    }
  }
  return jac_madd<CV>(acc, q);
}

#if defined(__HIPCC__)
constexpr int EC_LONG = 64;            // rows above this many terms are the long rows (R1CS_LONG of fft.hip)
constexpr int EC_LONG_LANES = 4096;    // partial sums of one long row, then 64, then 1

template <int TYPE>
__global__ __launch_bounds__(64) void k_ecfft_recode(EcFftTwiddle c, int n, ScaleSchedule* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ScaleSchedule s;
  ecfft_schedule(c, (u32)i, EcType<TYPE>::GLV, s);
  out[i] = s;
}

// out[bit-reversed i] = in[i], affine-normalised
template <int TYPE>
__global__ __launch_bounds__(64) void k_ecfft_permute(const u32* __restrict__ in, int n, int logn, u32* __restrict__ out) {
  using CV = typename EcType<TYPE>::CV;
  using IO = CurveIO<CV>;
  constexpr int PW = IO::WIRE_JAC_WORDS;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 j = logn ? __brev((u32)i) >> (32 - logn) : 0u;
  IO::template write_aff<WireIn>(IO::aff_from_wire(in + (size_t)PW * i), out + (size_t)PW * j);
}

// one pass of half-size h = 1 << logh over n = 1 << logn points, in place.  tab[j * stride]: the schedule of offset
// j; skip0: offset 0 has the twiddle 1; sa: the schedule applied to a (the inverse's last pass), or null
template <int TYPE>
__global__ __launch_bounds__(64) void k_ecfft_pass(u32* data, int logn, int logh, const ScaleSchedule* tab, int stride,
                                                   int skip0, const ScaleSchedule* sa) {
  using CV = typename EcType<TYPE>::CV;
  constexpr int PW = CurveIO<CV>::WIRE_JAC_WORDS;
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (1u << (logn - 1))) return;
  const int logb = logn - 1 - logh;
  const u32 j = t >> logb, k = t & ((1u << logb) - 1);
  u32* pa = data + (size_t)PW * (((size_t)k << (logh + 1)) + j);
  u32* pb = pa + ((size_t)PW << logh);
  const ScaleSchedule* sb = (j == 0 && skip0) ? nullptr : tab + (size_t)j * stride;
  ecfft_butterfly<CV, EcType<TYPE>::GLV>(pa, pb, sa, sb, pa, pb);
}

template <int TYPE>
__global__ __launch_bounds__(64) void k_points_add(const u32* a, const u32* b, int n, int negate_b, u32* out) {
  using CV = typename EcType<TYPE>::CV;
  constexpr int PW = CurveIO<CV>::WIRE_JAC_WORDS;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  points_add_one<CV>(a + (size_t)PW * i, b + (size_t)PW * i, negate_b != 0, out + (size_t)PW * i);
}

// rows of at most EC_LONG terms, one per lane; the long rows are left to the three kernels below
template <int TYPE>
__global__ __launch_bounds__(64) void k_sparse_points(const u32* __restrict__ ptr, const u32* __restrict__ idx,
                                                      const u32* __restrict__ coeff, const u32* __restrict__ points,
                                                      int rows, u32* __restrict__ out) {
  using CV = typename EcType<TYPE>::CV;
  using IO = CurveIO<CV>;
  constexpr int PW = IO::WIRE_JAC_WORDS;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const u32 b = ptr[row], e = ptr[row + 1];
  if (e - b > (u32)EC_LONG) return;
  Jac<CV> acc = jac_infinity<CV>();
  for (u32 t = b; t < e; t++)
    acc = sparse_term<CV>(acc, points + (size_t)PW * idx[t], coeff ? coeff + (size_t)8 * t : nullptr);
  IO::template write<WireIn>(acc, out + (size_t)PW * row);
}
// lane l of long row lr sums the terms b + l, b + l + 4096, ... into part[lr * 4096 + l]
template <int TYPE>
__global__ __launch_bounds__(64) void k_sparse_points_long(const u32* __restrict__ ptr, const u32* __restrict__ idx,
                                                           const u32* __restrict__ coeff, const u32* __restrict__ points,
                                                           const u32* __restrict__ long_rows, u32* __restrict__ part) {
  using CV = typename EcType<TYPE>::CV;
  using IO = CurveIO<CV>;
  constexpr int PW = IO::WIRE_JAC_WORDS;
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lr = g / EC_LONG_LANES, l = g % EC_LONG_LANES;
  const u32 row = long_rows[lr];
  const u32 b = ptr[row], e = ptr[row + 1];
  Jac<CV> acc = jac_infinity<CV>();
  for (u32 t = b + l; t < e; t += EC_LONG_LANES)
    acc = sparse_term<CV>(acc, points + (size_t)PW * idx[t], coeff ? coeff + (size_t)8 * t : nullptr);
  IO::template write<WireIn>(acc, part + (size_t)PW * g);
}
// out[dest ? dest[g] : g] = the sum of in[64 g .. 64 g + 64), g < groups
template <int TYPE>
__global__ __launch_bounds__(64) void k_points_sum64(const u32* __restrict__ in, int groups, const u32* __restrict__ dest,
                                                     u32* __restrict__ out) {
  using CV = typename EcType<TYPE>::CV;
  using IO = CurveIO<CV>;
  constexpr int PW = IO::WIRE_JAC_WORDS;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  Jac<CV> acc = jac_infinity<CV>();
  for (int i = 0; i < 64; i++) acc = jac_madd<CV>(acc, IO::aff_from_wire(in + (size_t)PW * (64 * (size_t)g + i)));
  IO::template write<WireIn>(acc, out + (size_t)PW * (dest ? dest[g] : (u32)g));
}
#endif

}  // namespace ozk
