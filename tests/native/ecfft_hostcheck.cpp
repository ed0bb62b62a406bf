// Host build of the per-lane functions of the point kernels (octopuszk_amd/csrc/ec_fft.cuh): the
// twiddle and its recoding, the butterfly, the term of the sparse product and the pointwise sum, for
// tests/test_srs_setup_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _ecfft_hostcheck.so ecfft_hostcheck.cpp
#include "../../octopuszk_amd/csrc/ec_fft.cuh"
using namespace ozk;

static EcFftTwiddle twiddle_of(const u32* base, const u32* k) {
  EcFftTwiddle c;
  for (int i = 0; i < 8; i++) {
    c.base[i] = base[i];
    c.k[i] = k[i];
  }
  return c;
}
// out = k base^i mod r
extern "C" void efhc_twiddle(const u32* base, const u32* k, u32 i, u32* out) {
  u32 w[8];
  ecfft_twiddle(twiddle_of(base, k), i, w);
  for (int j = 0; j < 8; j++) out[j] = w[j];
}
// the schedule of k base^i: steps[0 .. len) least significant first; returns len
extern "C" int efhc_schedule(const u32* base, const u32* k, u32 i, int type, uint8_t* steps) {
  ScaleSchedule s;
  ecfft_schedule(twiddle_of(base, k), i, type == 1, s);
  for (int j = 0; j < s.len; j++) steps[j] = (uint8_t)scale_step(s, j);
  return s.len;
}
// (oa, ob) = ([ka] a + [kb] b, [ka] a - [kb] b); a null scalar is the factor 1
extern "C" void efhc_butterfly(const u32* a, const u32* b, int type, const u32* ka, const u32* kb, u32* oa, u32* ob) {
  const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ScaleSchedule sa, sb;
  if (ka) ecfft_schedule(twiddle_of(zero, ka), 0, type == 1, sa);
  if (kb) ecfft_schedule(twiddle_of(one, kb), 5, type == 1, sb);
  if (type == 1)
    ecfft_butterfly<G1Cfg, true>(a, b, ka ? &sa : nullptr, kb ? &sb : nullptr, oa, ob);
  else
    ecfft_butterfly<G2Cfg, false>(a, b, ka ? &sa : nullptr, kb ? &sb : nullptr, oa, ob);
}
extern "C" void efhc_add(const u32* a, const u32* b, int type, int negate_b, u32* out) {
  if (type == 1)
    points_add_one<G1Cfg>(a, b, negate_b != 0, out);
  else
    points_add_one<G2Cfg>(a, b, negate_b != 0, out);
}
template <class CV>
static void efhc_term_of(const u32* acc, const u32* p, const u32* c, u32* out) {
  using IO = CurveIO<CV>;
  IO::template write<WireIn>(sparse_term<CV>(from_affine<CV>(IO::aff_from_wire(acc)), p, c), out);
}
// out = acc + [c] p; c null: the coefficient one
extern "C" void efhc_term(const u32* acc, const u32* p, const u32* c, int type, u32* out) {
  if (type == 1)
    efhc_term_of<G1Cfg>(acc, p, c, out);
  else
    efhc_term_of<G2Cfg>(acc, p, c, out);
}
// out = the wire-in point `in` (any Z) read with aff_from_wire and written back with write<WireIn>
extern "C" void efhc_roundtrip(const u32* in, int type, u32* out) {
  if (type == 1)
    CurveIO<G1Cfg>::write<WireIn>(from_affine<G1Cfg>(CurveIO<G1Cfg>::aff_from_wire(in)), out);
  else
    CurveIO<G2Cfg>::write<WireIn>(from_affine<G2Cfg>(CurveIO<G2Cfg>::aff_from_wire(in)), out);
}
