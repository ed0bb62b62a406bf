// Host build of the decoders that turn a compressed point into the prepared records of the variable-base MSM
// (octopuszk_amd/csrc/point_codec.cuh) and of the conversion they must agree with (k_convert_bases,
// octopuszk_amd/csrc/msm_var.cuh): the same functions the kernels compile, for tests/test_keyfile_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _keyfile_hostcheck.so keyfile_hostcheck.cpp
#include "../../octopuszk_amd/csrc/point_codec.cuh"
using namespace ozk;

// in: 8 words -> out: record (x, y) | record (beta x, y), 16 words each; returns the code
extern "C" int kfhc_g1_decode_prepared(const u32* in, u32* out) {
  Aff<G1Cfg::EA> q, q2;
  const int code = codec_g1_decode_prepared(in, q, q2);
  CurveIO<G1Cfg>::store_aff(q, out);
  CurveIO<G1Cfg>::store_aff(q2, out + 16);
  return code;
}
// in: 16 words -> out: two records of 32 words
extern "C" int kfhc_g2_decode_prepared(const u32* in, u32* out) {
  Aff<G2Cfg::EA> q, q2;
  const int code = codec_g2_decode_prepared(in, q, q2);
  CurveIO<G2Cfg>::store_aff(q, out);
  CurveIO<G2Cfg>::store_aff(q2, out + 32);
  return code;
}
// What k_convert_bases (msm_var.cuh, a kernel: device only) writes for one wire-in point (24 / 48 words, any Z), by
// its own steps: Z = 0 the marker, else the affine coordinates into Montgomery form, canonical, and their image.
template <class CV>
static Aff<typename CV::EA> convert_base(const u32* p) {
  using IO = CurveIO<CV>;
  using EA = typename CV::EA;
  using ET = ElemTraits<EA>;
  Aff<EA> q;
  const EA X = ET::from_wire(p), Y = ET::from_wire(p + IO::CW), Z = ET::from_wire(p + 2 * IO::CW);
  if (is_zero(Z)) {
    q.x = EA(el_zero(q.x));
    q.y = EA(el_zero(q.x));
    return q;
  }
  const auto zi = inv(Z);
  const auto zi2 = sqr(zi);
  q.x = EA(canonical(mul(X, zi2)));
  q.y = EA(canonical(mul(Y, mul(zi2, zi))));
  return q;
}
extern "C" void kfhc_g1_convert(const u32* wire, u32* out) {
  const Aff<G1Cfg::EA> q = convert_base<G1Cfg>(wire), q2 = glv_image<G1Cfg>(q);
  CurveIO<G1Cfg>::store_aff(q, out);
  CurveIO<G1Cfg>::store_aff(q2, out + 16);
}
extern "C" void kfhc_g2_convert(const u32* wire, u32* out) {
  const Aff<G2Cfg::EA> q = convert_base<G2Cfg>(wire), q2 = glv_image<G2Cfg>(q);
  CurveIO<G2Cfg>::store_aff(q, out);
  CurveIO<G2Cfg>::store_aff(q2, out + 32);
}
// [r]q == O for one stored G2 record (32 words): the test k_codec_subgroup_g2 makes
extern "C" int kfhc_g2_in_subgroup(const u32* rec) {
  const Aff<G2Cfg::EA> q = CurveIO<G2Cfg>::load_aff(rec);
  return is_inf(q) || is_inf(scalar_mul<G2Cfg>(q, GlvConsts::R32, 8)) ? 1 : 0;
}
