// TEST INFRASTRUCTURE: the operation table of the group-law conformance harness, written once and compiled twice: by
// hipcc into groupcheck.hip (one kernel per operation: the DEVICE branch of fp29.cuh under ec.cuh's large inlined
// functions) and by g++ into groupcheck_host.cpp (the host branch, no GPU needed).  Every operation goes through its
// production entry point; tests/grouparith.py holds the cases and the exact expectations.
//
// Four lists: 0 the per-lane group law over G1Cfg, 1 the same over G2Cfg (Fe2 coordinates, two records each), 2 what
// belongs to no curve (the GLV split), 3 the lane-group conversions of quad.cuh / fq2.cuh, which exist on the device
// only (the host build reports that list empty).  An operation is listed for a configuration only if production
// instantiates it there: jac_to_xyzz (the row / column window sums) and the lazily carried forms (CV::LAZY_MADD) are
// G1's alone; scalar_mul is called with 8 words everywhere and with 4 words for G1 by batch_verify.cuh.
//
// Include after fq2.cuh, glv.cuh and devcheck_common.h.
#pragma once

namespace gc {
using namespace dc;

#define GC_OP(ID, NAME, ARGS, ...) DC_OP_HD(ID, NAME, 1, ARGS, __VA_ARGS__)

template <class CV>
struct GroupOps {
  using A = Aff<typename CV::EA>;
  using J = Jac<CV>;
  using X = Xyzz<CV>;

  GC_OP(FromAffine, "from_affine", DC_A(0, A) return from_affine<CV>(a0);, A)
  GC_OP(XyzzFromAffine, "xyzz_from_affine", DC_A(0, A) return xyzz_from_affine<CV>(a0);, A)
  GC_OP(IsInfAff, "is_inf_aff", DC_A(0, A) return is_inf(a0);, A)
  GC_OP(IsInfJac, "is_inf_jac", DC_A(0, J) return is_inf(a0);, J)
  GC_OP(IsInfXyzz, "is_inf_xyzz", DC_A(0, X) return is_inf(a0);, X)
  GC_OP(JacDbl, "jac_dbl", DC_A(0, J) return jac_dbl<CV>(a0);, J)
  GC_OP(JacAdd, "jac_add", DC_A(0, J) DC_A(1, J) return jac_add<CV>(a0, a1);, J, J)
  GC_OP(JacMadd, "jac_madd", DC_A(0, J) DC_A(1, A) return jac_madd<CV>(a0, a1);, J, A)
  GC_OP(AffDbl, "aff_dbl", DC_A(0, A) return aff_dbl<CV>(a0);, A)
  GC_OP(JacNeg, "jac_neg", DC_A(0, J) return jac_neg<CV>(a0);, J)
  GC_OP(XyzzDblAffine, "xyzz_dbl_affine", DC_A(0, A) return xyzz_dbl_affine<CV>(a0);, A)
  GC_OP(XyzzMadd, "xyzz_madd", DC_A(0, X) DC_A(1, A) return xyzz_madd<CV>(a0, a1);, X, A)
  GC_OP(XyzzDbl, "xyzz_dbl", DC_A(0, X) return xyzz_dbl<CV>(a0);, X)
  GC_OP(XyzzAdd, "xyzz_add", DC_A(0, X) DC_A(1, X) return xyzz_add<CV>(a0, a1);, X, X)
  GC_OP(XyzzToJac, "xyzz_to_jac", DC_A(0, X) return xyzz_to_jac<CV>(a0);, X)
  GC_OP(GlvImage, "glv_image", DC_A(0, A) return glv_image<CV>(a0);, A)
  template <int W>
  struct ScalarMul : OpBase<1, A, Expo<W>> {
    static constexpr const char* name = "scalar_mul";
    static constexpr int PARAM = W;
    static DC_FN auto run(const u32* const* x) {
      int off[8];
      OpBase<1, A, Expo<W>>::offsets(off);
      DC_A(0, A) DC_A(1, Expo<W>) return scalar_mul<CV>(a0, a1.w, W);
    }
  };
  // ---- the base-field forms (lazily carried; CV::LAZY_MADD) and the conversion only the G1 window sums take
  GC_OP(XyzzMaddLazy, "xyzz_madd_lazy", DC_A(0, X) DC_A(1, A) DC_A(2, Flag) return xyzz_madd_lazy<CV>(a0, a1, a2.v);, X,
        A, Flag)
  GC_OP(XyzzFromAffineSigned, "xyzz_from_affine_signed",
        DC_A(0, A) DC_A(1, Flag) return xyzz_from_affine_signed<CV>(a0, a1.v);, A, Flag)
  GC_OP(XyzzAddAffine2Lazy, "xyzz_add_affine2_lazy",
        DC_A(0, X) DC_A(1, A) DC_A(2, Flag) return xyzz_add_affine2_lazy<CV>(a0, a1, a2.v);, X, A, Flag)
  GC_OP(JacToXyzz, "jac_to_xyzz", DC_A(0, J) return jac_to_xyzz<CV>(a0);, J)

  template <class... More>
  using Common = TL<FromAffine, XyzzFromAffine, IsInfAff, IsInfJac, IsInfXyzz, JacDbl, JacAdd, JacMadd, AffDbl, JacNeg,
                    XyzzDblAffine, XyzzMadd, XyzzDbl, XyzzAdd, XyzzToJac, GlvImage, ScalarMul<8>, More...>;
};

using G1 = GroupOps<G1Cfg>;
using G2 = GroupOps<G2Cfg>;
using G1List = G1::Common<G1::ScalarMul<4>, G1::XyzzMaddLazy, G1::XyzzFromAffineSigned, G1::XyzzAddAffine2Lazy,
                          G1::JacToXyzz>;
using G2List = G2::Common<>;

// the digit kernel's split: one wire scalar in; k1 | k2 (four words each) as one record, then the two sign flags
using SplitOut = Pair2<Words, Pair2<Flag, Flag>>;
GC_OP(GlvDecompose, "glv_decompose", DC_A(0, Wire) SplitOut r; u32 k1[4]; u32 k2[4];
      glv_decompose(a0.w, k1, r.b.a.v, k2, r.b.b.v);
      for (int i = 0; i < 4; i++) { r.a.w[i] = k1[i]; r.a.w[4 + i] = k2[i]; }
      return r;, Wire)
using MiscList = TL<GlvDecompose>;

#if defined(__HIPCC__)
// to_pair then from_pair of the serial chains' lane groups: every lane of the group holds the case and must return the
// same point (compared as an affine point, and bit for bit between the lanes and the copies; the group size as in
// devcheck.hip's quad and octet operations).  All lanes of a group hold the SAME case, so a from_pair that took the
// right limbs from the wrong lane of its own group would pass: only a read across groups is caught here, and the
// lane assignment inside a group is left to the kernel tests of the serial chains.
DC_OP(G1QuadRoundTrip, "g1_pair_round_trip", 4, DC_A(0, Jac<G1Cfg>) return from_pair(to_pair(a0));, Jac<G1Cfg>)
DC_OP(G2OctetRoundTrip, "g2_pair_round_trip", 8, DC_A(0, Jac<G2Cfg>) return from_pair(to_pair(a0));, Jac<G2Cfg>)
// ... and through one doubling of the lane group against the per-lane doubling's point
DC_OP(G1QuadDblVia, "g1_pair_dbl", 4, DC_A(0, Jac<G1Cfg>) return from_pair(jac_dbl(to_pair(a0)));, Jac<G1Cfg>)
DC_OP(G2OctetDblVia, "g2_pair_dbl", 8, DC_A(0, Jac<G2Cfg>) return from_pair(jac_dbl(to_pair(a0)));, Jac<G2Cfg>)
using LaneList = TL<G1QuadRoundTrip, G2OctetRoundTrip, G1QuadDblVia, G2OctetDblVia>;
#else
using LaneList = TL<>;
#endif

template <class F>
auto by_list(int list, F&& f) -> decltype(f(G1List())) {
  if (list == 0) return f(G1List());
  if (list == 1) return f(G2List());
  if (list == 2) return f(MiscList());
  if (list == 3) return f(LaneList());
  return -1;
}

}  // namespace gc
