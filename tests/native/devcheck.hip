// TEST INFRASTRUCTURE: the DEVICE branch of the arithmetic headers (fp29.cuh, fq2.cuh, ec.cuh, quad.cuh), which
// hostcheck.cpp cannot reach: the inline-asm Montgomery chains (mont_device / mont_sqr_col) and the lane-group group
// laws (quad.cuh DPP broadcasts, fq2.cuh lane pair / octet shuffles).  Compiled with the library's own hipcc flags
// (octopuszk_amd/build.py HIPCC_FLAGS), never linked into libozk_hip.so; driven by tests/test_device_arith_gpu.py.
//
// The record layout, the bound reports and the launcher are devcheck_common.h's (shared with towercheck.hip); this
// file holds the operation lists and the records of the one type only it uses (lane-pair Fq2); the records of points are
// devcheck_common.h's too.
#include "../../octopuszk_amd/csrc/fq2.cuh"
#include "devcheck_common.h"

namespace dc {
template <int B>
struct Bnd<Fe2L<B>> : Bnd<Fe2<B>> {};
template <int B>
struct Raw<Fe2L<B>> : RawFq2<Fe2L, B> {};
}  // namespace dc
using namespace dc;

namespace {

constexpr int SLACK = MONT_SLACK;
constexpr int isqrt_c(int v) {
  int r = 0;
  while ((r + 1) * (r + 1) <= v) r++;
  return r;
}
constexpr int SB = isqrt_c(SLACK * 256);   // the largest equal bounds a product admits
constexpr int SB2 = isqrt_c(SLACK * 128);  // ... two products of a dual product
constexpr int SB4 = isqrt_c(SLACK * 64);   // ... four

template <class P>
struct FieldOps {
  template <int B>
  using F = Fe<P, B>;
  template <int B, int L>
  using FL = FeL<P, B, L>;

  template <int B1, int B2>
  DC_OP(Mul, "mul", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) return mul(a0, a1);, F<B1>, F<B2>)
  template <int B>
  DC_OP(Sqr, "sqr", 1, DC_A(0, F<B>) return sqr(a0);, F<B>)
  template <int B1, int B2, int B3, int B4>
  DC_OP(Mul2, "mul2", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) DC_A(2, F<B3>) DC_A(3, F<B4>) return mul2(a0, a1, a2, a3);,
        F<B1>, F<B2>, F<B3>, F<B4>)
  template <int B1, int B2>
  DC_OP(Mul4, "mul4", 1,
        DC_A(0, F<B1>) DC_A(1, F<B2>) DC_A(2, F<B1>) DC_A(3, F<B2>) DC_A(4, F<B1>) DC_A(5, F<B2>) DC_A(6, F<B1>)
            DC_A(7, F<B2>) return mul4(a0, a1, a2, a3, a4, a5, a6, a7);,
        F<B1>, F<B2>, F<B1>, F<B2>, F<B1>, F<B2>, F<B1>, F<B2>)
  template <int B1, int B2, int B3, int B4>
  DC_OP(Mulsub, "mulsub", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) DC_A(2, F<B3>) DC_A(3, F<B4>) return mulsub(a0, a1, a2, a3);,
        F<B1>, F<B2>, F<B3>, F<B4>)
  template <int B1, int B2>
  DC_OP(Add, "add", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) return add(a0, a1);, F<B1>, F<B2>)
  template <int B>
  DC_OP(Dbl, "dbl", 1, DC_A(0, F<B>) return dbl(a0);, F<B>)
  template <int B1, int B2>
  DC_OP(Sub, "sub", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) return sub(a0, a1);, F<B1>, F<B2>)
  template <int B>
  DC_OP(Neg, "neg", 1, DC_A(0, F<B>) return neg(a0);, F<B>)
  template <int K, int B>
  struct Csub : OpBase<1, F<B>> {
    static constexpr const char* name = "csub";
    static constexpr int PARAM = K;
    static __device__ auto run(const u32* const* x) { return csub<K>(ld<F<B>>(x)); }
  };
  template <int TB, int B>
  DC_OP(ReduceTo, "reduce_to", 1, DC_A(0, F<B>) return reduce_to<TB>(a0);, F<B>)
  template <int B>
  DC_OP(ReduceQ, "reduce_q", 1, DC_A(0, F<B>) return reduce_q(a0);, F<B>)
  template <int B>
  DC_OP(Canonical, "canonical", 1, DC_A(0, F<B>) return canonical(a0);, F<B>)
  template <int B>
  DC_OP(CanonicalQ, "canonical_q", 1, DC_A(0, F<B>) return canonical_q(a0);, F<B>)
  DC_OP(Unpack, "unpack", 1, DC_A(0, Wire) return unpack<P>(a0.w);, Wire)
  template <int B>
  DC_OP(Pack, "pack", 1, DC_A(0, F<B>) Words w; pack(a0, w.w); return w;, F<B>)
  template <int B>
  DC_OP(Inv, "inv", 1, DC_A(0, F<B>) return inv(a0);, F<B>)
  template <int B>
  DC_OP(IsZero, "is_zero", 1, DC_A(0, F<B>) return is_zero(a0);, F<B>)
  template <int B1, int B2>
  DC_OP(Eq, "eq", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) return eq(a0, a1);, F<B1>, F<B2>)
  // ---- loose (FeL) forms
  template <int B1, int L1, int B2>
  DC_OP(MulL, "mul", 1, DC_A(0, FL<B1 COMMA L1>) DC_A(1, F<B2>) return mul(a0, a1);, FL<B1, L1>, F<B2>)
  template <int B1, int L1, int B2, int B3, int L3, int B4>
  DC_OP(Mul2L, "mul2", 1,
        DC_A(0, FL<B1 COMMA L1>) DC_A(1, F<B2>) DC_A(2, FL<B3 COMMA L3>) DC_A(3, F<B4>) return mul2(a0, a1, a2, a3);,
        FL<B1, L1>, F<B2>, FL<B3, L3>, F<B4>)
  template <int B1, int L1, int B2, int L2>
  DC_OP(MulLL, "mul", 1, DC_A(0, FL<B1 COMMA L1>) DC_A(1, FL<B2 COMMA L2>) return mul_ll(a0, a1);, FL<B1, L1>,
        FL<B2, L2>)
  template <int B1, int L1, int B2, int L2>
  DC_OP(Mul2LL, "mul2", 1,
        DC_A(0, FL<B1 COMMA L1>) DC_A(1, FL<B2 COMMA L2>) DC_A(2, FL<B1 COMMA L1>) DC_A(3, FL<B2 COMMA L2>) return mul2_ll(
            a0, a1, a2, a3);,
        FL<B1, L1>, FL<B2, L2>, FL<B1, L1>, FL<B2, L2>)
  template <int B1, int L1, int B2, int L2>
  DC_OP(Mul4LL, "mul4", 1,
        DC_A(0, FL<B1 COMMA L1>) DC_A(1, FL<B2 COMMA L2>) DC_A(2, FL<B1 COMMA L1>) DC_A(3, FL<B2 COMMA L2>)
            DC_A(4, FL<B1 COMMA L1>) DC_A(5, FL<B2 COMMA L2>) DC_A(6, FL<B1 COMMA L1>)
                DC_A(7, FL<B2 COMMA L2>) return mul4_ll(a0, a1, a2, a3, a4, a5, a6, a7);,
        FL<B1, L1>, FL<B2, L2>, FL<B1, L1>, FL<B2, L2>, FL<B1, L1>, FL<B2, L2>, FL<B1, L1>, FL<B2, L2>)
  template <int B, int L>
  DC_OP(Normalise, "normalise", 1, DC_A(0, FL<B COMMA L>) return normalise(a0);, FL<B, L>)
  template <int B1, int B2, int B3>
  DC_OP(SubSub2, "sub_sub2", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) DC_A(2, F<B3>) return sub_sub2(a0, a1, a2);, F<B1>,
        F<B2>, F<B3>)
  template <int B1, int B2>
  DC_OP(SubNc, "sub", 1, DC_A(0, F<B1>) DC_A(1, F<B2>) return sub_nc(a0, a1);, F<B1>, F<B2>)
  template <int B>
  DC_OP(NegNc, "neg", 1, DC_A(0, F<B>) return neg_nc(a0);, F<B>)
  template <int B1, int L1, int B2, int L2>
  DC_OP(AddNc, "add", 1, DC_A(0, FL<B1 COMMA L1>) DC_A(1, FL<B2 COMMA L2>) return add_nc(a0, a1);, FL<B1, L1>,
        FL<B2, L2>)
  template <int B, int L>
  DC_OP(DblNc, "dbl", 1, DC_A(0, FL<B COMMA L>) return dbl_nc(a0);, FL<B, L>)

  using List = TL<
      // products at the bounds the production call sites instantiate (G1Cfg / G2Cfg coordinates, quad.cuh's
      // levels 96 x 96, 116 x 116, 192 x 192, 96 x 20, 80 x 49, the FFT's twiddle x b1) and at the extreme the
      // static_assert admits (B1 B2 = MONT_SLACK x 256)
      Mul<16, 16>, Mul<17, 17>, Mul<17, 115>, Mul<96, 96>, Mul<116, 116>, Mul<192, 192>, Mul<96, 20>, Mul<80, 49>,
      Mul<16, 352>, Mul<SB, SB>, Mul<SLACK, 256>, Mul<640, SLACK * 256 / 640>, Sqr<17>, Sqr<32>, Sqr<96>, Sqr<116>, Sqr<192>,
      Sqr<SB>, Mul2<32, 32, 32, 32>, Mul2<96, 96, 96, 96>, Mul2<SB2, SB2, SB2, SB2>, Mul2<SLACK, 128, SLACK, 128>,
      Mul4<32, 32>, Mul4<SB4, SB4>, Mul4<SLACK, 64>, Mulsub<32, 32, 32, 32>, Mulsub<96, 64, 49, 96>,
      Mulsub<SB, SB, SB, SB>, Add<16, 16>, Add<94, 115>, Add<320, 320>, Dbl<17>, Dbl<320>, Sub<17, 17>, Sub<96, 94>,
      Sub<32, 607>, Neg<17>, Neg<94>, Neg<623>, Csub<1, 32>, Csub<4, 96>, Csub<20, 640>, ReduceTo<32, 640>,
      ReduceTo<17, 115>, ReduceTo<64, 352>, ReduceQ<85>, ReduceQ<352>, ReduceQ<640>, Canonical<17>, Canonical<640>,
      CanonicalQ<85>, CanonicalQ<640>, Unpack, Pack<16>, Pack<84>, Inv<17>, Inv<640>, IsZero<17>, IsZero<96>,
      IsZero<640>, Eq<17, 17>, Eq<96, 96>, Eq<304, 320>,
      // loose factors: the LU = 12 budget of one loose factor (alone and split over a dual product), the FFT's
      // uncarried factors (b1 < 2.5 x 2^30 = LU 10, LDS values < 1.5 x 2^30 = LU 6) and the LU products of 24
      MulL<SB, 12, SB>, MulL<640, 12, SLACK * 256 / 640>, MulL<320, 10, 16>, MulL<352, 6, 16>, MulL<96, 4, 17>,
      Mul2L<SB2, 6, SB2, SB2, 6, SB2>, Mul2L<112, 4, 17, 64, 8, 17>, MulLL<SB, 4, SB, 6>, MulLL<SB, 2, SB, 12>,
      Mul2LL<SB2, 4, SB2, 3>, Mul4LL<SB4, 2, SB4, 3>, Normalise<320, 15>, Normalise<640, 12>, SubSub2<32, 32, 32>,
      SubSub2<96, 200, 100>, SubNc<96, 94>, NegNc<94>, AddNc<192, 6, 192, 6>, DblNc<320, 6>,
      // is_zero at the bounds the group law of ec.cuh hands it H, rh, P, R, PP and Z / ZZ at over the base field
      // (DESIGN.md lists them; appended: the cases above are seeded by their index)
      IsZero<24>, IsZero<49>, IsZero<65>, IsZero<78>, IsZero<81>, IsZero<97>, IsZero<113>, IsZero<145>>;
};

// ---- Fq2 per lane, Fq2 on a lane pair, the G1 hot loop, the lane-quad G1 and lane-octet G2 group laws (Fq only)
template <int B1, int B2>
DC_OP(Fq2Mul, "fq2_mul", 1, DC_A(0, Fe2<B1>) DC_A(1, Fe2<B2>) return mul(a0, a1);, Fe2<B1>, Fe2<B2>)
template <int B>
DC_OP(Fq2Sqr, "fq2_sqr", 1, DC_A(0, Fe2<B>) return sqr(a0);, Fe2<B>)
template <int B1, int B2>
DC_OP(Fq2MulLz, "fq2_mul", 1, DC_A(0, Fe2<B1>) DC_A(1, Fe2<B2>) return mul_lz(a0, a1);, Fe2<B1>, Fe2<B2>)
template <int B>
DC_OP(Fq2SqrLz, "fq2_sqr", 1, DC_A(0, Fe2<B>) return sqr_lz(a0);, Fe2<B>)
template <int B1, int B2, int B3, int B4>
DC_OP(Fq2MulsubLz, "fq2_mulsub", 1,
      DC_A(0, Fe2<B1>) DC_A(1, Fe2<B2>) DC_A(2, Fe2<B3>) DC_A(3, Fe2<B4>) return mulsub_lz(a0, a1, a2, a3);, Fe2<B1>,
      Fe2<B2>, Fe2<B3>, Fe2<B4>)
template <int B1, int B2, int B3>
DC_OP(Fq2SubSub2, "fq2_sub_sub2", 1, DC_A(0, Fe2<B1>) DC_A(1, Fe2<B2>) DC_A(2, Fe2<B3>) return sub_sub2(a0, a1, a2);,
      Fe2<B1>, Fe2<B2>, Fe2<B3>)
template <int B1, int B2>
DC_OP(Fq2PairMul, "fq2_mul", 2, DC_A(0, Fe2L<B1>) DC_A(1, Fe2L<B2>) return mul(a0, a1);, Fe2L<B1>, Fe2L<B2>)
template <int B>
DC_OP(Fq2PairSqr, "fq2_sqr", 2, DC_A(0, Fe2L<B>) return sqr(a0);, Fe2L<B>)
// the forms the pairing tower (fq12.cuh) instantiates beside the products
template <int B>
DC_OP(Fq2Scale, "fq2_scale", 1, DC_A(0, Fe2<B>) DC_A(1, Fe<FqParams COMMA 16>) return scale(a0, a1);, Fe2<B>,
      Fe<FqParams, 16>)
template <int B>
DC_OP(Fq2Inv, "fq2_inv", 1, DC_A(0, Fe2<B>) return inv(a0);, Fe2<B>)
template <int B>
DC_OP(Fq2IsZero, "fq2_is_zero", 1, DC_A(0, Fe2<B>) return is_zero(a0);, Fe2<B>)
template <int TB, int B>
DC_OP(Fq2ReduceTo, "fq2_reduce_to", 1, DC_A(0, Fe2<B>) return reduce_to<TB>(a0);, Fe2<B>)
DC_OP(G1MaddLazy, "g1_xyzz_madd", 1,
      DC_A(0, Xyzz<G1Cfg>) DC_A(1, Aff<G1Cfg::EA>) DC_A(2, Flag) return xyzz_madd_lazy(a0, a1, a2.v);, Xyzz<G1Cfg>,
      Aff<G1Cfg::EA>, Flag)
DC_OP(G1QuadDbl, "g1_jac_dbl", 4, DC_A(0, Jac<G1CfgQ>) return jac_dbl(a0);, Jac<G1CfgQ>)
DC_OP(G1QuadAdd, "g1_jac_add", 4, DC_A(0, Jac<G1CfgQ>) DC_A(1, Jac<G1CfgQ>) return jac_add(a0, a1);, Jac<G1CfgQ>,
      Jac<G1CfgQ>)
DC_OP(G2OctetDbl, "g2_jac_dbl", 8, DC_A(0, Jac<G2CfgO>) return jac_dbl(a0);, Jac<G2CfgO>)
DC_OP(G2OctetAdd, "g2_jac_add", 8, DC_A(0, Jac<G2CfgO>) DC_A(1, Jac<G2CfgO>) return jac_add(a0, a1);, Jac<G2CfgO>,
      Jac<G2CfgO>)

using ExtList = TL<Fq2Mul<32, 32>, Fq2Mul<144, 112>, Fq2Mul<176, 80>, Fq2Sqr<32>, Fq2Sqr<176>, Fq2MulLz<17, 32>,
                   Fq2MulLz<144, 32>, Fq2SqrLz<32>, Fq2MulsubLz<32, 32, 80, 32>, Fq2MulsubLz<32, 32, 80, 17>,
                   Fq2SubSub2<32, 32, 32>, Fq2SubSub2<32, 32, 17>, Fq2PairMul<32, 32>, Fq2PairMul<112, 32>,
                   Fq2PairMul<144, 32>, Fq2PairSqr<32>, Fq2PairSqr<112>, G1MaddLazy, G1QuadDbl, G1QuadAdd, G2OctetDbl,
                   G2OctetAdd,
                   // the tower's Fq2 instantiations (appended: the cases above are seeded by their index)
                   Fq2Mul<32, 64>, Fq2Mul<32, 80>, Fq2Mul<64, 64>, Fq2Scale<32>, Fq2Scale<64>, Fq2Inv<32>,
                   Fq2IsZero<32>, Fq2IsZero<80>, Fq2ReduceTo<32, 64>, Fq2ReduceTo<32, 112>,
                   // ... and the group law's over Fq2 (G2Cfg): the affine coordinates, Z, R, rh, H, P (appended)
                   Fq2IsZero<17>, Fq2IsZero<112>, Fq2IsZero<128>, Fq2IsZero<160>, Fq2IsZero<192>, Fq2IsZero<224>>;

}  // namespace

// field: 0 = Fq, 1 = Fr, 2 = Fq2 / group-law code over Fq.  Returns the number of operations of that list.
extern "C" int dc_count(int field) {
  return field == 0 ? Nth<FieldOps<FqParams>::List>::N
                    : field == 1 ? Nth<FieldOps<FrParams>::List>::N : field == 2 ? Nth<ExtList>::N : 0;
}
// name: at least 32 bytes; v: at least 4 + 4 * 16 ints
extern "C" int dc_info(int field, int idx, char* name, int* v) {
  if (field == 0) return info<FieldOps<FqParams>::List>(idx, name, v);
  if (field == 1) return info<FieldOps<FrParams>::List>(idx, name, v);
  if (field == 2) return info<ExtList>(idx, name, v);
  return -1;
}
// in: NIN x n records of 9 words, out: n x NOUT records of 9 words, both device buffers; n a multiple of the group
extern "C" int dc_run(int field, int idx, const void* in, void* out, int n, void* stream) {
  const hipStream_t s = (hipStream_t)stream;
  constexpr int BLOCK = 256, LB = 1024;  // 256 lanes per block, no launch bound below the compiler's default
  if (n <= 0) return -3;
  if (field == 0) return launch<FieldOps<FqParams>::List, LB>(idx, (const u32*)in, (u32*)out, nullptr, n, BLOCK, s);
  if (field == 1) return launch<FieldOps<FrParams>::List, LB>(idx, (const u32*)in, (u32*)out, nullptr, n, BLOCK, s);
  if (field == 2) return launch<ExtList, LB>(idx, (const u32*)in, (u32*)out, nullptr, n, BLOCK, s);
  return -1;
}
// the constants the input builders need from the headers: MONT_SLACK, FE_MAXK
extern "C" int dc_const(int which) { return which == 0 ? MONT_SLACK : which == 1 ? FE_MAXK : -1; }
