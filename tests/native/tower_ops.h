// TEST INFRASTRUCTURE: the operation table of the pairing-tower conformance harness, written once and compiled twice:
// by hipcc into towercheck.hip (one kernel per operation, the DEVICE build of fq12.cuh: __noinline__ tower functions,
// arguments through the private stack) and by g++ into towercheck_host.cpp (the host branch, no GPU needed).
// Every operation goes through its production entry point; tests/towerarith.py holds the cases and expectations.
//
// Include after fq12.cuh / batch_verify.cuh and devcheck_common.h.
#pragma once

namespace dc {

// ---- records of the tower's types: their Fq components in the GT wire order, nine raw limbs each
template <>
struct Bnd<Fe6> : Bnd<Pair2<F2, Pair2<F2, F2>>> {};
template <>
struct Bnd<Fe12> : Bnd<Pair2<Fe6, Fe6>> {};
template <>
struct Bnd<Ell> : Bnd<Pair2<F2, Pair2<F2, F2>>> {};      // ell0, ellVW, ellVV
template <>
struct Bnd<G2Proj> : Bnd<Pair2<F2, Pair2<F2, F2>>> {};   // X, Y, Z
template <>
struct Raw<Fe6> {
  static DC_FN Fe6 ld(const u32* const* x) { return Fe6{Raw<F2>::ld(x), Raw<F2>::ld(x + 2), Raw<F2>::ld(x + 4)}; }
  static DC_FN void st(const Fe6& v, u32* o) {
    Raw<F2>::st(v.c0, o);
    Raw<F2>::st(v.c1, o + 18);
    Raw<F2>::st(v.c2, o + 36);
  }
};
template <>
struct Raw<Fe12> {
  static DC_FN Fe12 ld(const u32* const* x) { return Fe12{Raw<Fe6>::ld(x), Raw<Fe6>::ld(x + 6)}; }
  static DC_FN void st(const Fe12& v, u32* o) {
    Raw<Fe6>::st(v.c0, o);
    Raw<Fe6>::st(v.c1, o + 54);
  }
};
template <>
struct Raw<Ell> {
  static DC_FN Ell ld(const u32* const* x) { return Ell{Raw<F2>::ld(x), Raw<F2>::ld(x + 2), Raw<F2>::ld(x + 4)}; }
  static DC_FN void st(const Ell& v, u32* o) {
    Raw<F2>::st(v.ell0, o);
    Raw<F2>::st(v.ellVW, o + 18);
    Raw<F2>::st(v.ellVV, o + 36);
  }
};
template <>
struct Raw<G2Proj> {
  static DC_FN G2Proj ld(const u32* const* x) { return G2Proj{Raw<F2>::ld(x), Raw<F2>::ld(x + 2), Raw<F2>::ld(x + 4)}; }
  static DC_FN void st(const G2Proj& v, u32* o) {
    Raw<F2>::st(v.X, o);
    Raw<F2>::st(v.Y, o + 18);
    Raw<F2>::st(v.Z, o + 36);
  }
};
// a GT wire value: 96 words as twelve records of eight (B = -1 out, B = -2 in)
struct Words12 {
  u32 w[96];
};
struct Wire12 {
  u32 w[96];
};
template <>
struct Bnd<Words12> {
  static constexpr int N = 12;
  static void get(int* b, int* l) {
    for (int k = 0; k < 12; k++) b[k] = -1, l[k] = 0;
  }
};
template <>
struct Bnd<Wire12> {
  static constexpr int N = 12;
  static void get(int* b, int* l) {
    for (int k = 0; k < 12; k++) b[k] = -2, l[k] = 0;
  }
};
template <>
struct Raw<Words12> {
  static DC_FN void st(const Words12& v, u32* o) {
    for (int k = 0; k < 12; k++) {
      for (int i = 0; i < 8; i++) o[9 * k + i] = v.w[8 * k + i];
      o[9 * k + 8] = 0;
    }
  }
};
template <>
struct Raw<Wire12> {
  static DC_FN Wire12 ld(const u32* const* x) {
    Wire12 r;
    for (int k = 0; k < 12; k++)
      for (int i = 0; i < 8; i++) r.w[8 * k + i] = x[k][i];
    return r;
  }
};
// (an exponent of W little-endian words: devcheck_common.h's Expo<W>)

}  // namespace dc

namespace tc {
using namespace dc;
using Fq32 = Fe<FqParams, 32>;
using StepOut = Pair2<Ell, G2Proj>;   // a line step's two results: the line, then the updated point
using F2Pair = Pair2<F2, F2>;

#define TC_OP(ID, NAME, ARGS, ...) DC_OP_HD(ID, NAME, 1, ARGS, __VA_ARGS__)
// the same with a template parameter reported as PARAM
#define TC_OPK(ID, NAME, K, ARGS, ...)                                                \
  struct ID : OpBase<1, __VA_ARGS__> {                                               \
    static constexpr const char* name = NAME;                                        \
    static constexpr int PARAM = K;                                                  \
    static DC_FN auto run(const u32* const* x) {                                     \
      int off[8];                                                                    \
      OpBase<1, __VA_ARGS__>::offsets(off);                                          \
      ARGS                                                                           \
    }                                                                                \
  };

// ---- the Fq2 helpers of fq12.cuh
TC_OP(MulXi, "mul_xi", DC_A(0, F2) return mul_xi(a0);, F2)
TC_OP(F2Conj, "f2_conj", DC_A(0, F2) return f2_conj(a0);, F2)
TC_OP(F2Neg, "f2_neg", DC_A(0, F2) return f2_neg(a0);, F2)
TC_OP(F2Add, "f2_add", DC_A(0, F2) DC_A(1, F2) return f2_add(a0, a1);, F2, F2)
TC_OP(F2Sub, "f2_sub", DC_A(0, F2) DC_A(1, F2) return f2_sub(a0, a1);, F2, F2)
template <int B>
TC_OPK(F2n, "f2n", B, DC_A(0, Fe2<B>) return f2n(a0);, Fe2<B>)

// ---- Fq6
TC_OP(F6Add, "f6_add", DC_A(0, Fe6) DC_A(1, Fe6) return add(a0, a1);, Fe6, Fe6)
TC_OP(F6Sub, "f6_sub", DC_A(0, Fe6) DC_A(1, Fe6) return sub(a0, a1);, Fe6, Fe6)
TC_OP(F6Neg, "f6_neg", DC_A(0, Fe6) return neg(a0);, Fe6)
TC_OP(F6Mul, "f6_mul", DC_A(0, Fe6) DC_A(1, Fe6) return mul(a0, a1);, Fe6, Fe6)
TC_OP(F6MulF2, "f6_mul_f2", DC_A(0, Fe6) DC_A(1, F2) return mul(a0, a1);, Fe6, F2)
TC_OP(F6Sqr, "f6_sqr", DC_A(0, Fe6) return sqr(a0);, Fe6)
TC_OP(F6Inv, "f6_inv", DC_A(0, Fe6) return inv(a0);, Fe6)
template <int K>
TC_OPK(F6Frob, "f6_frobenius", K, DC_A(0, Fe6) return frobenius<K>(a0);, Fe6)
TC_OP(F6MulByV, "f6_mul_by_v", DC_A(0, Fe6) return mul_by_v(a0);, Fe6)
TC_OP(F6IsZero, "f6_is_zero", DC_A(0, Fe6) return is_zero(a0);, Fe6)

// ---- Fq12
TC_OP(F12Mul, "f12_mul", DC_A(0, Fe12) DC_A(1, Fe12) return mul(a0, a1);, Fe12, Fe12)
TC_OP(F12Sqr, "f12_sqr", DC_A(0, Fe12) return sqr(a0);, Fe12)
TC_OP(F12Inv, "f12_inv", DC_A(0, Fe12) return inv(a0);, Fe12)
TC_OP(F12Conj, "f12_conj", DC_A(0, Fe12) return conj(a0);, Fe12)
template <int K>
TC_OPK(F12Frob, "f12_frobenius", K, DC_A(0, Fe12) return frobenius<K>(a0);, Fe12)
TC_OP(F12CycSqr, "f12_cyclotomic_sqr", DC_A(0, Fe12) return cyclotomic_sqr(a0);, Fe12)
// operands in mulBy024's order: ell0, ellVW, ellVV
TC_OP(F12MulBy024, "f12_mul_by_024", DC_A(0, Fe12) DC_A(1, F2) DC_A(2, F2) DC_A(3, F2) return mul_by_024(a0, a1, a2, a3);,
      Fe12, F2, F2, F2)
TC_OP(F12IsZero, "f12_is_zero", DC_A(0, Fe12) return is_zero(a0);, Fe12)
TC_OP(F12Eq, "f12_eq", DC_A(0, Fe12) DC_A(1, Fe12) return f12_eq(a0, a1);, Fe12, Fe12)
TC_OP(ExpByNegZ, "exp_by_neg_z", DC_A(0, Fe12) return exp_by_neg_z(a0);, Fe12)
TC_OP(FinalFirst, "final_exp_first_chunk", DC_A(0, Fe12) return final_exp_first_chunk(a0);, Fe12)
TC_OP(FinalLast, "final_exp_last_chunk", DC_A(0, Fe12) return final_exp_last_chunk(a0);, Fe12)
TC_OP(FinalExp, "final_exponentiation", DC_A(0, Fe12) return final_exponentiation(a0);, Fe12)
template <int W>
TC_OPK(GtPow, "gt_pow", W, DC_A(0, Fe12) DC_A(1, Expo<W>) return gt_pow(a0, a1.w, W);, Fe12, Expo<W>)

// ---- steps of the Miller loop
TC_OP(DoublingStep, "doubling_step", DC_A(0, G2Proj) StepOut r; r.b = a0; r.a = doubling_step(r.b);
      return r;, G2Proj)
TC_OP(MixedAdditionStep, "mixed_addition_step",
      DC_A(0, F2) DC_A(1, F2) DC_A(2, G2Proj) StepOut r; r.b = a2; r.a = mixed_addition_step(a0, a1, r.b);
      return r;, F2, F2, G2Proj)
TC_OP(MulByQ, "mul_by_q", DC_A(0, F2) DC_A(1, F2) F2Pair r; r.a = a0; r.b = a1; mul_by_q(r.a, r.b); return r;,
      F2, F2)
TC_OP(ApplyLine, "apply_line", DC_A(0, Fe12) DC_A(1, Ell) DC_A(2, Fq32) DC_A(3, Fq32) return apply_line(a0, a1, a2, a3);,
      Fe12, Ell, Fq32, Fq32)

// ---- storage
// store_f12 then load_f12 through a lane-interleaved array: element w of lane i at scratch[w * lanes + i]
struct StoreLoad : OpBase<1, Fe12> {
  static constexpr const char* name = "store_load_f12";
  static constexpr int SCRATCH = FE12_WORDS;
  static DC_FN Fe12 run(const u32* const* x, u32* slot, int lanes) {
    store_f12(ld<Fe12>(x), slot, lanes);
    return load_f12(slot, lanes);
  }
};
TC_OP(F12ToWire, "f12_to_wire", DC_A(0, Fe12) Words12 w; f12_to_wire(a0, w.w); return w;, Fe12)
TC_OP(F12FromWire, "f12_from_wire", DC_A(0, Wire12) return f12_from_wire(a0.w);, Wire12)

using List = TL<MulXi, F2Conj, F2Neg, F2Add, F2Sub, F2n<49>, F2n<80>, F2n<96>, F2n<112>, F2n<128>, F2n<144>, F2n<176>,
                F2n<288>, F6Add, F6Sub, F6Neg, F6Mul, F6MulF2, F6Sqr, F6Inv, F6Frob<1>, F6Frob<2>, F6Frob<3>, F6MulByV,
                F6IsZero, F12Mul, F12Sqr, F12Inv, F12Conj, F12Frob<1>, F12Frob<2>, F12Frob<3>, F12CycSqr, F12MulBy024,
                F12IsZero, F12Eq, ExpByNegZ, FinalFirst, FinalLast, FinalExp, GtPow<4>, GtPow<8>, DoublingStep,
                MixedAdditionStep, MulByQ, ApplyLine, StoreLoad, F12ToWire, F12FromWire>;

}  // namespace tc
