// TEST INFRASTRUCTURE shared by the device conformance harnesses (devcheck.hip: fp29 / fq2 / ec / quad; towercheck.hip
// and towercheck_host.cpp: the pairing tower; groupcheck.hip and groupcheck_host.cpp: the group law).  Include it after
// the arithmetic headers under test (fq2.cuh at least: the records of Fe2 and of the points of ec.cuh are here).
//
// Every operation is a struct: `In` lists its operand types, run() applies it.  Each lane reads its operands as raw
// 9-limb records (operand k of lane i at in[(k * n + i) * 9]), applies the operation once and writes the raw limbs
// of every output element (out[(i * NOUT + j) * 9]).  info() reports each operand's and each output's bound from
// the C++ types themselves (decltype of run()), so the tests check what the type claims, not a copy of it.
//
// The record and bound machinery compiles for the host too (plain g++), so that a harness can run one operation
// table through both branches of the headers; k_op and launch exist under hipcc only.
#pragma once
#include <string.h>
#include <type_traits>

#if defined(__HIPCC__)
#define DC_FN __host__ __device__
#else
#define DC_FN
#endif

namespace dc {
using namespace ozk;

// ---- bounds of a type: element count, and per element (value bound in sixteenths of p, limb bound LU in units of
// 2^28; LU 2 = normalised).  Special kinds: B = 0 a bool (word 0), B = -1 eight packed words, B = -2 a wire operand,
// B = -3 an exponent or scalar of LU words.
struct Wire {
  u32 w[8];
};
struct Words {
  u32 w[8];
};
struct Flag {
  bool v;
};
template <class T>
struct Bnd;
template <class P, int B>
struct Bnd<Fe<P, B>> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = B, l[0] = 2; }
};
template <class P, int B, int L>
struct Bnd<FeL<P, B, L>> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = B, l[0] = L; }
};
template <int B>
struct Bnd<Fe2<B>> {
  static constexpr int N = 2;
  static void get(int* b, int* l) { b[0] = b[1] = B, l[0] = l[1] = 2; }
};
template <>
struct Bnd<bool> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = 0, l[0] = 0; }
};
template <>
struct Bnd<Flag> : Bnd<bool> {};
template <>
struct Bnd<Words> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = -1, l[0] = 0; }
};
template <>
struct Bnd<Wire> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = -2, l[0] = 0; }
};
template <class A, class B>
struct Pair2 {  // two elements written one after the other (a point's coordinates, an operation's two results)
  A a;
  B b;
};
template <class A, class B>
struct Bnd<Pair2<A, B>> {
  static constexpr int N = Bnd<A>::N + Bnd<B>::N;
  static void get(int* b, int* l) {
    Bnd<A>::get(b, l);
    Bnd<B>::get(b + Bnd<A>::N, l + Bnd<A>::N);
  }
};

template <class... T>
struct TL {
  static constexpr int N = (0 + ... + Bnd<T>::N);
  static void get(int* b, int* l) {
    int k = 0;
    ((Bnd<T>::get(b + k, l + k), k += Bnd<T>::N), ...);
  }
};

// ---- raw record <-> typed value
template <class T>
struct Raw;
template <class P, int B>
struct Raw<Fe<P, B>> {
  static DC_FN Fe<P, B> ld(const u32* const* x) {
    Fe<P, B> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = x[0][i];
    return r;
  }
  static DC_FN void st(const Fe<P, B>& v, u32* o) {
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = v.l[i];
  }
};
template <class P, int B, int L>
struct Raw<FeL<P, B, L>> {
  static DC_FN FeL<P, B, L> ld(const u32* const* x) {
    FeL<P, B, L> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = x[0][i];
    return r;
  }
  static DC_FN void st(const FeL<P, B, L>& v, u32* o) {
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = v.l[i];
  }
};
template <template <int> class E, int B>
struct RawFq2 {
  static DC_FN E<B> ld(const u32* const* x) {
    E<B> r;
    r.c0 = Raw<Fe<FqParams, B>>::ld(x);
    r.c1 = Raw<Fe<FqParams, B>>::ld(x + 1);
    return r;
  }
  static DC_FN void st(const E<B>& v, u32* o) {
    Raw<Fe<FqParams, B>>::st(v.c0, o);
    Raw<Fe<FqParams, B>>::st(v.c1, o + 9);
  }
};
template <int B>
struct Raw<Fe2<B>> : RawFq2<Fe2, B> {};
template <>
struct Raw<bool> {
  static DC_FN void st(bool v, u32* o) {
    o[0] = v ? 1u : 0u;
#pragma unroll
    for (int i = 1; i < 9; i++) o[i] = 0;
  }
};
template <>
struct Raw<Flag> {
  static DC_FN Flag ld(const u32* const* x) { return Flag{x[0][0] != 0}; }
  static DC_FN void st(const Flag& v, u32* o) { Raw<bool>::st(v.v, o); }
};
template <>
struct Raw<Words> {
  static DC_FN void st(const Words& v, u32* o) {
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = v.w[i];
    o[8] = 0;
  }
};
template <>
struct Raw<Wire> {
  static DC_FN Wire ld(const u32* const* x) {
    Wire r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.w[i] = x[0][i];
    return r;
  }
};
template <class A, class B>
struct Raw<Pair2<A, B>> {
  static DC_FN void st(const Pair2<A, B>& v, u32* o) {
    Raw<A>::st(v.a, o);
    Raw<B>::st(v.b, o + 9 * Bnd<A>::N);
  }
};

// an exponent or scalar of W little-endian words (B = -3, the LU slot holds W)
template <int W>
struct Expo {
  u32 w[8];
};
template <int W>
struct Bnd<Expo<W>> {
  static constexpr int N = 1;
  static void get(int* b, int* l) { b[0] = -3, l[0] = W; }
};
template <int W>
struct Raw<Expo<W>> {
  static DC_FN Expo<W> ld(const u32* const* x) {
    Expo<W> r;
    for (int i = 0; i < 8; i++) r.w[i] = x[0][i];
    return r;
  }
};

// ---- points (ec.cuh): the coordinates one after the other, each with as many records as its field has components
// (one over Fq, two over Fq2 and over the lane-pair Fq2 of the octet code)
template <class CV>
struct Bnd<Jac<CV>> : Bnd<Pair2<typename CV::EX, Pair2<typename CV::EY, typename CV::EZ>>> {};
template <class CV>
struct Bnd<Xyzz<CV>>
    : Bnd<Pair2<typename CV::XX, Pair2<typename CV::XY, Pair2<typename CV::XZZ, typename CV::XZZZ>>>> {};
template <class EA>
struct Bnd<Aff<EA>> : Bnd<Pair2<EA, EA>> {};
template <class CV>
struct Raw<Jac<CV>> {
  static constexpr int NX = Bnd<typename CV::EX>::N, NY = Bnd<typename CV::EY>::N;
  static DC_FN Jac<CV> ld(const u32* const* x) {
    Jac<CV> r;
    r.X = Raw<typename CV::EX>::ld(x);
    r.Y = Raw<typename CV::EY>::ld(x + NX);
    r.Z = Raw<typename CV::EZ>::ld(x + NX + NY);
    return r;
  }
  static DC_FN void st(const Jac<CV>& v, u32* o) {
    Raw<typename CV::EX>::st(v.X, o);
    Raw<typename CV::EY>::st(v.Y, o + 9 * NX);
    Raw<typename CV::EZ>::st(v.Z, o + 9 * (NX + NY));
  }
};
template <class CV>
struct Raw<Xyzz<CV>> {
  static constexpr int NX = Bnd<typename CV::XX>::N, NY = Bnd<typename CV::XY>::N, NZ = Bnd<typename CV::XZZ>::N;
  static DC_FN Xyzz<CV> ld(const u32* const* x) {
    Xyzz<CV> r;
    r.X = Raw<typename CV::XX>::ld(x);
    r.Y = Raw<typename CV::XY>::ld(x + NX);
    r.ZZ = Raw<typename CV::XZZ>::ld(x + NX + NY);
    r.ZZZ = Raw<typename CV::XZZZ>::ld(x + NX + NY + NZ);
    return r;
  }
  static DC_FN void st(const Xyzz<CV>& v, u32* o) {
    Raw<typename CV::XX>::st(v.X, o);
    Raw<typename CV::XY>::st(v.Y, o + 9 * NX);
    Raw<typename CV::XZZ>::st(v.ZZ, o + 9 * (NX + NY));
    Raw<typename CV::XZZZ>::st(v.ZZZ, o + 9 * (NX + NY + NZ));
  }
};
template <class EA>
struct Raw<Aff<EA>> {
  static DC_FN Aff<EA> ld(const u32* const* x) {
    Aff<EA> r;
    r.x = Raw<EA>::ld(x);
    r.y = Raw<EA>::ld(x + Bnd<EA>::N);
    return r;
  }
  static DC_FN void st(const Aff<EA>& v, u32* o) {
    Raw<EA>::st(v.x, o);
    Raw<EA>::st(v.y, o + 9 * Bnd<EA>::N);
  }
};

template <class T>
DC_FN T ld(const u32* const* x) {
  return Raw<T>::ld(x);
}

// ---- the operations.  DC_OP(ID, NAME, GROUP, BODY over a0, a1, ..., OPERANDS...) defines one; GROUP is the number
// of lanes that hold one case (1, or 2 / 4 / 8 for the lane-pair, quad and octet code).  DC_OP_HD is the same
// for an operation that runs on either side.  (Two macros, not one forwarding to the other: a second expansion
// would turn the COMMA of an operand type into an argument separator.)
#define COMMA ,
#define DC_A(k, T) const auto a##k = ld<T>(x + off[k]);
template <int G, class... T>
struct OpBase {
  using In = TL<T...>;
  static constexpr int GROUP = G;
  static constexpr int PARAM = 0;    // csub's K, a Frobenius power
  static constexpr int SCRATCH = 0;  // words of scratch per lane; run() then takes (x, scratch + lane, lanes)
  static DC_FN void offsets(int (&off)[8]) {
    int k = 0, o = 0;
    ((off[k++] = o, o += Bnd<T>::N), ...);
  }
};

#define DC_OP(ID, NAME, G, ARGS, ...)                                                \
  struct ID : OpBase<G, __VA_ARGS__> {                                               \
    static constexpr const char* name = NAME;                                        \
    static __device__ auto run(const u32* const* x) {                                \
      int off[8];                                                                    \
      OpBase<G, __VA_ARGS__>::offsets(off);                                          \
      ARGS                                                                           \
    }                                                                                \
  };
#define DC_OP_HD(ID, NAME, G, ARGS, ...)                                             \
  struct ID : OpBase<G, __VA_ARGS__> {                                               \
    static constexpr const char* name = NAME;                                        \
    static DC_FN auto run(const u32* const* x) {                                     \
      int off[8];                                                                    \
      OpBase<G, __VA_ARGS__>::offsets(off);                                          \
      ARGS                                                                           \
    }                                                                                \
  };

template <class L>
struct Nth;
template <class... T>
struct Nth<TL<T...>> {
  static constexpr int N = sizeof...(T);
};
template <int I, class L>
struct At;
template <int I, class H, class... T>
struct At<I, TL<H, T...>> : At<I - 1, TL<T...>> {};
template <class H, class... T>
struct At<0, TL<H, T...>> {
  using type = H;
};

template <class Op, bool S = (Op::SCRATCH > 0)>
struct OutOf {
  using type = std::decay_t<decltype(Op::run(nullptr))>;
};
template <class Op>
struct OutOf<Op, true> {
  using type = std::decay_t<decltype(Op::run(nullptr, nullptr, 0))>;
};
template <class Op>
using OutT = typename OutOf<Op>::type;

#if defined(__HIPCC__)
// LB: the kernel's launch bound (1024 is what the compiler assumes without one)
template <class Op, int LB>
__global__ __launch_bounds__(LB) void k_op(const u32* __restrict__ in, u32* __restrict__ out, u32* __restrict__ scratch,
                                           int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int NIN = Op::In::N;
  if constexpr (Op::SCRATCH > 0) {
    if (i >= n) return;  // (an operation with scratch has no lane groups to keep whole)
    const u32* x[NIN];
#pragma unroll
    for (int k = 0; k < NIN; k++) x[k] = in + ((size_t)k * n + i) * 9;
    const auto r = Op::run(x, scratch + i, n);
    Raw<OutT<Op>>::st(r, out + (size_t)i * Bnd<OutT<Op>>::N * 9);
  } else {
    // a lane past the end still runs (on a copy of lane 0's operands) so that no lane group is split, but writes
    // nothing
    const int src = i < n ? i : 0;
    const u32* x[NIN];
#pragma unroll
    for (int k = 0; k < NIN; k++) x[k] = in + ((size_t)k * n + src) * 9;
    const auto r = Op::run(x);
    if (i < n) Raw<OutT<Op>>::st(r, out + (size_t)i * Bnd<OutT<Op>>::N * 9);
  }
}

// scratch: n * Op::SCRATCH words for an operation that asks for them (else unused)
template <class L, int LB, int I = 0>
int launch(int idx, const u32* in, u32* out, u32* scratch, int n, int block, hipStream_t s) {
  if constexpr (I == Nth<L>::N) {
    return -1;
  } else {
    if (idx != I) return launch<L, LB, I + 1>(idx, in, out, scratch, n, block, s);
    using Op = typename At<I, L>::type;
    if (block <= 0 || block > LB) return -4;
    if (Op::SCRATCH > 0 && scratch == nullptr) return -5;
    (void)hipGetLastError();  // drop a stale error left by somebody else's call
    hipLaunchKernelGGL((k_op<Op, LB>), dim3((n + block - 1) / block), dim3(block), 0, s, in, out, scratch, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
}
#endif

// info: [GROUP, NIN, NOUT, PARAM, in bounds (NIN), in LU (NIN), out bounds (NOUT), out LU (NOUT)]
template <class L, int I = 0>
int info(int idx, char* name, int* v) {
  if constexpr (I == Nth<L>::N) {
    return -1;
  } else {
    if (idx != I) return info<L, I + 1>(idx, name, v);
    using Op = typename At<I, L>::type;
    constexpr int NIN = Op::In::N, NOUT = Bnd<OutT<Op>>::N;
    strcpy(name, Op::name);
    v[0] = Op::GROUP;
    v[1] = NIN;
    v[2] = NOUT;
    v[3] = Op::PARAM;
    Op::In::get(v + 4, v + 4 + NIN);
    Bnd<OutT<Op>>::get(v + 4 + 2 * NIN, v + 4 + 2 * NIN + NOUT);
    return 0;
  }
}

template <class L, int I = 0>
int scratch_words(int idx) {
  if constexpr (I == Nth<L>::N) {
    return -1;
  } else {
    return idx == I ? At<I, L>::type::SCRATCH : scratch_words<L, I + 1>(idx);
  }
}

}  // namespace dc
