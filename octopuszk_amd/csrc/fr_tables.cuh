// What the Fr kernels of fft.hip and bace.cuh share: element I/O, host words in kernel arguments, exponentiation by a
// word, the two-level power table, and the description of one domain's tables.  Included by
// fft.hip only.
#pragma once
#include "curve.cuh"
#include "ozk_common.h"

namespace ozk {

using FrP = FrParams;

// ---- element I/O: 8 packed words (32 bytes, 16-byte aligned) as two 128-bit accesses ------------------------
// (ElemTraits<...>::load / store / from_wire / to_wire of curve.cuh are the word-by-word forms, for the one-lane
// kernels and for buffers whose alignment is the caller's.)
__device__ __forceinline__ void fr_store_words(const u32 (&o)[8], u32* dst) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  d[0] = make_uint4(o[0], o[1], o[2], o[3]);
  d[1] = make_uint4(o[4], o[5], o[6], o[7]);
}
template <int B>
__device__ __forceinline__ void fr_store(const Fe<FrP, B>& v, u32* dst) {
  u32 o[8];
  pack(v, o);
  fr_store_words(o, dst);
}
template <int B = 85>
__device__ __forceinline__ Fe<FrP, B> fr_load(const u32* src) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  const uint4 a = s[0], b = s[1];
  const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return unpack<FrP, B>(w);
}

// Montgomery form -> canonical plain words, word by word (the bound is the argument's)
template <int B>
__device__ __forceinline__ void fr_to_wire(const Fe<FrP, B>& v, u32* dst) {
  ElemTraits<Fe<FrP, B>>::to_wire(v, dst);
}

// ---- host words in the kernel arguments ------------------------------------------------------------------------
// Small host values reach the device as kernel arguments (captured at launch: no host buffer has to outlive the
// call): N elements of 8 packed words.  A kernel takes single elements this way (FrArg), and k_fr_put writes a batch
// to device memory: BACE's constants and roots of unity, which are temporaries of its host code, a domain's omega, the
// points of a set opening.
template <int N>
struct FrWords {
  u32 w[8 * N];
};
using FrArg = FrWords<1>;
template <int N>
__global__ void __launch_bounds__(256) k_fr_put(FrWords<N> c, int nw, u32* __restrict__ dst) {
  for (int i = threadIdx.x; i < nw; i += blockDim.x) dst[i] = c.w[i];
}
// one element of host memory to dst
inline void fr_put_element(const uint8_t* host32, u32* dst, hipStream_t st) {
  FrArg c;
  memcpy(c.w, host32, 32);
  hipLaunchKernelGGL(k_fr_put<1>, dim3(1), dim3(64), 0, st, c, 8, dst);
}

// base^e (base in Montgomery form, any bound the multiplier takes): 32 squarings, a product per set bit
template <int B>
OZK_HD Fe<FrP, 32> fe_pow_u32(const Fe<FrP, B>& base, unsigned e) {
  Fe<FrP, 32> r = fe_one<FrP>();
  for (int b = 31; b >= 0; b--) {
    r = Fe<FrP, 32>(sqr(r));
    if ((e >> b) & 1) r = Fe<FrP, 32>(mul(r, base));
  }
  return r;
}

// ---- the two-level power table ------------------------------------------------------------------------------
// pw[j] = base^j for j < lo, pw[lo + j] = base^(j lo) for j < hi; Montgomery form, packed 8 words: base^i for every
// i < lo hi is ONE product of two entries (pow_at), and the table is built by lo + hi independent lanes.
constexpr int TW_LO = 2048;
__global__ void __launch_bounds__(256) k_tw_small(const u32* __restrict__ base_wire, int lo, int hi,
                                                  u32* __restrict__ pw) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lo + hi) return;
  const auto base = ElemTraits<Fe<FrP, 32>>::from_wire(base_wire);
  const unsigned e = (t < lo) ? (unsigned)t : (unsigned)(t - lo) * (unsigned)lo;
  ElemTraits<Fe<FrP, 16>>::store(canonical(fe_pow_u32(base, e)), pw + (size_t)t * 8);
}
// base^i R, i < lo hi
__device__ __forceinline__ auto pow_at(const u32* __restrict__ pw, int lo, int i) {
  using ET = ElemTraits<Fe<FrP, 16>>;
  return mul(ET::load(pw + (size_t)(i % lo) * 8), ET::load(pw + (size_t)(lo + i / lo) * 8));
}
struct PowTable {
  int lo, hi;
  size_t words() const { return (size_t)(lo + hi) * 8; }
  // the transform's twiddles omega^t, t < half: no first level longer than the table
  static PowTable twiddles(int half) {
    const int lo = half < TW_LO ? half : TW_LO;
    return PowTable{lo, (half + lo - 1) / lo};
  }
  // base^i for every i <= n (coset powers, Lagrange coefficients, the powers of the setup's secret point)
  static PowTable upto(int n) { return PowTable{TW_LO, (n + TW_LO - 1) / TW_LO + 1}; }
  void build(const u32* d_base_wire, u32* pw, hipStream_t st) const {
    hipLaunchKernelGGL(k_tw_small, dim3((lo + hi + 255) / 256), dim3(256), 0, st, d_base_wire, lo, hi, pw);
  }
};

// ---- one domain's tables --------------------------------------------------------------------------------------
struct QapConsts {  // device-resident, packed 8 words each
  u32 omega[8], omega_inv[8], g[8], g_inv[8];  // wire form (plain canonical)
  u32 m_inv_mont[8];                           // (1/m) R
  u32 zinv_mont[8];                            // (1 / (g^m - 1)) R
};
// Everything that depends only on (n, omega[, g]).  A transform reads tw_f and needs consts->omega and `small` to
// build it; the witness map (g given) reads all of it.  The tables live in a plan of the cache or, built per call,
// in the caller's workspace: the same struct and the same carving describe both.
struct DomainTables {
  QapConsts* consts;     // a transform alone uses only its first field, omega
  u32* small;            // scratch of the twiddle builds: the two-level table of omega, then of omega^-1
  u32 *tw_f, *tw_i;      // twiddle pyramids of omega and omega^-1: n - 1 entries each
  u32 *pw_g, *pw_gi;     // two-level power tables of g and g^-1
  u32 *sc_g, *sc_gi;     // g^i / m and g^-i / m for every i < n: what a folded last pass multiplies by
};
inline int fft_half(int n) { return n / 2 > 0 ? n / 2 : 1; }
// the head of every carving: the root of unity and the scratch table
inline void carve_head(Bump& b, const PowTable& small, DomainTables& t) {
  t.consts = b.take<QapConsts>(1);   // (32 or 192 bytes: the next slot starts 256 bytes on either way)
  t.small = b.take<u32>(small.words());
}
// One order and one set of sizes for the caller's workspace and for a plan's memory, with a null base for the size
// alone.  `roomy`: the plan cache has always sized `small` for the powers up to n whatever the key; the byte budget
// counts it, so it stays.
inline DomainTables carve(Bump& b, int n, bool qap, bool roomy = false) {
  DomainTables t = {};
  const PowTable up = PowTable::upto(n);
  carve_head(b, qap || roomy ? up : PowTable::twiddles(fft_half(n)), t);
  t.tw_f = b.take<u32>((size_t)(n > 1 ? n : 1) * 8);
  if (qap) {
    t.tw_i = b.take<u32>((size_t)n * 8);
    t.pw_g = b.take<u32>(up.words());
    t.pw_gi = b.take<u32>(up.words());
    t.sc_g = b.take<u32>((size_t)n * 8);
    t.sc_gi = b.take<u32>((size_t)n * 8);
  }
  return t;
}

// n is a power of two in [lo, 2^28]; `what` names it in the message
inline int check_pow2(int n, int lo, const char* what) {
  if (n < lo || (n & (n - 1)) || n > (1 << 28))
    return fail(OZK_E_INVALID, "%s %d is not a power of two in [%d, 2^28]", what, n, lo);
  return OZK_OK;
}

}  // namespace ozk
