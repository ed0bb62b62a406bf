// What the Fr units (fft.hip, bace.hip, kzg.hip, plonk.hip) share: element I/O, host words in kernel arguments,
// exponentiation by a word, the two-level power table, the description of one domain's tables, the workgroup sum and
// the small kernels that more than one unit launches (DESIGN.md sections 19 and 34).  Stands alone.  A kernel here
// that is no template is `static` (hipcc ignores `inline` on a kernel): under -fno-gpu-rdc each unit that launches it
// compiles and registers its own copy.
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
static __global__ void __launch_bounds__(256) k_tw_small(const u32* __restrict__ base_wire, int lo, int hi,
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

// ---- the workgroup sum ------------------------------------------------------------------------------------------
// The sum of the 256 lanes' accumulators: a tree over the partials in LDS (part: 9 x 256 words, limb-major)
using FrAcc = Fe<FrP, 32>;
__device__ __forceinline__ FrAcc fr_block_sum(FrAcc acc, u32* part) {
#pragma unroll
  for (int i = 0; i < 9; i++) part[i * 256 + threadIdx.x] = acc.l[i];
  block_sync();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      FrAcc x, y;
#pragma unroll
      for (int i = 0; i < 9; i++) {
        x.l[i] = part[i * 256 + threadIdx.x];
        y.l[i] = part[i * 256 + threadIdx.x + o];
      }
      const FrAcc s = FrAcc(reduce_to<32>(add(x, y)));
#pragma unroll
      for (int i = 0; i < 9; i++) part[i * 256 + threadIdx.x] = s.l[i];
    }
    block_sync();
  }
  FrAcc r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = part[i * 256];
  return r;
}

// ---- small kernels that more than one unit launches --------------------------------------------------------------
// wire (plain canonical) constants -> Montgomery form, in place: one lane per 8-word element
static __global__ void k_to_mont_inplace(u32* __restrict__ v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ElemTraits<Fe<FrP, 16>>::store(canonical(ElemTraits<Fe<FrP, 17>>::from_wire(v + (size_t)i * 8)), v + (size_t)i * 8);
}

// Polynomial evaluation at a point (ozk_fr_poly_eval_dev of kzg.hip, ozk_bace_columns_at_dev of bace.hip).
// Lane g of polynomial y (S = gridDim.x x 256 lanes per polynomial) runs Horner in r^S over the coefficients
// c[g], c[g + S], ... (consecutive lanes read consecutive coefficients), multiplies by r^g, and the workgroup's sum
// goes to partial[y gridDim.x + blockIdx.x]; k_fr_sum_partials adds each polynomial's partials.  The coefficients are
// any 256-bit words, reduced mod r on load (the KZG callers pass their rows as they got them); the partials are canonical.
static __global__ void __launch_bounds__(256) k_fr_poly_eval(const u32* __restrict__ c, size_t poly_cs, int len,
                                                             const u32* __restrict__ r_mont, u32* __restrict__ partial) {
  __shared__ u32 part[9 * 256];
  const u32 S = gridDim.x * 256u;
  const u32 g = blockIdx.x * 256u + threadIdx.x;
  const u32* cp = c + (size_t)blockIdx.y * poly_cs;
  const auto r = ElemTraits<Fe<FrP, 16>>::load(r_mont);
  FrAcc acc = FrAcc(fe_zero<FrP>());
  if (g < (u32)len) {
    const FrAcc rS = fe_pow_u32(r, S);
    // No reduction inside the loop: the product is below 18/16 r, a coefficient as loaded below 85/16 r, and the
    // multiplier takes their sum (below 103/16 r) as it is.  The bounds are the types': a wider one does not compile.
    Fe<FrP, 103> h = Fe<FrP, 103>(fe_zero<FrP>());
    for (long long k = ((u32)len - 1 - g) / S; k >= 0; k--)   // plain: (h rS R) / R
      h = add(mul(h, rS), fr_load<85>(cp + ((size_t)g + (size_t)k * S) * 8));
    acc = FrAcc(mul(h, fe_pow_u32(r, g)));
  }
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x == 0) fr_store(canonical(sum), partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8);
}
static __global__ void __launch_bounds__(256) k_fr_sum_partials(const u32* __restrict__ partial, int per, u32* __restrict__ out) {
  __shared__ u32 part[9 * 256];
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = threadIdx.x; i < per; i += 256)
    acc = FrAcc(reduce_to<32>(add(acc, fr_load<16>(partial + ((size_t)blockIdx.x * per + i) * 8))));
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x == 0) fr_store(canonical(sum), out + (size_t)blockIdx.x * 8);
}
// the batched polynomial evaluation: npolys polynomials of len coefficients at c + y poly_cs (words); r_mont: device
constexpr int FR_POLY_EVAL_MAX = 65535;   // polynomials of one call: gridDim.y
static void fr_poly_eval(const u32* c, size_t poly_cs, int len, int npolys, const u32* r_mont, u32* partial, u32* out,
                         hipStream_t st) {
  int nb = (len + 256 * 32 - 1) / (256 * 32);
  if (nb > 256) nb = 256;
  hipLaunchKernelGGL(k_fr_poly_eval, dim3(nb, npolys), dim3(256), 0, st, c, poly_cs, len, r_mont, partial);
  hipLaunchKernelGGL(k_fr_sum_partials, dim3(npolys), dim3(256), 0, st, (const u32*)partial, nb, out);
}

// n is a power of two in [lo, 2^28]; `what` names it in the message
inline int check_pow2(int n, int lo, const char* what) {
  if (n < lo || (n & (n - 1)) || n > (1 << 28))
    return fail(OZK_E_INVALID, "%s %d is not a power of two in [%d, 2^28]", what, n, lo);
  return OZK_OK;
}

}  // namespace ozk
