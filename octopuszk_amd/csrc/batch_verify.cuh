// Randomized batch verification of Groth16 proofs ("Batch verification"): K proofs become one check
//
//   FE( prod_i ML(r_i A_i, B_i) * (ML(ABC*, gamma) ML(C*, delta))^-1 ) == alphaBeta^S
//   ABC* = sum_j s_j gammaABC_j,  s_j = sum_i r_i x_ij mod r,  C* = sum_i r_i C_i,  S = sum_i r_i
//
// over the proofs that are well-formed (A, C on the curve, B on the twist and of order r, no Z = 0).  The arithmetic
// below compiles for the host too (tests/native/batch_verify_hostcheck.cpp); the kernels at the end exist only in the
// device pass of pairing.hip, which includes this header after its own miller() and point loaders.
#pragma once
#include "fq12.cuh"

namespace ozk {

using BvFq = Fe<FqParams, 32>;

// little-endian 32-bit words of the field moduli
constexpr u32 BV_Q_WORDS[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                               0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
constexpr u32 BV_R_WORDS[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u,
                               0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
constexpr int BV_REC_WORDS = 192;   // one proof record A (48 words) | B (96) | C (48), wire-out

// one wire-out Fq value (16 words): canonical, i.e. the upper 32 bytes zero and the lower ones < q
OZK_HD bool bv_canonical(const u32* p) {
  for (int i = 8; i < 16; i++)
    if (p[i]) return false;
  for (int i = 7; i >= 0; i--)
    if (p[i] != BV_Q_WORDS[i]) return p[i] < BV_Q_WORDS[i];
  return false;
}
OZK_HD BvFq bv_fq(const u32* p) {
  u32 w[8];
  for (int i = 0; i < 8; i++) w[i] = p[i];
  return BvFq(to_mont<FqParams>(w));
}
OZK_HD F2 bv_f2(const u32* p) {
  F2 r;
  r.c0 = bv_fq(p);
  r.c1 = bv_fq(p + 16);
  return r;
}

// A or C: canonical coordinates, Z != 0 and Y^2 = X^3 + 3 Z^6.  G1 has cofactor 1, so that makes it a point of G1.
OZK_HD bool bv_g1_wellformed(const u32* p) {
  for (int c = 0; c < 3; c++)
    if (!bv_canonical(p + 16 * c)) return false;
  const BvFq X = bv_fq(p), Y = bv_fq(p + 16), Z = bv_fq(p + 32);
  if (is_zero(Z)) return false;
  const u32 three[8] = {3, 0, 0, 0, 0, 0, 0, 0};
  const BvFq z2 = BvFq(sqr(Z));
  const BvFq z6 = BvFq(mul(BvFq(sqr(z2)), z2));
  const BvFq x3 = BvFq(mul(BvFq(sqr(X)), X));
  const BvFq rhs = BvFq(reduce_to<32>(add(x3, BvFq(mul(BvFq(to_mont<FqParams>(three)), z6)))));
  return is_zero(sub(BvFq(sqr(Y)), rhs));
}

// (scalar_mul, [e]q for an affine q: ec.cuh, where point_codec.cuh finds it too)

// B: canonical coordinates, Z != 0, Y^2 = X^3 + b' Z^6 with b' = 3 / (9 + u), and [r]B = O (the order-r subgroup;
// the twist's group has order r h with a large cofactor h, so the curve equation alone is not enough)
OZK_BIG bool bv_g2_wellformed(const u32* p) {
  for (int c = 0; c < 6; c++)
    if (!bv_canonical(p + 16 * c)) return false;
  const F2 X = bv_f2(p), Y = bv_f2(p + 32), Z = bv_f2(p + 64);
  if (is_zero(Z)) return false;
  const F2 z2 = sqr(Z);
  const F2 z6 = mul(sqr(z2), z2);
  const F2 rhs = f2_add(mul(sqr(X), X), mul(f2_const(pc::TWIST_B), z6));
  if (!is_zero(sub(sqr(Y), rhs))) return false;
  const F2 zi = inv(Z), zi2 = sqr(zi);
  const F2 x = mul(X, zi2), y = mul(Y, mul(zi2, zi));
  Aff<G2Cfg::EA> q;
  q.x.c0 = canonical(x.c0);
  q.x.c1 = canonical(x.c1);
  q.y.c0 = canonical(y.c0);
  q.y.c1 = canonical(y.c1);
  return is_inf(scalar_mul<G2Cfg>(q, BV_R_WORDS, 8));
}

OZK_HD int bv_proof_wellformed(const u32* rec) {
  return bv_g1_wellformed(rec) && bv_g1_wellformed(rec + 144) && bv_g2_wellformed(rec + 48) ? 1 : 0;
}

// r P for a well-formed G1 point (wire-out, any Z != 0) and a scalar r of `words` words, as the affine (x, y) that
// miller() takes.  r P = O (r a multiple of the order) gives (0, 1), the Java's affine form of infinity.
OZK_HD void bv_g1_mul_affine(const u32* p, const u32* r, int words, BvFq& x, BvFq& y) {
  const BvFq X = bv_fq(p), Y = bv_fq(p + 16), Z = bv_fq(p + 32);
  const BvFq zi = inv(Z), zi2 = BvFq(sqr(zi));
  Aff<G1Cfg::EA> q;
  q.x = canonical(BvFq(mul(X, zi2)));
  q.y = canonical(BvFq(mul(Y, BvFq(mul(zi2, zi)))));
  const Jac<G1Cfg> t = scalar_mul<G1Cfg>(q, r, words);
  if (is_inf(t)) {
    x = fe_zero<FqParams>();
    y = fe_one<FqParams>();
    return;
  }
  const BvFq ti = inv(t.Z), ti2 = BvFq(sqr(ti));
  x = BvFq(mul(t.X, ti2));
  y = BvFq(mul(t.Y, BvFq(mul(ti2, ti))));
}

// a^e for a in GT (the cyclotomic subgroup, where cyclotomic_sqr is the square), e of `words` little-endian words;
// e = 0 gives one
OZK_BIG Fe12 gt_pow(const Fe12& a, const u32* e, int words) {
  int top = -1;
  for (int i = 32 * words - 1; i >= 0 && top < 0; i--)
    if ((e[i >> 5] >> (i & 31)) & 1) top = i;
  if (top < 0) return f12_one();
  Fe12 res = a;
  for (int i = top - 1; i >= 0; i--) {
    res = cyclotomic_sqr(res);
    if ((e[i >> 5] >> (i & 31)) & 1) res = mul(res, a);
  }
  return res;
}

// ---- the Fr combination s_j = sum_i r_i x_ij mod r.  x in Montgomery form times r_i as a plain integer (< 2^128 < r)
// is the plain product x r_i, so every term costs one conversion and one product.
using BvFr = Fe<FrParams, 32>;
OZK_HD BvFr bv_fr_term(const u32* x, const u32* r) {
  u32 a[8], b[8];
  for (int i = 0; i < 8; i++) {
    a[i] = x[i];
    b[i] = r[i];
  }
  return BvFr(mul(to_mont<FrParams>(a), Fe<FrParams, 16>(unpack<FrParams, 16>(b))));
}
OZK_HD BvFr bv_fr_add(const BvFr& a, const BvFr& b) { return BvFr(reduce_to<32>(add(a, b))); }
OZK_HD void bv_fr_store(const BvFr& a, u32* out) {
  u32 w[8];
  pack(canonical(a), w);
  for (int i = 0; i < 8; i++) out[i] = w[i];
}
OZK_HD BvFr bv_fr_load(const u32* p) {
  u32 w[8];
  for (int i = 0; i < 8; i++) w[i] = p[i];
  return BvFr(unpack<FrParams, 16>(w));
}
// S = sum_i r_i as an integer: r_i < 2^128, so 192 bits hold 2^64 terms
struct BvSum {
  u64 w[3];
};
OZK_HD void bv_sum_add(BvSum& s, const u32* r) {
  const u64 lo = (u64)r[0] | (u64)r[1] << 32, hi = (u64)r[2] | (u64)r[3] << 32;
  s.w[0] += lo;
  const u64 c0 = s.w[0] < lo;
  const u64 h = hi + c0;   // hi + c0 wraps only when hi = 2^64 - 1 and c0 = 1
  const u64 c1 = h < hi;
  s.w[1] += h;
  s.w[2] += c1 + (s.w[1] < h);
}
OZK_HD void bv_sum_merge(BvSum& s, const BvSum& t) {
  s.w[0] += t.w[0];
  const u64 c0 = s.w[0] < t.w[0];
  const u64 h = t.w[1] + c0;
  const u64 c1 = h < t.w[1];
  s.w[1] += h;
  s.w[2] += t.w[2] + c1 + (s.w[1] < h);
}

// the product of f_in[lo, hi) (stride `stride`)
OZK_BIG Fe12 f12_prod_range(const u32* f_in, long stride, long lo, long hi) {
  Fe12 acc = load_f12(f_in + lo, stride);
  for (long j = lo + 1; j < hi; j++) acc = mul(acc, load_f12(f_in + j, stride));
  return acc;
}

#if defined(__HIPCC__) && !defined(OZK_BV_NO_KERNELS)
// ---------------------------------------------------------------------------------------------- kernels
// (miller, g1_affine, g2_affine: pairing.hip; tests/native/towercheck.hip, which has none of them, defines
// OZK_BV_NO_KERNELS and takes the arithmetic above alone)

__global__ __launch_bounds__(64) void k_wellformed(const u32* __restrict__ recs, int k, int32_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  ok[i] = bv_proof_wellformed(recs + (long)i * BV_REC_WORDS);
}

// the inputs of the C* MSM: C_i as a wire-in base and r_i as its scalar for a proof the check covers, else
// infinity (Z = 0) and 0.  use[i] = 1 (covered) when proof i is well-formed and 0 < r_i < 2^128.
__global__ __launch_bounds__(64) void k_rlc_inputs(const u32* __restrict__ recs, const u32* __restrict__ r,
                                                   const int32_t* __restrict__ wf, int k, u32* __restrict__ c_bases,
                                                   u32* __restrict__ c_scalars, int32_t* __restrict__ use) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const u32* ri = r + 8L * i;
  bool nz = false, small = true;
  for (int w = 0; w < 4; w++) nz = nz || ri[w] != 0;
  for (int w = 4; w < 8; w++) small = small && ri[w] == 0;
  const bool on = wf[i] && nz && small;
  const u32* c = recs + (long)i * BV_REC_WORDS + 144;
  for (int co = 0; co < 3; co++)
    for (int w = 0; w < 8; w++) c_bases[24L * i + 8 * co + w] = on ? c[16 * co + w] : 0u;
  for (int w = 0; w < 8; w++) c_scalars[8L * i + w] = on ? ri[w] : 0u;
  use[i] = on ? 1 : 0;
}

// blockIdx.x < n: s_j for j = blockIdx.x; blockIdx.x == n: S.  256 threads stride over the proofs, then a tree in LDS.
// x: k rows of n 32-byte values; s_out: n 32-byte canonical values (the MSM's scalars), then S as a 32-byte integer.
__global__ __launch_bounds__(256) void k_rlc_combine(const u32* __restrict__ x, const u32* __restrict__ r,
                                                     const int32_t* __restrict__ use, int k, int n,
                                                     u32* __restrict__ s_out) {
  __shared__ u64 l64[256 * 4];
  u32* lds = (u32*)l64;
  const int t = threadIdx.x, j = blockIdx.x;
  if (j < n) {
    BvFr acc = BvFr(fe_zero<FrParams>());
    for (int i = t; i < k; i += 256)
      if (use[i]) acc = bv_fr_add(acc, bv_fr_term(x + (8L * n) * i + 8L * j, r + 8L * i));
    bv_fr_store(acc, lds + 8 * t);
    for (int h = 128; h > 0; h >>= 1) {
      block_sync();
      if (t < h) bv_fr_store(bv_fr_add(bv_fr_load(lds + 8 * t), bv_fr_load(lds + 8 * (t + h))), lds + 8 * t);
    }
    block_sync();
    if (t < 8) s_out[8L * j + t] = lds[t];
  } else {
    BvSum acc{{0, 0, 0}};
    for (int i = t; i < k; i += 256)
      if (use[i]) bv_sum_add(acc, r + 8L * i);
    for (int w = 0; w < 3; w++) l64[4 * t + w] = acc.w[w];
    for (int h = 128; h > 0; h >>= 1) {
      block_sync();
      if (t < h) {
        BvSum a{{l64[4 * t], l64[4 * t + 1], l64[4 * t + 2]}};
        const BvSum b{{l64[4 * (t + h)], l64[4 * (t + h) + 1], l64[4 * (t + h) + 2]}};
        bv_sum_merge(a, b);
        for (int w = 0; w < 3; w++) l64[4 * t + w] = a.w[w];
      }
    }
    block_sync();
    if (t < 8) s_out[8L * n + t] = t < 6 ? (u32)(l64[t >> 1] >> (32 * (t & 1))) : 0u;
  }
}

// The Miller loops of the check, one per lane.  Three single-lane blocks come first, so that they are dispatched
// before the proof blocks fill the machine and overlap them at every K: block 0 ML(ABC*, gamma) and block 1
// ML(C*, delta) over the prepared keys (status[0 / 1] = 1 when the point is at infinity), block 2 alphaBeta^S.
// Blocks [3, 3 + ceil(k / 64)): proof i = lane, ML(r_i A_i, B_i) with B_i's steps inline, or one for a proof outside
// the combination.
constexpr int RLC_KEY_BLOCKS = 3;
__global__ __launch_bounds__(64) void k_rlc_miller(const u32* __restrict__ recs, const u32* __restrict__ r,
                                                   const int32_t* __restrict__ use, int k,
                                                   const u32* __restrict__ abc_star, const u32* __restrict__ c_star,
                                                   const u32* __restrict__ gamma_prep,
                                                   const u32* __restrict__ delta_prep,
                                                   const u32* __restrict__ alpha_beta, const u32* __restrict__ S,
                                                   u32* __restrict__ f_out, u32* __restrict__ key_out,
                                                   u32* __restrict__ pow_out, int32_t* __restrict__ status) {
  const int b = blockIdx.x;
  if (b >= RLC_KEY_BLOCKS) {
    const int i = (b - RLC_KEY_BLOCKS) * blockDim.x + threadIdx.x;
    if (i >= k) return;
    Fe12 f = f12_one();
    if (use[i]) {
      const u32* rec = recs + (long)i * BV_REC_WORDS;
      BvFq px, py;
      bv_g1_mul_affine(rec, r + 8L * i, 4, px, py);
      F2 qx, qy;
      g2_affine<16>(rec + 48, qx, qy);
      f = miller(px, py, qx, qy, nullptr, 0);
    }
    store_f12(f, f_out + i, k);
    return;
  }
  if (threadIdx.x != 0) return;
  if (b < 2) {
    const u32* p = b == 0 ? abc_star : c_star;
    const bool inf = is_zero(bv_fq(p + 32));
    status[b] = inf ? 1 : 0;
    Fe12 f = f12_one();
    if (!inf) {
      BvFq px, py;
      g1_affine<16>(p, px, py);
      f = miller(px, py, f2_zero(), f2_zero(), b == 0 ? gamma_prep : delta_prep, 1);
    }
    store_f12(f, key_out + b, 2);
  } else {
    store_f12(gt_pow(f12_from_wire(alpha_beta), S, 8), pow_out, 1);
  }
}

// out[i] = the product of in[i chunk, min(n, (i + 1) chunk)); in has stride n, out stride ceil(n / chunk)
__global__ __launch_bounds__(64) void k_f12_prod(const u32* __restrict__ f_in, int n, int chunk,
                                                 u32* __restrict__ f_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = (n + chunk - 1) / chunk;
  if (i >= m) return;
  const long lo = (long)i * chunk, hi = lo + chunk < n ? lo + chunk : n;
  store_f12(f12_prod_range(f_in, n, lo, hi), f_out + i, m);
}

// verdict: 1 accepted, 0 rejected, -1 declined (ABC* or C* at infinity, or a zero Miller value: the product form is
// then not exact and the caller judges the proofs one by one)
__global__ __launch_bounds__(64) void k_rlc_final(const u32* __restrict__ prod, const u32* __restrict__ key,
                                                  const u32* __restrict__ pw, const int32_t* __restrict__ status,
                                                  int32_t* __restrict__ verdict) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (status[0] || status[1]) {
    *verdict = -1;
    return;
  }
  const Fe12 a = load_f12(prod, 1);
  const Fe12 bc = mul(load_f12(key, 2), load_f12(key + 1, 2));
  if (is_zero(a) || is_zero(bc)) {
    *verdict = -1;
    return;
  }
  *verdict = f12_eq(final_exponentiation(mul(a, inv(bc))), load_f12(pw, 1)) ? 1 : 0;
}

// ozk_gt_pow_dev: gt_out[i] = gt_in[i]^e_i, e_i a 32-byte little-endian integer
__global__ __launch_bounds__(64) void k_gt_pow(const u32* __restrict__ gt_in, const u32* __restrict__ e, int n,
                                               u32* __restrict__ gt_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f12_to_wire(gt_pow(f12_from_wire(gt_in + 96L * i), e + 8L * i, 8), gt_out + 96L * i);
}
#endif

}  // namespace ozk
