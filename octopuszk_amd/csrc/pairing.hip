// The BN254a optimal-ate pairing and the Groth16 verifier on the device (BNPairing.java, Verifier.java:24-59).
// One pairing per lane; the tower and the steps are fq12.cuh.
//
//   k_g2_prepare    the 102 line-coefficient triples of precomputeG2 per point (BNPairing.java:284-325)
//   k_miller        millerLoop (BNPairing.java:236-276) over prepared coefficients, or with the G2 steps inline
//   k_final_exp     finalExponentiation (BNPairing.java:333-336) -> GT wire bytes
//   k_verify_final  per proof FE(ML(A,B) (ML(ABC,gamma) ML(C,delta))^-1) == alphaG1betaG2
//   batch_verify.cuh  randomized batch verification of K proofs as one check, products of pairings, GT powers
//
// A Miller value f lives in one lane's registers (108 VGPRs); the kernels are launched one wave per workgroup with
// __launch_bounds__(64) so the compiler may use the whole register file.  The Miller values between the loop and
// the final exponentiation go through HBM (432 B per pair), which keeps the two register budgets apart.
#include <algorithm>

#include "ozk_common.h"
#include "curve.cuh"
#include "fq12.cuh"

namespace ozk {

using Fq32 = Fe<FqParams, 32>;

__device__ __forceinline__ Fq32 fq_from_words(const u32* p) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = p[i];
  return Fq32(to_mont<FqParams>(w));
}
// toAffineCoordinates (BNG1.java:163-172): infinity (Z = 0) -> (0, 1); else (X / Z^2, Y / Z^3).  S = words per Fq
// value in the record: 8 (wire-in) or 16 (wire-out).
template <int S>
__device__ __forceinline__ void g1_affine(const u32* p, Fq32& x, Fq32& y) {
  const Fq32 X = fq_from_words(p), Y = fq_from_words(p + S), Z = fq_from_words(p + 2 * S);
  if (is_zero(Z)) {
    x = fe_zero<FqParams>();
    y = fe_one<FqParams>();
  } else {
    const Fq32 zi = inv(Z);
    const Fq32 z2 = Fq32(sqr(zi));
    x = Fq32(mul(X, z2));
    y = Fq32(mul(Y, Fq32(mul(z2, zi))));
  }
}
template <int S>
__device__ __forceinline__ F2 f2_from_words(const u32* p) {
  F2 r;
  r.c0 = fq_from_words(p);
  r.c1 = fq_from_words(p + S);
  return r;
}
// BNG2.java:168-177
template <int S>
__device__ __forceinline__ void g2_affine(const u32* p, F2& x, F2& y) {
  const F2 X = f2_from_words<S>(p), Y = f2_from_words<S>(p + 2 * S), Z = f2_from_words<S>(p + 4 * S);
  if (is_zero(Z)) {
    x = f2_zero();
    y = f2_one();
  } else {
    const F2 zi = inv(Z);
    const F2 z2 = sqr(zi);
    x = mul(X, z2);
    y = mul(Y, mul(z2, zi));
  }
}

// The Miller loop of one pair.  prep != nullptr: line coefficients of step s at prep[(s * ELL_WORDS + w) * pstride],
// else the G2 steps run inline on (qx, qy).  Step kinds come from pc::ATE_STEP_KIND (0 doubling, 1 + Q, 2 + Q1,
// 3 + (-Q2)); every doubling is preceded by the squaring of f.
__device__ Fe12 miller(const Fq32& px, const Fq32& py, F2 qx, F2 qy, const u32* prep, long pstride) {
  Fe12 f = f12_one();
  G2Proj cur{qx, qy, f2_one()};
  F2 bx = qx, by = qy;
  for (int s = 0; s < pc::ATE_STEPS; s++) {
    const int kind = pc::ATE_STEP_KIND[s];
    if (kind == 0) f = sqr(f);
    Ell c;
    if (prep) {
      const u32* q = prep + (long)s * ELL_WORDS * pstride;
      c.ell0 = load_f2(q, pstride);
      c.ellVW = load_f2(q + 18 * pstride, pstride);
      c.ellVV = load_f2(q + 36 * pstride, pstride);
    } else if (kind == 0) {
      c = doubling_step(cur);
    } else {
      if (kind >= 2) {
        mul_by_q(bx, by);                 // Q1 = pi(Q), then Q2 = pi(Q1)
        if (kind == 3) by = f2_neg(by);   // -Q2
      }
      c = mixed_addition_step(bx, by, cur);
    }
    f = apply_line(f, c, px, py);
  }
  return f;
}

__global__ __launch_bounds__(64) void k_g2_prepare(const u32* __restrict__ q_wire, int n, u32* __restrict__ prep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F2 x, y;
  g2_affine<8>(q_wire + (long)i * 48, x, y);
  G2Proj cur{x, y, f2_one()};
  F2 bx = x, by = y;
  u32* out = prep + i;
  for (int s = 0; s < pc::ATE_STEPS; s++) {
    const int kind = pc::ATE_STEP_KIND[s];
    Ell c;
    if (kind == 0) {
      c = doubling_step(cur);
    } else {
      if (kind >= 2) {
        mul_by_q(bx, by);
        if (kind == 3) by = f2_neg(by);
      }
      c = mixed_addition_step(bx, by, cur);
    }
    u32* q = out + (long)s * ELL_WORDS * n;
    store_f2(c.ell0, q, n);
    store_f2(c.ellVW, q + 18L * n, n);
    store_f2(c.ellVV, q + 36L * n, n);
  }
}

// pairs (p_wire[i], q[i]) in wire-in format; prepared: q is n prepared points (k_g2_prepare's layout)
__global__ __launch_bounds__(64) void k_miller(const u32* __restrict__ p_wire, const u32* __restrict__ q, int prepared,
                                               int n, u32* __restrict__ f_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq32 px, py;
  g1_affine<8>(p_wire + (long)i * 24, px, py);
  F2 qx = f2_zero(), qy = f2_zero();
  if (!prepared) g2_affine<8>(q + (long)i * 48, qx, qy);
  const Fe12 f = miller(px, py, qx, qy, prepared ? q + i : nullptr, n);
  store_f12(f, f_out + i, n);
}

// Groth16: blockIdx.y selects the pair of every proof, uniformly over the wave: 0 (A, B) with B's steps inline,
// 1 (evaluationABC, gamma) and 2 (C, delta) over the prepared keys.  f_out holds 3k values, pair y of proof j at
// index y k + j.
__global__ __launch_bounds__(64) void k_verify_miller(const u32* __restrict__ proofs, const u32* __restrict__ abc,
                                                      const u32* __restrict__ gamma_prep,
                                                      const u32* __restrict__ delta_prep, int k, u32* __restrict__ f_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int y = blockIdx.y;
  const u32* rec = proofs + (long)j * 192;   // A (48 words) | B (96) | C (48), wire-out
  Fq32 px, py;
  F2 qx = f2_zero(), qy = f2_zero();
  const u32* prep = nullptr;
  if (y == 0) {
    g1_affine<16>(rec, px, py);
    g2_affine<16>(rec + 48, qx, qy);
  } else if (y == 1) {
    g1_affine<16>(abc + (long)j * 48, px, py);
    prep = gamma_prep;
  } else {
    g1_affine<16>(rec + 144, px, py);
    prep = delta_prep;
  }
  const Fe12 f = miller(px, py, qx, qy, prep, 1);
  store_f12(f, f_out + (long)y * k + j, 3L * k);
}

__global__ __launch_bounds__(64) void k_final_exp(const u32* __restrict__ f_in, int n, u32* __restrict__ gt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe12 r = final_exponentiation(load_f12(f_in + i, n));
  f12_to_wire(r, gt + (long)i * 96);
}

// Verifier.java checks FE(AB) == alphaBeta FE(ABC gamma) FE(C delta).  The final exponentiation is the power map
// x -> x^e on Fq12*, hence multiplicative, so for non-zero Miller values a, b, c that is exactly
// FE(a (b c)^-1) == alphaBeta: one final exponentiation instead of three.  A Miller value is zero only if one of
// its line values is (Fq12 is a field); the Java then has no boolean to give — its final exponentiation inverts
// the zero value and BigInteger.modInverse throws — and the proof is reported as not verified.
__global__ __launch_bounds__(64) void k_verify_final(const u32* __restrict__ f_in, int k,
                                                     const u32* __restrict__ alpha_beta, int32_t* __restrict__ ok) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const long st = 3L * k;
  const Fe12 a = load_f12(f_in + j, st);
  const Fe12 bc = mul(load_f12(f_in + k + j, st), load_f12(f_in + 2L * k + j, st));
  int32_t v = 0;
  if (!is_zero(a) && !is_zero(bc)) v = f12_eq(final_exponentiation(mul(a, inv(bc))), f12_from_wire(alpha_beta)) ? 1 : 0;
  ok[j] = v;
}

constexpr size_t PREP_BYTES = (size_t)pc::ATE_STEPS * ELL_WORDS * 4;
constexpr size_t F12_BYTES = (size_t)FE12_WORDS * 4;
constexpr int MAX_N = 1 << 24;   // (indices are 64-bit; this only rejects absurd counts)
constexpr int PROD_CHUNK = 16;   // Miller values multiplied per lane at each level of the product tree

}  // namespace ozk

#include "batch_verify.cuh"

namespace ozk {

// the product of the n Miller values in d_f (stride n) into d_out (one value), through d_tmp (ceil(n / 16) values)
static hipError_t f12_product(u32* d_f, int n, u32* d_tmp, u32* d_out, hipStream_t s) {
  u32* src = d_f;
  while (n > 1) {
    const int m = (n + PROD_CHUNK - 1) / PROD_CHUNK;
    u32* dst = m == 1 ? d_out : (src == d_tmp ? d_f : d_tmp);
    hipLaunchKernelGGL(k_f12_prod, dim3((m + 63) / 64), dim3(64), 0, s, (const u32*)src, n, PROD_CHUNK, dst);
    src = dst;
    n = m;
  }
  return src != d_out ? hipMemcpyAsync(d_out, src, F12_BYTES, hipMemcpyDeviceToDevice, s) : hipSuccess;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace ozk

using namespace ozk;

extern "C" {

size_t ozk_pairing_g2_prepared_bytes(int32_t n) { return n > 0 ? (size_t)n * PREP_BYTES : 0; }

int ozk_pairing_g2_prepare_dev(const void* d_q, int32_t n, void* d_prep, size_t prep_bytes, void* stream) {
  hip_clear_stale();
  if (!d_q || !d_prep || n <= 0 || n > MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (prep_bytes < ozk_pairing_g2_prepared_bytes(n))
    return fail(OZK_E_INVALID, "prepared buffer too small: %zu < %zu", prep_bytes, ozk_pairing_g2_prepared_bytes(n));
  hipLaunchKernelGGL(k_g2_prepare, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const u32*)d_q, (int)n,
                     (u32*)d_prep);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_reduced_pairing_dev(const void* d_p, const void* d_q_or_prep, int32_t prepared, int32_t n, void* d_gt,
                            void* stream) {
  hip_clear_stale();
  if (!d_p || !d_q_or_prep || !d_gt || n <= 0 || n > MAX_N) return fail(OZK_E_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  u32* d_f = nullptr;
  OZK_HIP(hipMallocAsync((void**)&d_f, (size_t)n * F12_BYTES, s));
  hipLaunchKernelGGL(k_miller, dim3((n + 63) / 64), dim3(64), 0, s, (const u32*)d_p, (const u32*)d_q_or_prep,
                     (int)(prepared != 0), (int)n, d_f);
  hipLaunchKernelGGL(k_final_exp, dim3((n + 63) / 64), dim3(64), 0, s, (const u32*)d_f, (int)n, (u32*)d_gt);
  const hipError_t e = hipGetLastError();
  OZK_HIP(hipFreeAsync(d_f, s));
  OZK_HIP(e);
  return OZK_OK;
}

int ozk_groth16_verify_dev(const void* d_alpha_beta, const void* d_gamma_prep, const void* d_delta_prep,
                           const void* d_proofs, const void* d_abc, int32_t k, int32_t* d_ok, void* stream) {
  hip_clear_stale();
  if (!d_alpha_beta || !d_gamma_prep || !d_delta_prep || !d_proofs || !d_abc || !d_ok || k <= 0 || k > MAX_N)
    return fail(OZK_E_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  u32* d_f = nullptr;
  OZK_HIP(hipMallocAsync((void**)&d_f, (size_t)3 * k * F12_BYTES, s));
  hipLaunchKernelGGL(k_verify_miller, dim3((k + 63) / 64, 3), dim3(64), 0, s, (const u32*)d_proofs, (const u32*)d_abc,
                     (const u32*)d_gamma_prep, (const u32*)d_delta_prep, (int)k, d_f);
  hipLaunchKernelGGL(k_verify_final, dim3((k + 63) / 64), dim3(64), 0, s, (const u32*)d_f, (int)k,
                     (const u32*)d_alpha_beta, d_ok);
  const hipError_t e = hipGetLastError();
  OZK_HIP(hipFreeAsync(d_f, s));
  OZK_HIP(e);
  return OZK_OK;
}

int ozk_pairing_product_dev(const void* d_p, const void* d_q_or_prep, int32_t prepared, int32_t n, void* d_gt,
                            void* stream) {
  hip_clear_stale();
  if (!d_p || !d_q_or_prep || !d_gt || n <= 0 || n > MAX_N) return fail(OZK_E_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int m = (n + PROD_CHUNK - 1) / PROD_CHUNK;
  u32* d_f = nullptr;
  OZK_HIP(hipMallocAsync((void**)&d_f, ((size_t)n + m + 1) * F12_BYTES, s));
  u32* d_tmp = d_f + (size_t)n * FE12_WORDS;
  u32* d_prod = d_tmp + (size_t)m * FE12_WORDS;
  hipLaunchKernelGGL(k_miller, dim3((n + 63) / 64), dim3(64), 0, s, (const u32*)d_p, (const u32*)d_q_or_prep,
                     (int)(prepared != 0), (int)n, d_f);
  hipError_t e = f12_product(d_f, n, d_tmp, d_prod, s);
  hipLaunchKernelGGL(k_final_exp, dim3(1), dim3(64), 0, s, (const u32*)d_prod, 1, (u32*)d_gt);
  if (e == hipSuccess) e = hipGetLastError();
  OZK_HIP(hipFreeAsync(d_f, s));
  OZK_HIP(e);
  return OZK_OK;
}

int ozk_gt_pow_dev(const void* d_gt, const void* d_exp, int32_t n, void* d_out, void* stream) {
  hip_clear_stale();
  if (!d_gt || !d_exp || !d_out || n <= 0 || n > MAX_N) return fail(OZK_E_INVALID, "bad argument");
  hipLaunchKernelGGL(k_gt_pow, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const u32*)d_gt,
                     (const u32*)d_exp, (int)n, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_groth16_wellformed_dev(const void* d_proofs, int32_t k, int32_t* d_flags, void* stream) {
  hip_clear_stale();
  if (!d_proofs || !d_flags || k <= 0 || k > MAX_N) return fail(OZK_E_INVALID, "bad argument");
  hipLaunchKernelGGL(k_wellformed, dim3((k + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const u32*)d_proofs,
                     (int)k, d_flags);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_groth16_verify_rlc_dev(const void* d_alpha_beta, const void* d_gamma_prep, const void* d_delta_prep,
                               const void* d_gamma_abc, int32_t n, const void* d_proofs, const void* d_inputs,
                               const void* d_r, int32_t k, int32_t* d_covered, int32_t* d_verdict, float* stage_ms,
                               void* stream) {
  hip_clear_stale();
  if (!d_alpha_beta || !d_gamma_prep || !d_delta_prep || !d_gamma_abc || !d_proofs || !d_inputs || !d_r ||
      !d_covered || !d_verdict || n <= 0 || n > MAX_N || k <= 0 || k > MAX_N)
    return fail(OZK_E_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t ws_bytes = std::max(ozk_var_msm_workspace_bytes(n, OZK_G1), ozk_var_msm_workspace_bytes(k, OZK_G1));
  if (ws_bytes == 0) return fail(OZK_E_INVALID, "MSM workspace size query failed");
  const int nb = (k + 63) / 64, m = (k + PROD_CHUNK - 1) / PROD_CHUNK;
  // one allocation, carved: wf, C* bases, C* scalars, s_j | S, ABC*, C*, status, Miller values, tree, key values,
  // alphaBeta^S, product, MSM workspace
  const size_t sz[] = {(size_t)k * 4, (size_t)k * 96, (size_t)k * 32, ((size_t)n + 1) * 32, 192, 192, 8,
                       (size_t)k * F12_BYTES, (size_t)m * F12_BYTES, 2 * F12_BYTES, F12_BYTES, F12_BYTES, ws_bytes};
  constexpr int NP = sizeof(sz) / sizeof(sz[0]);
  size_t off[NP], total = 0;
  for (int i = 0; i < NP; i++) {
    off[i] = total;
    total += align256(sz[i]);
  }
  uint8_t* base = nullptr;
  OZK_HIP(hipMallocAsync((void**)&base, total, s));
  int32_t* d_wf = (int32_t*)(base + off[0]);
  u32* d_cb = (u32*)(base + off[1]);
  u32* d_cs = (u32*)(base + off[2]);
  u32* d_s = (u32*)(base + off[3]);
  u32* d_abc = (u32*)(base + off[4]);
  u32* d_cstar = (u32*)(base + off[5]);
  int32_t* d_status = (int32_t*)(base + off[6]);
  u32* d_f = (u32*)(base + off[7]);
  u32* d_tmp = (u32*)(base + off[8]);
  u32* d_key = (u32*)(base + off[9]);
  u32* d_pow = (u32*)(base + off[10]);
  u32* d_prod = (u32*)(base + off[11]);
  void* d_ws = base + off[12];

  // stage_ms != nullptr: five stage times (combination, MSMs, Miller loops, product tree, final exponentiation),
  // taken with events; the call then waits for the stream
  hipEvent_t ev[6] = {};
  int rc = OZK_OK;
  hipError_t e = hipSuccess;
  if (stage_ms)
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
  auto mark = [&](int i) {
    if (stage_ms && e == hipSuccess) e = hipEventRecord(ev[i], s);
  };
  mark(0);
  hipLaunchKernelGGL(k_wellformed, dim3(nb), dim3(64), 0, s, (const u32*)d_proofs, (int)k, d_wf);
  hipLaunchKernelGGL(k_rlc_inputs, dim3(nb), dim3(64), 0, s, (const u32*)d_proofs, (const u32*)d_r,
                     (const int32_t*)d_wf, (int)k, d_cb, d_cs, d_covered);
  hipLaunchKernelGGL(k_rlc_combine, dim3(n + 1), dim3(256), 0, s, (const u32*)d_inputs, (const u32*)d_r,
                     (const int32_t*)d_covered, (int)k, (int)n, d_s);
  mark(1);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) rc = ozk_var_msm_dev(d_gamma_abc, d_s, n, OZK_G1, d_abc, d_ws, ws_bytes, s);
  if (e == hipSuccess && rc == OZK_OK) rc = ozk_var_msm_dev(d_cb, d_cs, k, OZK_G1, d_cstar, d_ws, ws_bytes, s);
  mark(2);
  if (e == hipSuccess && rc == OZK_OK) {
    hipLaunchKernelGGL(k_rlc_miller, dim3(RLC_KEY_BLOCKS + nb), dim3(64), 0, s, (const u32*)d_proofs,
                       (const u32*)d_r, (const int32_t*)d_covered, (int)k, (const u32*)d_abc, (const u32*)d_cstar,
                       (const u32*)d_gamma_prep, (const u32*)d_delta_prep, (const u32*)d_alpha_beta,
                       (const u32*)(d_s + 8L * n), d_f, d_key, d_pow, d_status);
    mark(3);
    e = f12_product(d_f, k, d_tmp, d_prod, s);
    mark(4);
    hipLaunchKernelGGL(k_rlc_final, dim3(1), dim3(64), 0, s, (const u32*)d_prod, (const u32*)d_key,
                       (const u32*)d_pow, (const int32_t*)d_status, d_verdict);
    mark(5);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (stage_ms && e == hipSuccess && rc == OZK_OK) {
    e = hipEventSynchronize(ev[5]);
    for (int i = 0; i < 5 && e == hipSuccess; i++) e = hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]);
  }
  for (int i = 0; i < 6; i++)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  const hipError_t ef = hipFreeAsync(base, s);
  OZK_HIP(e);
  OZK_HIP(ef);
  return rc;
}

}  // extern "C"
