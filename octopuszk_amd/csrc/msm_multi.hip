// Batched MSM over SHARED bases, G1:  out_i = sum_{j < n} s_ij P_j  for k scalar rows over the same n bases
// (the Groth16 verifier's evaluationABC of k proofs under one key; include/ozk.h, ozk_multi_msm_*).
//
// The variable-base pipeline (msm_var.hip) is built for ONE MSM of 2^20 pairs: sort, buckets, window sums and a
// Horner chain of ~120 dependent doublings, 0.7 ms of latency however small n is, and nothing amortised over k.
// With the bases fixed the fixed-base method (msm_fixed.hip) applies to every base at once: a window table per
// base, built once, after which an output is nothing but table gathers and mixed additions — no sort, no
// buckets, no doublings.
//
// Table (msm_multi.cuh): per base the affine records of d * 2^(w*ws) * P_j, signed digits (2^(ws-1) entries per
// window), one table of ceil(128 / ws) windows for both GLV halves.  Built in chunks of bases so that the
// Jacobian scratch stays small:
//   k_mm_chain    D[b][j] = 2^b P_j, one lane per base                        (the serial item: ~128 doublings)
//   k_mm_level k  entry 2^k + i = entry i + D[w*ws + k], all bases, windows and i in parallel
//   k_mm_affine   Jacobian -> affine, MM_BATCH entries per shared inversion
// Evaluation:
//   k_mm_eval     T = 2^t lanes per output, lane = (half, slice of the bases): recode in registers, gather,
//                 xyzz_madd_lazy; phi on the half-1 lanes' sums; shuffle tree over the lanes of one output
//   k_mm_parts    only when an output spans several waves (T > 64): one wave sums its partial records
//   k_mm_norm     affine normalisation, MM_BATCH outputs per shared inversion, 192-byte wire-out records
#include "msm_var.cuh"   // RunAcc (XYZZ accumulator), shfl_down_jac, glv_beta
#include "msm_multi.cuh"
#include "ozk_common.h"

namespace ozk {

using MmCV = G1Cfg;
using MmIO = CurveIO<MmCV>;
constexpr int MM_BATCH = 8;                              // entries per shared inversion
constexpr size_t MM_SCRATCH_BUDGET = (size_t)32 << 20;   // Jacobian scratch of one chunk of bases
constexpr long long MM_TARGET_LANES = 1ll << 18;         // lanes wanted in flight: 4096 waves, 4 per SIMD

__global__ void __launch_bounds__(64) k_mm_chain(const u32* __restrict__ bases_wire, int cnt, int total,
                                                 u32* __restrict__ D) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt) return;
  Jac<MmCV> p = MmIO::jac_from_wire(bases_wire + (size_t)t * MmIO::WIRE_JAC_WORDS);
  for (int b = 0; b < total; b++) {
    MmIO::store_jac(p, D + ((size_t)b * cnt + t) * MmIO::JAC_WORDS);
    p = jac_dbl(p);   // (infinity stays infinity: Z3 = 2 Y Z)
  }
}

// level k < ws - 1 (shift = k): digits d = 2^k + i, i < 2^k;  level ws - 1 (shift = 0): d = 2^(ws-1) alone
__global__ void __launch_bounds__(256) k_mm_level(u32* __restrict__ jt, const u32* __restrict__ D, int cnt, int oc,
                                                  int ws, int k, int shift) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ((size_t)cnt * oc) << shift) return;
  const u32 i = (u32)t & ((1u << shift) - 1u);
  const size_t rest = t >> shift;
  const int w = (int)(rest % oc);
  const size_t jb = rest / oc;
  const size_t row = (jb * oc + w) << (ws - 1);
  const Jac<MmCV> add = MmIO::load_jac(D + ((size_t)(w * ws + k) * cnt + jb) * MmIO::JAC_WORDS);
  Jac<MmCV> r = add;
  if (i != 0) r = jac_add(MmIO::load_jac(jt + (row + i - 1) * MmIO::JAC_WORDS), add);
  MmIO::store_jac(r, jt + (row + (1u << k) + i - 1) * MmIO::JAC_WORDS);
}

// lane t normalises entries t, t + lanes, ... (interleaved, as k_fb_table_affine); infinity -> (0, 0)
__global__ void __launch_bounds__(256) k_mm_affine(const u32* __restrict__ jac, size_t n, u32* __restrict__ aff) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t lanes = (n + MM_BATCH - 1) / MM_BATCH;
  if (t >= lanes) return;
  batch_normalise<MmCV, MM_BATCH>(jac, n, t, lanes, [&](size_t i, bool, const Aff<MmCV::EA>& q) {
    MmIO::store_aff(q, aff + i * MmIO::AFF_WORDS);
  });
}

__device__ __forceinline__ Aff<MmCV::EA> mm_load_record(const u32* p) {
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
  u32 w[MmIO::AFF_WORDS];
#pragma unroll
  for (int q = 0; q < MmIO::AFF_WORDS / 4; q++) {
    const uint4 v = p4[q];
    w[4 * q] = v.x;
    w[4 * q + 1] = v.y;
    w[4 * q + 2] = v.z;
    w[4 * q + 3] = v.w;
  }
  return MmIO::load_aff(w);
}

// tree sum over groups of L (a power of two <= 64) adjacent lanes; the group's lane 0 ends with the sum
__device__ __forceinline__ void mm_group_sum(Jac<MmCV>& r, int lg, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) {
    const Jac<MmCV> v = shfl_down_jac(r, o);
    const Jac<MmCV> s = jac_add(r, v);   // (complete: P = Q and P = -Q occur with repeated bases)
    if (lg < o) r = s;
  }
}

// T lanes per output (a power of two >= 2; a multiple of 64 or a divisor of 64).  Lane lt of an output: half
// h = lt & 1 of the GLV split, bases j = lt >> 1, + T / 2, ...  `parts`: one Jacobian record per (output, wave of
// the output), max(T / 64, 1) per output.
__global__ void __launch_bounds__(256) k_mm_eval(const u32* __restrict__ table, const u32* __restrict__ scalars, int n,
                                                 int k, int oc, int ws, int T, u32* __restrict__ parts) {
  using EA = MmCV::EA;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = g / (size_t)T;
  const int lt = (int)(g % (size_t)T);
  const int h = lt & 1;
  const int S = T >> 1;
  const bool live = i < (size_t)k;
  Aff<EA> inf;
  inf.x = EA(el_zero(inf.x));
  inf.y = EA(el_zero(inf.x));
  RunAcc<MmCV, true> acc;
  acc.start_q(inf);
  if (live) {
    const size_t per_base = (size_t)oc << (ws - 1);
    for (int j = lt >> 1; j < n; j += S) {
      u32 s[8];
      const uint4* sp = reinterpret_cast<const uint4*>(scalars + ((size_t)i * n + j) * 8);
      const uint4 a = sp[0], b = sp[1];
      s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
      s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
      u32 k1[4], k2[4];
      bool n1, n2;
      glv_decompose(s, k1, n1, k2, n2);
      const u32 kk0 = h ? k2[0] : k1[0], kk1 = h ? k2[1] : k1[1], kk2 = h ? k2[2] : k1[2], kk3 = h ? k2[3] : k1[3];
      const bool ng = h ? n2 : n1;
      const u32* tab = table + (size_t)j * per_base * MmIO::AFF_WORDS;
      u32 carry = 0;
      for (int w = 0; w < oc; w++) {
        const int d = mm_signed_digit(kk0, kk1, kk2, kk3, w, ws, carry);
        if (d != 0) {
          const u32 mag = (u32)(d < 0 ? -d : d);
          const Aff<EA> q = mm_load_record(tab + ((((size_t)w) << (ws - 1)) + mag - 1) * MmIO::AFF_WORDS);
          acc.accumulate_signed(q, (d < 0) != ng);
        }
      }
    }
  }
  Jac<MmCV> r = xyzz_to_jac(acc.a);
  // phi(X, Y, Z) = (beta X, Y, Z) on the sums of the second halves
  const MmCV::EX bx = MmCV::EX(reduce_to<32>(scale(r.X, glv_beta<MmCV>())));
  r.X = select_el(h != 0, bx, r.X);
  const int L = T < 64 ? T : 64;
  const int lg = lt & (L - 1);
  mm_group_sum(r, lg, L);
  if (live && lg == 0) {
    const size_t P = T > 64 ? (size_t)(T >> 6) : 1;
    MmIO::store_jac(r, parts + (i * P + (size_t)(lt >> 6)) * MmIO::JAC_WORDS);
  }
}

// one wave per output: the sum of its P partial records
__global__ void __launch_bounds__(64) k_mm_parts(const u32* __restrict__ parts, int k, int P, u32* __restrict__ sums) {
  const int i = blockIdx.x;
  if (i >= k) return;
  const int l = threadIdx.x;
  Jac<MmCV> r = jac_infinity<MmCV>();
  for (int p = l; p < P; p += 64) r = jac_add(r, MmIO::load_jac(parts + ((size_t)i * P + p) * MmIO::JAC_WORDS));
  mm_group_sum(r, l, 64);
  if (l == 0) MmIO::store_jac(r, sums + (size_t)i * MmIO::JAC_WORDS);
}

// k Jacobian sums -> wire-out records (64-byte little-endian coordinates, Z = 1; infinity (0, 1, 0)), as
// write_normalised (msm_var.cuh) with the inversion shared by MM_BATCH outputs
__global__ void __launch_bounds__(256) k_mm_norm(const u32* __restrict__ jac, int n, u32* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int lanes = (n + MM_BATCH - 1) / MM_BATCH;
  if (t >= lanes) return;
  batch_normalise<MmCV, MM_BATCH>(jac, n, t, lanes, [&](size_t i, bool inf, const Aff<MmCV::EA>& q) {
    MmIO::write_aff<WireOut>(inf, q, out + i * (3 * WireOut::FQ_WORDS));
  });
}

// ---- host side ---------------------------------------------------------------------------------
struct MmPlan {
  int ws, oc;
  size_t per_base;   // table records per base
  int chunk;         // bases per table-build chunk
};
static bool mm_shape_ok(int n, int type) { return type == OZK_G1 && n >= 1 && n <= MM_MAX_N; }
static bool mm_run_shape_ok(int n, int k, int type) {
  return mm_shape_ok(n, type) && k >= 1 && (long long)k * n <= MM_MAX_KN;
}
static MmPlan mm_plan(int n) {
  MmPlan p;
  p.ws = mm_window_bits(n);
  // OZK_MM_WS: the window size for measurements (read once, like every tuning switch: table and calls agree)
  const int forced = knob_or(K_MM_WS, p.ws);
  if (forced >= MM_WS_MIN && forced <= MM_WS_MAX) p.ws = forced;
  p.oc = mm_windows(p.ws);
  p.per_base = mm_records_per_base(p.ws);
  size_t c = MM_SCRATCH_BUDGET / (p.per_base * MmIO::JAC_WORDS * 4);
  if (c < 1) c = 1;
  p.chunk = c > (size_t)n ? n : (int)c;
  return p;
}
// lanes per output: enough of them to fill the device, never more than two per base
static int mm_lanes_per_output(int n, int k) {
  int cap = 2;
  while (cap < 2 * n) cap <<= 1;
  int T = 2;
  while (T < cap && (long long)(2 * T) * k <= MM_TARGET_LANES) T <<= 1;
  return T;
}
struct MmLayout {
  u32 *D, *jt, *parts, *sums;
  size_t bytes;
};
static MmLayout mm_layout(const MmPlan& p, int n, int k, void* wsp, size_t wsb) {
  (void)n;
  MmLayout L;
  // the table build and a run never overlap on a stream: their scratch shares the workspace
  Bump a(wsp, wsb);
  L.D = a.take<u32>((size_t)p.chunk * p.oc * p.ws * MmIO::JAC_WORDS);
  L.jt = a.take<u32>((size_t)p.chunk * p.per_base * MmIO::JAC_WORDS);
  const size_t build = a.off;
  Bump b(wsp, wsb);
  L.parts = L.sums = nullptr;
  if (k > 0) {
    const int T = mm_lanes_per_output(n, k);
    const size_t P = T > 64 ? T / 64 : 1;
    L.parts = b.take<u32>((size_t)k * P * MmIO::JAC_WORDS);
    L.sums = b.take<u32>((size_t)k * MmIO::JAC_WORDS);
  }
  L.bytes = (build > b.off ? build : b.off) + 256;
  return L;
}

}  // namespace ozk

using namespace ozk;

extern "C" {

int ozk_multi_msm_plan(int32_t n, int32_t* window_bits, int32_t* windows) {
  if (n < 1 || n > MM_MAX_N) return fail(OZK_E_INVALID, "multi MSM: n = %d out of range [1, %d]", n, MM_MAX_N);
  const MmPlan p = mm_plan(n);
  if (window_bits) *window_bits = p.ws;
  if (windows) *windows = p.oc;
  return OZK_OK;
}

size_t ozk_multi_msm_table_bytes(int32_t n, int32_t type) {
  if (!mm_shape_ok(n, type)) return 0;
  return (size_t)n * mm_plan(n).per_base * MmIO::AFF_WORDS * 4;
}

size_t ozk_multi_msm_workspace_bytes(int32_t n, int32_t k, int32_t type) {
  if (!mm_run_shape_ok(n, k, type)) return 0;
  return mm_layout(mm_plan(n), n, k, nullptr, 0).bytes;
}

int ozk_multi_msm_prepare_dev(const void* d_bases, int32_t n, int32_t type, void* d_table, size_t table_bytes,
                              void* d_workspace, size_t workspace_bytes, void* stream) {
  if (type != OZK_G1) return fail(OZK_E_INVALID, "multi MSM: G1 only (type %d)", type);
  if (!mm_shape_ok(n, type)) return fail(OZK_E_INVALID, "multi MSM: n = %d out of range [1, %d]", n, MM_MAX_N);
  if (!d_bases || !d_table || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  const MmPlan p = mm_plan(n);
  const size_t need_t = (size_t)n * p.per_base * MmIO::AFF_WORDS * 4;
  if (table_bytes < need_t) return fail(OZK_E_INVALID, "multi MSM: table too small: need %zu bytes, got %zu", need_t, table_bytes);
  const MmLayout L = mm_layout(p, n, 0, d_workspace, workspace_bytes);
  if (L.bytes > workspace_bytes)
    return fail(OZK_E_INVALID, "multi MSM: workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hip_clear_stale();
  hipStream_t st = (hipStream_t)stream;
  const int TB = 256;
  for (int j0 = 0; j0 < n; j0 += p.chunk) {
    const int cnt = n - j0 < p.chunk ? n - j0 : p.chunk;
    hipLaunchKernelGGL(k_mm_chain, dim3((cnt + 63) / 64), dim3(64), 0, st,
                       (const u32*)d_bases + (size_t)j0 * MmIO::WIRE_JAC_WORDS, cnt, p.oc * p.ws, L.D);
    for (int lv = 0; lv < p.ws; lv++) {
      const int shift = lv == p.ws - 1 ? 0 : lv;
      const size_t tot = ((size_t)cnt * p.oc) << shift;
      hipLaunchKernelGGL(k_mm_level, dim3((unsigned)((tot + TB - 1) / TB)), dim3(TB), 0, st, L.jt, L.D, cnt, p.oc, p.ws,
                         lv, shift);
    }
    const size_t entries = (size_t)cnt * p.per_base;
    const size_t tl = (entries + MM_BATCH - 1) / MM_BATCH;
    hipLaunchKernelGGL(k_mm_affine, dim3((unsigned)((tl + TB - 1) / TB)), dim3(TB), 0, st, L.jt, entries,
                       (u32*)d_table + (size_t)j0 * p.per_base * MmIO::AFF_WORDS);
  }
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_multi_msm_dev(const void* d_table, const void* d_scalars, int32_t n, int32_t k, int32_t type, void* d_out,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
  if (type != OZK_G1) return fail(OZK_E_INVALID, "multi MSM: G1 only (type %d)", type);
  if (!mm_run_shape_ok(n, k, type))
    return fail(OZK_E_INVALID, "multi MSM: shape n = %d, k = %d rejected (1 <= n <= %d, k >= 1, k n <= 2^28)", n, k, MM_MAX_N);
  if (!d_table || !d_scalars || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  const MmPlan p = mm_plan(n);
  const MmLayout L = mm_layout(p, n, k, d_workspace, workspace_bytes);
  if (L.bytes > workspace_bytes)
    return fail(OZK_E_INVALID, "multi MSM: workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hip_clear_stale();
  hipStream_t st = (hipStream_t)stream;
  const int TB = 256;
  const int T = mm_lanes_per_output(n, k);
  const int P = T > 64 ? T / 64 : 1;
  const size_t lanes = (size_t)k * T;
  hipLaunchKernelGGL(k_mm_eval, dim3((unsigned)((lanes + TB - 1) / TB)), dim3(TB), 0, st, (const u32*)d_table,
                     (const u32*)d_scalars, n, k, p.oc, p.ws, T, L.parts);
  const u32* sums = L.parts;
  if (P > 1) {
    hipLaunchKernelGGL(k_mm_parts, dim3(k), dim3(64), 0, st, L.parts, k, P, L.sums);
    sums = L.sums;
  }
  const int nl = (k + MM_BATCH - 1) / MM_BATCH;
  hipLaunchKernelGGL(k_mm_norm, dim3((nl + TB - 1) / TB), dim3(TB), 0, st, sums, k, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
