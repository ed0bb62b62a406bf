// BACE on the GPU: Williams' Merlin-Arthur proof for batch arithmetic-circuit evaluation (the reference's bace/
// package: Prover.computeProof, Verifier.verifyProof / getResult, NaiveEvaluator.getResult, Common.getInputPolynomials).
// A unit of its own: from fft.hip it takes the twiddle plans (domain_tables) and the tiled transform (fft_core, batched
// through in_cs / out_cs), declared in fft_plan.h; the evaluation at a point is fr_tables.cuh's.  DESIGN.md section 11.
//
//   n inputs per instance, N instances (a power of two), circuit degree deg, D = lowestPowerOfTwo(deg N).
//   prove:  beta_j = iFFT_N(column j); evaluations beta_j(omega_D^k) = FFT_D(beta_j zero-padded); R_k = C(beta(omega_D^k));
//           proof = iFFT_D(R) (D coefficients).
//   verify: claim = proof(r); accept iff claim == C(beta_1(r), ..., beta_n(r)).
//   result: FFT_D(proof) at every (D/N)-th point = FFT_N(proof folded mod z^N - 1).
//
// Every value in HBM is 32 bytes LE, plain (non-Montgomery) and canonical unless stated otherwise.
#include "fft_plan.h"
#include "fr_tables.cuh"

namespace ozk {

constexpr int BACE_LDS_FFT_MAX = 2048;      // transforms up to this size: one workgroup per column, column in LDS (64 KiB)
constexpr int BACE_WG = 64;                 // circuit interpreter: one wave per workgroup, one lane per point
constexpr int BACE_MAX_LANES = 65536;       // lanes of one interpreter launch (each loops over points beyond that)
constexpr int BACE_LDS_SLOTS_MAX = 28;      // 28 x 9 words x 64 lanes x 4 B = 63 KiB of LDS per workgroup
// (OZK_BACE_LDS_SLOTS defaults to 16 slots in LDS, 36 KiB: four workgroups per CU)
constexpr int BACE_MAX_N = 65535;           // columns: gridDim.y of the batched kernels
constexpr int BACE_OP_WORDS = 4;            // {op, dst, a, b}

// A primitive 2^28-th root of unity of Fr: FR_ROOT^((r - 1) / 2^28), so that Fp.rootOfUnity(n) = FR_ROOT^(r / n) =
// BACE_W28^(2^28 / n) for every power of two 2 <= n <= 2^28 (Fp.java:98-102); its inverse; and 1/2.
static const u32 BACE_W28[8] = {0x88590882u, 0xb8dde849u, 0x0e1a5d5du, 0x67cf5acdu,
                                0x723d5c5fu, 0xe1ed0cc8u, 0xc8953178u, 0x188c51b4u};
static const u32 BACE_W28_INV[8] = {0xe25ab83bu, 0x44c8eb25u, 0x9d2ac154u, 0xc66b9e1bu,
                                    0xb17a4c68u, 0xc023ff24u, 0xb5e12a84u, 0x18f27f93u};
static const u32 BACE_INV2[8] = {0xf8000001u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u,
                                 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};

// ---- host arithmetic (a few dozen operations per call) ----
// omega_n (inverse: omega_n^-1) as plain words: the 2^28-th root squared 28 - log2 n times
static void bace_root_host(int logn, bool inverse, u32 (&out)[8]) {
  u32 w[8];
  memcpy(w, inverse ? BACE_W28_INV : BACE_W28, 32);
  Fe<FrP, 32> a = Fe<FrP, 32>(to_mont<FrP>(w));
  for (int i = logn; i < 28; i++) a = Fe<FrP, 32>(sqr(a));
  from_mont(a, out);
}
// 2^-k, Montgomery form (mont = true) or plain
static void bace_inv_pow2_host(int k, bool mont, u32 (&out)[8]) {
  u32 w[8];
  memcpy(w, BACE_INV2, 32);
  const Fe<FrP, 32> h = Fe<FrP, 32>(to_mont<FrP>(w));
  Fe<FrP, 32> a = Fe<FrP, 32>(fe_one<FrP>());
  for (int i = 0; i < k; i++) a = Fe<FrP, 32>(mul(a, h));
  if (mont) pack(canonical(a), out);
  else from_mont(a, out);
}

// ---- the columns ----
// out[j N + k] = in[k n + j] / N (row-major instances -> column-major, with the 1/N of the inverse transforms that
// follow: the transform is linear, so scaling its input is the same as scaling its output).  k_mont = (1/N) R.
__global__ void __launch_bounds__(256) k_bace_to_cols(const u32* __restrict__ in, int n, int N,
                                                      const u32* __restrict__ k_mont, u32* __restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * N) return;
  const long long j = t / N, k = t % N;
  const auto x = fr_load<85>(in + ((size_t)k * n + (size_t)j) * 8);
  fr_store(canonical(mul(x, ElemTraits<Fe<FrP, 16>>::load(k_mont))), out + (size_t)t * 8);
}

// ---- transforms up to BACE_LDS_FFT_MAX: one workgroup per column, the whole column in LDS ----
// The algorithm of k_fft_small (bit reversal, then log2 n radix-2 stages over the plain twiddle table tw[t] =
// omega^t, t < n/2, Montgomery form) with the column in LDS instead of global scratch.  Column c reads
// in + c in_cs and writes out + c out_cs (words); in == out is allowed (the column is read whole before any write).
__global__ void __launch_bounds__(256) k_bace_fft_lds(const u32* in, size_t in_cs, u32* out, size_t out_cs,
                                                      const u32* __restrict__ tw, int n, int logn) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];  // n x 8 words, values < 2p
  using ET = ElemTraits<Fe<FrP, 32>>;
  const u32* src = in + (size_t)blockIdx.x * in_cs;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int s = logn ? (int)(__brev((unsigned)i) >> (32 - logn)) : 0;
    u32 o[8];
    pack(canonical(fr_load<85>(src + (size_t)s * 8)), o);
#pragma unroll
    for (int k = 0; k < 8; k++) lds[i * 8 + k] = o[k];
  }
  block_sync();
  for (int s = 1; s <= logn; s++) {
    const int m = 1 << (s - 1);
    for (int b = threadIdx.x; b < n / 2; b += 256) {
      const int j = b & (m - 1);
      const int k0 = ((b >> (s - 1)) << s) | j;
      const auto w = ElemTraits<Fe<FrP, 16>>::load(tw + (size_t)((long long)j << (logn - s)) * 8);
      const auto x = ET::load(lds + k0 * 8);
      const auto y = ET::load(lds + (k0 + m) * 8);
      const auto t = mul(w, y);
      u32 o[8];
      pack(Fe<FrP, 32>(reduce_to<32>(add(x, t))), o);
#pragma unroll
      for (int k = 0; k < 8; k++) lds[k0 * 8 + k] = o[k];
      pack(Fe<FrP, 32>(reduce_to<32>(sub(x, t))), o);
#pragma unroll
      for (int k = 0; k < 8; k++) lds[(k0 + m) * 8 + k] = o[k];
    }
    block_sync();
  }
  u32* dst = out + (size_t)blockIdx.x * out_cs;
  for (int i = threadIdx.x; i < n; i += 256) fr_store(canonical(ET::load(lds + i * 8)), dst + (size_t)i * 8);
}

// ---- the circuit interpreter ----
// The program (include/ozk.h, "BACE programs"): n_ops records {op, dst, a, b} of int32, read uniformly by every lane.
//   op 0 INPUT: slot dst <- input a of the point     op 1 CONST: slot dst <- constant a
//   op 2 ADD:   slot dst <- slot a + slot b          op 3 MUL:   slot dst <- slot a * slot b
// The value of the last record is the circuit's output.  Slots hold Montgomery-form values < 2p: slots below
// lds_slots in LDS (limb-major, 9 words per slot, conflict-free across the wave), the others in a slot-major HBM
// scratch (slot s of lane g at hbm + ((s - lds_slots) lanes + g) 8 words: a wave's 64 lanes touch 2 KiB contiguously).
struct BaceEval {
  const u32* in;
  size_t pstride, jstride;   // input a of point p: in + p pstride + a jstride (words)
  int npoints;
  const int4* prog;
  int n_ops;
  const u32* consts;         // Montgomery form, 8 words each
  int lds_slots;
  u32* hbm;
  int lanes;                 // gridDim.x x BACE_WG
  const u32* k_out;          // plain: out[p] = C(point p) k_out (1/D for the prover, 1 for the evaluators)
  u32* out;                  // npoints x 8 words
};
using BaceV = Fe<FrP, 32>;

__device__ __forceinline__ BaceV bace_slot_get(const BaceEval& e, const u32* lds, int s, int g) {
  if (s < e.lds_slots) {
    BaceV v;
#pragma unroll
    for (int i = 0; i < 9; i++) v.l[i] = lds[(s * 9 + i) * BACE_WG + threadIdx.x];
    return v;
  }
  return fr_load<32>(e.hbm + ((size_t)(s - e.lds_slots) * e.lanes + g) * 8);
}
__device__ __forceinline__ void bace_slot_put(const BaceEval& e, u32* lds, int s, int g, const BaceV& v) {
  if (s < e.lds_slots) {
#pragma unroll
    for (int i = 0; i < 9; i++) lds[(s * 9 + i) * BACE_WG + threadIdx.x] = v.l[i];
    return;
  }
  fr_store(v, e.hbm + ((size_t)(s - e.lds_slots) * e.lanes + g) * 8);
}

__global__ void __launch_bounds__(BACE_WG) k_bace_circuit(BaceEval e) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];  // lds_slots x 9 x BACE_WG words
  const int g = blockIdx.x * BACE_WG + threadIdx.x;
  const auto r2 = fe_const<FrP, 16>(FrP::R2);
  const auto ko = ElemTraits<Fe<FrP, 16>>::load(e.k_out);
  for (int p = g; p < e.npoints; p += e.lanes) {
    BaceV last = BaceV(fe_zero<FrP>());
    for (int t = 0; t < e.n_ops; t++) {
      const int4 op = e.prog[t];
      BaceV v;
      if (op.x == 0) {
        v = BaceV(mul(fr_load<85>(e.in + (size_t)p * e.pstride + (size_t)op.z * e.jstride), r2));
      } else if (op.x == 1) {
        v = BaceV(ElemTraits<Fe<FrP, 16>>::load(e.consts + (size_t)op.z * 8));
      } else if (op.x == 2) {
        v = BaceV(reduce_to<32>(add(bace_slot_get(e, lds, op.z, g), bace_slot_get(e, lds, op.w, g))));
      } else {
        v = BaceV(mul(bace_slot_get(e, lds, op.z, g), bace_slot_get(e, lds, op.w, g)));
      }
      bace_slot_put(e, lds, op.y, g, v);
      last = v;
    }
    fr_store(canonical(mul(last, ko)), e.out + (size_t)p * 8);   // Montgomery x plain = plain
  }
}

// ---- result extraction: f[i] = sum_k proof[i + k N], k < D / N (the proof folded mod z^N - 1) ----
__global__ void __launch_bounds__(256) k_bace_fold(const u32* __restrict__ proof, int D, int N, u32* __restrict__ f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int k = i; k < D; k += N) acc = FrAcc(reduce_to<32>(add(acc, fr_load<85>(proof + (size_t)k * 8))));
  fr_store(canonical(acc), f + (size_t)i * 8);
}

// ---- host side ----
static int bace_lds_slot_cap() {
  int cap = knob(K_BACE_LDS_SLOTS);
  if (cap < 0) cap = 0;
  if (cap > BACE_LDS_SLOTS_MAX) cap = BACE_LDS_SLOTS_MAX;
  return cap;
}
static int bace_lanes(int npoints) {
  const int l = (npoints + BACE_WG - 1) / BACE_WG * BACE_WG;
  return l < BACE_MAX_LANES ? l : BACE_MAX_LANES;
}

struct BaceLayout {
  u32 *cst;                      // [0] 1/N (Montgomery)  [8] 1/D (plain)  [16] 1 (plain)  [24] r (Montgomery)
  DomainTables dom;              // consts->omega and small of the per-call twiddle builds (without the plan cache)
  u32 *tw[4];                    // omega_N^-1, omega_N, omega_D, omega_D^-1: n/2 ... pyramids of N or D entries
  u32 *cols, *lde, *vals, *buf0, *buf1, *partial;
  int4* prog;
  u32 *consts, *hbm;
  size_t bytes;
};
static size_t bace_hbm_words(int n_slots, int npoints) {
  const int spill = n_slots - bace_lds_slot_cap();
  return spill > 0 ? (size_t)spill * bace_lanes(npoints) * 8 : 0;
}
// n columns, N instances, D evaluation points; n_ops / n_slots / n_consts of the program (0: no circuit step), run at
// npoints points.  (The slot scratch follows the LDS slot cap in force: query the size right before the call.)
static BaceLayout bace_layout(int n, int N, int D, int n_ops, int n_slots, int n_consts, int npoints, void* wsp) {
  BaceLayout L;
  Bump b(wsp, ~(size_t)0);
  L.cst = b.take<u32>(64);
  L.dom = DomainTables{};
  carve_head(b, PowTable::twiddles(fft_half(D)), L.dom);
  L.tw[0] = b.take<u32>((size_t)N * 8);
  L.tw[1] = b.take<u32>((size_t)N * 8);
  L.tw[2] = b.take<u32>((size_t)D * 8);
  L.tw[3] = b.take<u32>((size_t)D * 8);
  L.cols = b.take<u32>((size_t)n * N * 8);
  L.lde = b.take<u32>((size_t)n * D * 8);
  L.vals = b.take<u32>((size_t)D * 8);
  L.buf0 = b.take<u32>((size_t)n * D * 8);
  L.buf1 = b.take<u32>((size_t)n * D * 8);
  L.partial = b.take<u32>((size_t)(n > 1 ? n : 1) * 256 * 8);
  L.prog = b.take<int4>(n_ops > 0 ? n_ops : 1);
  L.consts = b.take<u32>((size_t)(n_consts > 0 ? n_consts : 1) * 8);
  L.hbm = b.take<u32>(bace_hbm_words(n_slots, npoints));
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}

// the twiddle table of omega_size (or its inverse): from the plan cache (pinned in `pin`), else built per call in `slot`
static int bace_twiddles(int size, bool inverse, const BaceLayout& L, u32* slot, PlanPin& pin, hipStream_t st,
                         const u32** tw) {
  u32 om[8];
  bace_root_host(ilog2((uint32_t)size), inverse, om);
  DomainTables t = L.dom;
  *tw = t.tw_f = slot;
  if (size < 2) return OZK_OK;   // (a transform of one element reads no twiddle)
  // (om is a temporary: by value)
  const int rc = domain_tables(size, (const uint8_t*)om, nullptr, true, &t, pin, st);
  *tw = t.tw_f;
  return rc;
}

// `batch` columns of `size` elements: column c from in + c in_cs to out + c out_cs (words), one pipeline of launches
// whatever the batch.  Up to BACE_LDS_FFT_MAX: k_bace_fft_lds; above: the tiled passes through buf0 / buf1
// (batch x size x 8 words each).  out may equal in: above BACE_LDS_FFT_MAX a transform takes at least two passes
// (at most 10 stages each), and only the first reads `in`, only the last writes `out`.
static int bace_transform(const u32* in, size_t in_cs, u32* out, size_t out_cs, int size, int batch, const u32* tw,
                          u32* buf0, u32* buf1, hipStream_t st) {
  const int logn = ilog2((uint32_t)size);
  if (size <= BACE_LDS_FFT_MAX) {
    hipLaunchKernelGGL(k_bace_fft_lds, dim3(batch), dim3(256), (size_t)size * 32, st, in, in_cs, out, out_cs, tw, size,
                       logn);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  }
  return fft_core(in, size, tw, out, 8, buf0, buf1, st, nullptr, batch, in_cs, out_cs);
}

// the circuit at `npoints` points: input a of point p at in + p pstride + a jstride (words)
static int bace_eval(const BaceLayout& L, const u32* in, size_t pstride, size_t jstride, int npoints, int n_ops,
                     int n_slots, const u32* k_out, u32* out, hipStream_t st) {
  const int cap = bace_lds_slot_cap();
  BaceEval e;
  e.in = in;
  e.pstride = pstride;
  e.jstride = jstride;
  e.npoints = npoints;
  e.prog = L.prog;
  e.n_ops = n_ops;
  e.consts = L.consts;
  e.lds_slots = n_slots < cap ? n_slots : cap;
  e.hbm = L.hbm;
  e.lanes = bace_lanes(npoints);
  e.k_out = k_out;
  e.out = out;
  hipLaunchKernelGGL(k_bace_circuit, dim3(e.lanes / BACE_WG), dim3(BACE_WG), (size_t)e.lds_slots * 9 * BACE_WG * 4, st, e);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

// checks a host program against n inputs, n_slots slots and n_consts constants (every record, so that the kernel never
// reads or writes outside its slots, inputs or constants), then uploads it and the constants (Montgomery form)
static int bace_upload_program(const BaceLayout& L, const int32_t* program, int n_ops, int n_slots, const uint8_t* consts,
                               int n_consts, int n, hipStream_t st) {
  if (!program || n_ops <= 0 || n_slots <= 0 || n_consts < 0 || (n_consts > 0 && !consts))
    return fail(OZK_E_INVALID, "bad program arguments");
  for (int t = 0; t < n_ops; t++) {
    const int32_t* r = program + (size_t)t * BACE_OP_WORDS;
    const int op = r[0], dst = r[1], a = r[2], b = r[3];
    bool ok = op >= 0 && op <= 3 && dst >= 0 && dst < n_slots;
    if (op == 0) ok = ok && a >= 0 && a < n;
    else if (op == 1) ok = ok && a >= 0 && a < n_consts;
    else ok = ok && a >= 0 && a < n_slots && b >= 0 && b < n_slots;
    if (!ok) return fail(OZK_E_INVALID, "program record %d {%d, %d, %d, %d} is malformed", t, op, dst, a, b);
  }
  OZK_HIP(hipMemcpyAsync(L.prog, program, (size_t)n_ops * 16, hipMemcpyHostToDevice, st));
  if (n_consts > 0) {
    OZK_HIP(hipMemcpyAsync(L.consts, consts, (size_t)n_consts * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_to_mont_inplace, dim3((n_consts + 255) / 256), dim3(256), 0, st, L.consts, n_consts);
  }
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

// the constant block L.cst: 1/N (Montgomery), 1/D (plain), 1 (plain), and r (Montgomery) when r_host32 is given
static int bace_upload_consts(const BaceLayout& L, int N, int D, const uint8_t* r_host32, hipStream_t st) {
  FrWords<4> c;
  memset(c.w, 0, sizeof(c.w));
  u32 t[8];
  bace_inv_pow2_host(ilog2((uint32_t)N), true, t);
  memcpy(c.w, t, 32);
  bace_inv_pow2_host(ilog2((uint32_t)D), false, t);
  memcpy(c.w + 8, t, 32);
  c.w[16] = 1;
  if (r_host32) memcpy(c.w + 24, r_host32, 32);
  hipLaunchKernelGGL(k_fr_put<4>, dim3(1), dim3(64), 0, st, c, 32, L.cst);
  if (r_host32) hipLaunchKernelGGL(k_to_mont_inplace, dim3(1), dim3(64), 0, st, L.cst + 24, 1);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

// beta_j = iFFT_N(column j) for all j into L.lde with column stride out_cs (coefficients, padded by the caller)
static int bace_columns(const BaceLayout& L, const void* d_inputs, int n, int N, size_t out_cs, PlanPin& pin,
                        hipStream_t st) {
  const u32* tw = nullptr;
  int rc = bace_twiddles(N, true, L, L.tw[0], pin, st, &tw);
  if (rc) return rc;
  const long long tot = (long long)n * N;
  hipLaunchKernelGGL(k_bace_to_cols, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const u32*)d_inputs, n, N,
                     L.cst, L.cols);
  OZK_HIP(hipGetLastError());
  return bace_transform(L.cols, (size_t)N * 8, L.lde, out_cs, N, n, tw, L.buf0, L.buf1, st);
}

static int bace_check_shape(int n, int N, int D) {
  if (n <= 0 || n > BACE_MAX_N) return fail(OZK_E_INVALID, "input count %d out of range [1, %d]", n, BACE_MAX_N);
  if (int rc = check_pow2(N, 1, "instance count")) return rc;
  if (D < N || (D & (D - 1)) || D > (1 << 28))
    return fail(OZK_E_INVALID, "D = %d is not a power of two in [N, 2^28] (N = %d)", D, N);
  return OZK_OK;
}

}  // namespace ozk

using namespace ozk;

extern "C" {

size_t ozk_bace_workspace_bytes(int32_t n, int32_t N, int32_t D, int32_t n_ops, int32_t n_slots, int32_t n_consts) {
  if (n <= 0 || n > BACE_MAX_N || N <= 0 || (N & (N - 1)) || D < N || (D & (D - 1)) || D > (1 << 28) || n_ops < 0 ||
      n_slots < 0 || n_consts < 0)
    return 0;
  return bace_layout(n, N, D, n_ops, n_slots, n_consts, D, nullptr).bytes;
}

size_t ozk_bace_evaluate_workspace_bytes(int32_t rows, int32_t n_ops, int32_t n_slots, int32_t n_consts) {
  if (rows <= 0 || rows > (1 << 28) || n_ops < 0 || n_slots < 0 || n_consts < 0) return 0;
  return bace_layout(1, 1, 1, n_ops, n_slots, n_consts, rows, nullptr).bytes;
}

int ozk_bace_prove_dev(const void* d_inputs, int32_t n, int32_t N, const int32_t* program, int32_t n_ops,
                       int32_t n_slots, const uint8_t* consts, int32_t n_consts, int32_t D, void* d_proof,
                       void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_inputs || !d_proof || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  int rc = bace_check_shape(n, N, D);
  if (rc) return rc;
  const BaceLayout L = bace_layout(n, N, D, n_ops, n_slots, n_consts, D, d_workspace);
  if (L.bytes > workspace_bytes) return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = bace_upload_program(L, program, n_ops, n_slots, consts, n_consts, n, st))) return rc;
  if ((rc = bace_upload_consts(L, N, D, nullptr, st))) return rc;
  PlanPin pin_n, pin_f, pin_i;   // held until the last launch reading the tables is enqueued
  // 1. beta_j, zero-padded to D   2. their evaluations at omega_D^k, in place
  if (D > N) OZK_HIP(hipMemset2DAsync(L.lde + (size_t)N * 8, (size_t)D * 32, 0, (size_t)(D - N) * 32, n, st));
  if ((rc = bace_columns(L, d_inputs, n, N, (size_t)D * 8, pin_n, st))) return rc;
  const u32 *tw_f = nullptr, *tw_i = nullptr;
  if ((rc = bace_twiddles(D, false, L, L.tw[2], pin_f, st, &tw_f))) return rc;
  if ((rc = bace_transform(L.lde, (size_t)D * 8, L.lde, (size_t)D * 8, D, n, tw_f, L.buf0, L.buf1, st))) return rc;
  // 3. R(omega_D^k) / D = C(beta(omega_D^k)) / D   4. the D coefficients of R
  if ((rc = bace_eval(L, L.lde, 8, (size_t)D * 8, D, n_ops, n_slots, L.cst + 8, L.vals, st))) return rc;
  if ((rc = bace_twiddles(D, true, L, L.tw[3], pin_i, st, &tw_i))) return rc;
  return bace_transform(L.vals, 0, (u32*)d_proof, 0, D, 1, tw_i, L.buf0, L.buf1, st);
}

int ozk_bace_evaluate_dev(const void* d_inputs, int32_t n, int32_t rows, const int32_t* program, int32_t n_ops,
                          int32_t n_slots, const uint8_t* consts, int32_t n_consts, void* d_out, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_inputs || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  if (n <= 0 || n > BACE_MAX_N || rows <= 0 || rows > (1 << 28)) return fail(OZK_E_INVALID, "bad shape n = %d, rows = %d", n, rows);
  const BaceLayout L = bace_layout(1, 1, 1, n_ops, n_slots, n_consts, rows, d_workspace);
  if (L.bytes > workspace_bytes) return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  int rc = bace_upload_program(L, program, n_ops, n_slots, consts, n_consts, n, st);
  if (rc) return rc;
  if ((rc = bace_upload_consts(L, 1, 1, nullptr, st))) return rc;
  return bace_eval(L, (const u32*)d_inputs, (size_t)n * 8, 8, rows, n_ops, n_slots, L.cst + 16, (u32*)d_out, st);
}

int ozk_bace_columns_at_dev(const void* d_inputs, int32_t n, int32_t N, const uint8_t* r_host32, void* d_out,
                            void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_inputs || !r_host32 || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  int rc = bace_check_shape(n, N, N);
  if (rc) return rc;
  const BaceLayout L = bace_layout(n, N, N, 0, 0, 0, 0, d_workspace);
  if (L.bytes > workspace_bytes) return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = bace_upload_consts(L, N, N, r_host32, st))) return rc;
  PlanPin pin;
  if ((rc = bace_columns(L, d_inputs, n, N, (size_t)N * 8, pin, st))) return rc;
  fr_poly_eval(L.lde, (size_t)N * 8, N, n, L.cst + 24, L.partial, (u32*)d_out, st);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_bace_result_dev(const void* d_proof, int32_t D, int32_t N, void* d_out, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
  hip_clear_stale();
  if (!d_proof || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  int rc = bace_check_shape(1, N, D);
  if (rc) return rc;
  const BaceLayout L = bace_layout(1, N, N, 0, 0, 0, 0, d_workspace);
  if (L.bytes > workspace_bytes) return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", L.bytes, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bace_fold, dim3((N + 255) / 256), dim3(256), 0, st, (const u32*)d_proof, D, N, L.vals);
  OZK_HIP(hipGetLastError());
  PlanPin pin;
  const u32* tw = nullptr;
  if ((rc = bace_twiddles(N, false, L, L.tw[1], pin, st, &tw))) return rc;
  return bace_transform(L.vals, 0, (u32*)d_out, 0, N, 1, tw, L.buf0, L.buf1, st);
}

}  // extern "C"
