// The two kernels that make a PLONK proof zero-knowledge: the blinders of coefficient rows, and
// the split of the quotient into its three blinded parts.  A section of the plonk.hip unit, which alone includes it,
// after plonk_r1cs.cuh.  Everything else of a zero-knowledge proof is the kernels of plonk.cuh, plonk_lookup.cuh and
// the KZG unit at rows of n + 8 coefficients.  Values in HBM are 32 bytes LE, plain; inputs are taken mod r, outputs
// are canonical.  The blinders arrive in host memory and travel in the kernel arguments: nothing is uploaded.
//
// Blind.  Row y of k gets counts[y] <= 4 blinders r_0 ..: row[j] -= r_j and row[n + j] = r_j, which adds
// (r_0 + r_1 X + ..)(X^n - 1) to the polynomial and so leaves its values on the domain of n points as they are.  One
// lane per (row, j): at most 4 k <= 32 lanes of one workgroup; no lane touches an element another one does (n >= 4).
//   bytes per blinder: 32 read, 64 written.
//
// Split.  One lane per column c < max(out_stride, 2 n) takes that column of the three output rows: it reads t[c],
// t[n + c] (c < n) and t[2 n + c] (c < 2 n), every coefficient of t once, and writes
//   t_lo'[c]  = t[c], then u_0, u_1 at n, n + 1;
//   t_mid'[c] = t[n + c] - u_c (c < 2), then v_0, v_1 at n, n + 1;
//   t_hi'[c]  = t[2 n + c] - v_c (c < 2) for c < n + 6,
// zero up to out_stride.  A coefficient t[2 n + c], c >= n + 6, is not written anywhere: it is counted when it is not
// zero (a ballot per wave, one atomic per workgroup that has any).
//   bytes: 4 n x 32 read, 3 out_stride x 32 written.
#pragma once
#include "plonk_r1cs.cuh"

namespace ozk {

constexpr int ZK_ROW_BLINDERS = 4;            // the most blinders of one row
constexpr int ZK_BLIND_ROWS = 8;              // the most rows of one call: 32 elements of kernel arguments
constexpr int ZK_PAD = 8;                     // a row of a zero-knowledge key has n + ZK_PAD coefficients
constexpr int ZK_T_COEFFS = 6;                // t has at most 3 n + ZK_T_COEFFS coefficients
constexpr int ZK_SPLIT_WG = 256;

#if defined(__HIPCC__)
struct ZkBlindArgs {
  FrWords<ZK_BLIND_ROWS * ZK_ROW_BLINDERS> r;   // slot 4 y + j: blinder j of row y, canonical
  int count[ZK_BLIND_ROWS];
};

__global__ void __launch_bounds__(64) k_fr_rows_blind(u32* __restrict__ rows, int k, int n, size_t cs, ZkBlindArgs a) {
  const int y = threadIdx.x / ZK_ROW_BLINDERS, j = threadIdx.x % ZK_ROW_BLINDERS;
  if (y >= k || j >= a.count[y]) return;
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.r.w[8 * threadIdx.x + i];
  u32* row = rows + (size_t)y * cs;
  const KzgV head = KzgV(reduce_to<32>(fr_load<85>(row + (size_t)j * 8)));
  fr_store(canonical(sub(head, unpack<FrP, 16>(w))), row + (size_t)j * 8);
  fr_store_words(w, row + ((size_t)n + j) * 8);
}

struct ZkSplitArgs {
  FrArg u[2], v[2];   // canonical
};

// b[c] for c < 2, zero beyond (c is the lane's own: no indexing of the arguments by it)
__device__ __forceinline__ Fe<FrP, 16> zk_low(const FrArg (&b)[2], unsigned c) {
  Fe<FrP, 16> r = Fe<FrP, 16>(fe_zero<FrP>());
  if (c == 0) r = plonk_arg(b[0]);
  if (c == 1) r = plonk_arg(b[1]);
  return r;
}

__global__ void __launch_bounds__(ZK_SPLIT_WG) k_plonk_quotient_split(const u32* __restrict__ t, unsigned n,
                                                                     u32* __restrict__ out, unsigned out_stride,
                                                                     ZkSplitArgs a, int* __restrict__ nonzero) {
  __shared__ int waves[ZK_SPLIT_WG / 64];
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t cs = (size_t)out_stride * 8;
  const bool writes = c < out_stride;
  const Fe<FrP, 16> zero = Fe<FrP, 16>(fe_zero<FrP>());
  Fe<FrP, 16> lo = zero, mid = zero, hi = zero;
  bool extra = false;
  if (c < n) {
    lo = canonical(fr_load<85>(t + (size_t)c * 8));
    mid = canonical(sub(KzgV(reduce_to<32>(fr_load<85>(t + ((size_t)n + c) * 8))), zk_low(a.u, c)));
  } else {
    lo = zk_low(a.u, c - n);
    mid = zk_low(a.v, c - n);
  }
  if (c < 2 * n) {
    const KzgV x = KzgV(reduce_to<32>(fr_load<85>(t + ((size_t)2 * n + c) * 8)));
    if (c < n + ZK_T_COEFFS) hi = canonical(sub(x, zk_low(a.v, c)));
    else extra = !is_zero(x);
  }
  if (writes) {
    fr_store(lo, out + (size_t)c * 8);
    fr_store(mid, out + cs + (size_t)c * 8);
    fr_store(hi, out + 2 * cs + (size_t)c * 8);
  }
  const unsigned long long found = __ballot(extra);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = __popcll(found);
  block_sync();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int i = 0; i < ZK_SPLIT_WG / 64; i++) sum += waves[i];
    if (sum) atomicAdd(nonzero, sum);
  }
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

int ozk_fr_rows_blind_dev(void* d_rows, int32_t k, int32_t n, int64_t stride, const uint8_t* blinders_host,
                          const int32_t* counts_host, void* stream) {
  hip_clear_stale();
  if (k < 1 || k > ZK_BLIND_ROWS || n < ZK_ROW_BLINDERS || (long long)n + ZK_ROW_BLINDERS > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad shape: %d rows of n = %d (1 <= k <= %d, %d <= n, n + %d <= 2^28)", k, n, ZK_BLIND_ROWS,
                ZK_ROW_BLINDERS, ZK_ROW_BLINDERS);
  if (stride < (long long)n + ZK_ROW_BLINDERS || (long long)k * stride > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad stride: %lld (>= n + %d = %d, k stride <= 2^28)", (long long)stride, ZK_ROW_BLINDERS,
                n + ZK_ROW_BLINDERS);
  if (int rc = fr_check_pointers(d_rows, blinders_host, counts_host)) return rc;
  if (int rc = fr_check_aligned16(d_rows)) return rc;
  ZkBlindArgs a;
  memset(&a, 0, sizeof a);
  const uint8_t* next = blinders_host;
  for (int y = 0; y < k; y++) {
    if (counts_host[y] < 0 || counts_host[y] > ZK_ROW_BLINDERS)
      return fail(OZK_E_INVALID, "row %d: %d blinders (0 .. %d)", y, counts_host[y], ZK_ROW_BLINDERS);
    a.count[y] = counts_host[y];
    for (int j = 0; j < counts_host[y]; j++, next += 32) {
      const FrArg r = plonk_plain(next);
      memcpy(a.r.w + 8 * (ZK_ROW_BLINDERS * y + j), r.w, 32);
    }
  }
  hipLaunchKernelGGL(k_fr_rows_blind, dim3(1), dim3(64), 0, (hipStream_t)stream, (u32*)d_rows, k, n, (size_t)stride * 8, a);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_plonk_quotient_split_dev(const void* d_t, int32_t n, void* d_out, int64_t out_stride, const uint8_t* blinders_host128,
                                 int32_t* d_nonzero, void* stream) {
  hip_clear_stale();
  if (n < ZK_PAD || (n & (n - 1)) || n > (1 << 26))
    return fail(OZK_E_INVALID, "n = %d is not a power of two in [%d, 2^26]", n, ZK_PAD);
  if (out_stride < (long long)n + ZK_PAD || 3 * out_stride > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad stride: out_stride %lld (>= n + %d = %d, 3 out_stride <= 2^28)", (long long)out_stride,
                ZK_PAD, n + ZK_PAD);
  if (int rc = fr_check_pointers(d_t, d_out, blinders_host128, d_nonzero)) return rc;
  if (int rc = fr_check_aligned16(d_t, d_out)) return rc;
  if (lookup_misaligned4(d_nonzero)) return fail(OZK_E_INVALID, "d_nonzero must be 4-byte aligned");
  const size_t t_bytes = (size_t)4 * n * 32, out_bytes = (size_t)3 * out_stride * 32;
  if (kzg_overlap(d_t, t_bytes, d_out, out_bytes)) return fail(OZK_E_INVALID, "d_out overlaps d_t");
  if (kzg_overlap(d_t, t_bytes, d_nonzero, 4) || kzg_overlap(d_out, out_bytes, d_nonzero, 4))
    return fail(OZK_E_INVALID, "d_nonzero overlaps d_t or d_out");
  ZkSplitArgs a;
  for (int j = 0; j < 2; j++) {
    a.u[j] = plonk_plain(blinders_host128 + 32 * j);
    a.v[j] = plonk_plain(blinders_host128 + 64 + 32 * j);
  }
  hipStream_t st = (hipStream_t)stream;
  const long long columns = out_stride > 2ll * n ? (long long)out_stride : 2ll * n;
  OZK_HIP(hipMemsetAsync(d_nonzero, 0, 4, st));
  hipLaunchKernelGGL(k_plonk_quotient_split, dim3((unsigned)((columns + ZK_SPLIT_WG - 1) / ZK_SPLIT_WG)), dim3(ZK_SPLIT_WG), 0,
                     st, (const u32*)d_t, (unsigned)n, (u32*)d_out, (unsigned)out_stride, a, (int*)d_nonzero);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
