// The Fr kernels of the KZG multi-opening: a weighted sum of rows per GROUP of rows, the groups
// any partition of the rows, and the values of every row at its own t points without a quotient.  A section of the
// kzg.hip unit, which alone includes it: kernels, layouts and entry points, after kzg_set.cuh, whose first pass and scan
// it runs as they are.
//
// Grouped combine.  out[g][j] = sum_{i : id[i] = g} w_i rows[i][j].  One lane per column, the group on the grid's
// second dimension; the ids travel in the kernel arguments, so that `id[i] == g` is uniform over the wave and a row
// that is not of the group costs a scalar compare and no load.  Every input element is read by exactly one workgroup
// and every output element written once, whatever the grouping.
//   products per input element: 1 (by the weight), and 1 per output element (by R^2); bytes: 32 read per input
//   element, 32 written per output element.
//
// Values at a set.  The first pass of section 23 leaves the value of every tile at every point (the tile is read
// once), the scan of section 22 turns those into the tails above every tile, and p(z_i) = (the value of tile 0) +
// z_i^KZG_TILE (the tail above it).  Nothing here divides by a difference of points, so the points of a row may repeat.
//   products per coefficient: t (1 + 8 / KZG_L); bytes: 32 read for any t.
#pragma once
#include "kzg_set.cuh"

namespace ozk {

constexpr int KZG_MULTI_ROWS = 256;     // rows of a grouped combine
constexpr int KZG_MULTI_GROUPS = 32;    // groups of a grouped combine

#if defined(__HIPCC__)
struct KzgGroupIds {   // the group of every row: 256 bytes of kernel arguments
  u32 w[KZG_MULTI_ROWS / 4];
};
__device__ __forceinline__ int kzg_group_of(const KzgGroupIds& ids, int i) { return (ids.w[i >> 2] >> (8 * (i & 3))) & 0xff; }

// out[g][j] = sum_{i : id[i] = g} w_i rows[i][j]: k_fr_rows_combine's arithmetic over the rows of group g = blockIdx.y
__global__ void __launch_bounds__(256) k_fr_rows_combine_groups(const u32* __restrict__ rows, int k, int len, size_t row_cs,
                                                                const u32* __restrict__ weights, KzgGroupIds ids,
                                                                u32* __restrict__ out, size_t out_cs) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (j >= len) return;
  // x w / R per term; the sum times R^2 / R at the end
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = 0; i < k; i++) {
    if (kzg_group_of(ids, i) != g) continue;   // (uniform over the grid's row)
    acc = FrAcc(reduce_to<32>(add(acc, mul(fr_load<85>(rows + (size_t)i * row_cs + (size_t)j * 8),
                                           fr_load<85>(weights + (size_t)i * 8)))));
  }
  fr_store(canonical(mul(acc, fe_const<FrP, 16>(FrP::R2))), out + (size_t)g * out_cs + (size_t)j * 8);
}

// one lane per row and point: the constants of section 22 and the scan's multipliers, as k_kzg_set_consts leaves them,
// without the table of divided differences
__global__ void __launch_bounds__(64) k_kzg_eval_set_consts(const u32* __restrict__ points, long long np,
                                                            KzgRow* __restrict__ rows, KzgSetPows* __restrict__ pows) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= np) return;
  kzg_row_consts(ElemTraits<Fe<FrP, 17>>::from_wire(points + g * 8), rows + g, pows + g);
}
// one lane per row and point: p(z) = (the value of tile 0) + z^KZG_TILE (the tail above it), as k_kzg_set_mix leaves it
__global__ void __launch_bounds__(256) k_kzg_eval_set_values(const u32* __restrict__ agg, const u32* __restrict__ tails, int nt,
                                                             long long np, const KzgRow* __restrict__ rows,
                                                             u32* __restrict__ values) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= np) return;
  const size_t at = (size_t)g * nt;
  kzg_row_value(agg + at * 8, tails + at * 8, rows[g], values + (size_t)g * 8);
}

// ---- host side ----
struct KzgEvalSetLayout {
  u32 *pts, *agg, *tails;
  KzgRow* rows;
  KzgSetPows* pows;
  int nt;
  size_t bytes;
};
static KzgEvalSetLayout kzg_eval_set_layout(int npolys, int len, int t, void* wsp) {
  KzgEvalSetLayout L;
  Bump b(wsp, ~(size_t)0);
  const size_t np = (size_t)npolys * t;
  L.nt = (len + KZG_TILE - 1) / KZG_TILE;
  L.pts = b.take<u32>(np * 8);
  L.rows = b.take<KzgRow>(np);
  L.pows = b.take<KzgSetPows>(np);
  L.agg = b.take<u32>(np * L.nt * 8);
  L.tails = b.take<u32>(np * L.nt * 8);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static bool kzg_eval_set_shape_ok(int npolys, int len, int t) {
  return kzg_shape_ok(npolys, len) && t >= 1 && t <= KZG_SET_T && (long long)npolys * t <= KZG_MAX_ELEMS;
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

int ozk_fr_rows_combine_groups_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const void* d_weights,
                                   const int32_t* group_of_row_host, int32_t groups, void* d_out, int64_t out_stride,
                                   void* stream) {
  hip_clear_stale();
  if (k < 1 || k > KZG_MULTI_ROWS || len < 1 || (long long)k * len > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad shape: %d rows of %d elements (1 <= k <= %d, 1 <= len, k len <= 2^28)", k, len,
                KZG_MULTI_ROWS);
  if (groups < 1 || groups > KZG_MULTI_GROUPS || (long long)groups * len > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad shape: %d groups (1 <= groups <= %d, groups len <= 2^28)", groups, KZG_MULTI_GROUPS);
  if (row_stride < len || out_stride < len)
    return fail(OZK_E_INVALID, "bad strides: row_stride %lld, out_stride %lld (both >= len), len %d", (long long)row_stride,
                (long long)out_stride, len);
  if (int rc = fr_check_pointers(d_rows, d_weights, group_of_row_host, d_out)) return rc;
  if (int rc = fr_check_aligned16(d_rows, d_weights, d_out)) return rc;
  if (kzg_overlap(d_rows, kzg_span(k, len, row_stride), d_out, kzg_span(groups, len, out_stride)))
    return fail(OZK_E_INVALID, "d_out overlaps d_rows");
  KzgGroupIds ids;
  memset(ids.w, 0, sizeof(ids.w));
  for (int i = 0; i < k; i++) {
    const int32_t g = group_of_row_host[i];
    if (g < 0 || g >= groups) return fail(OZK_E_INVALID, "row %d is of group %d: there are %d groups", i, g, groups);
    ids.w[i >> 2] |= (u32)g << (8 * (i & 3));
  }
  hipLaunchKernelGGL(k_fr_rows_combine_groups, dim3((len + 255) / 256, groups), dim3(256), 0, (hipStream_t)stream,
                     (const u32*)d_rows, k, len, (size_t)row_stride * 8, (const u32*)d_weights, ids, (u32*)d_out,
                     (size_t)out_stride * 8);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_fr_poly_eval_set_workspace_bytes(int32_t npolys, int32_t len, int32_t t) {
  if (!kzg_eval_set_shape_ok(npolys, len, t)) return 0;
  return kzg_eval_set_layout(npolys, len, t, nullptr).bytes;
}

int ozk_fr_poly_eval_set_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, int32_t t,
                             const uint8_t* points_host, void* d_values, void* d_workspace, size_t workspace_bytes,
                             void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(npolys, len))
    return fail(OZK_E_INVALID, "bad shape: %d polynomials of %d coefficients (1 <= both, product <= 2^28)", npolys, len);
  if (t < 1 || t > KZG_SET_T || (long long)npolys * t > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad set: %d points a row (1 <= t <= %d, npolys t <= 2^28)", t, KZG_SET_T);
  if (poly_stride != 0 && poly_stride < len)
    return fail(OZK_E_INVALID, "bad stride: poly_stride %lld (0 or >= len), len %d", (long long)poly_stride, len);
  if (int rc = fr_check_pointers(d_coeffs, points_host, d_values, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_coeffs, d_values)) return rc;
  if (kzg_overlap(d_coeffs, kzg_span(npolys, len, poly_stride), d_values, (size_t)npolys * t * 32))
    return fail(OZK_E_INVALID, "d_values overlaps d_coeffs");
  const KzgEvalSetLayout L = kzg_eval_set_layout(npolys, len, t, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long long np = (long long)npolys * t;
  kzg_set_upload(points_host, (size_t)np, L.pts, st);
  hipLaunchKernelGGL(k_kzg_eval_set_consts, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, st, (const u32*)L.pts, np, L.rows,
                     L.pows);
  hipLaunchKernelGGL(k_kzg_set_tiles, dim3((unsigned)((long long)npolys * L.nt)), dim3(KZG_WG), 0, st, (const u32*)d_coeffs,
                     (size_t)poly_stride * 8, len, L.nt, t, (const KzgRow*)L.rows, (const KzgSetPows*)L.pows, L.agg);
  hipLaunchKernelGGL(k_kzg_open_carries, dim3((unsigned)np), dim3(KZG_WG), 0, st, (const u32*)L.agg, L.nt,
                     (const KzgRow*)L.rows, L.tails);
  hipLaunchKernelGGL(k_kzg_eval_set_values, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, (const u32*)L.agg,
                     (const u32*)L.tails, L.nt, np, (const KzgRow*)L.rows, (u32*)d_values);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
