// The Fr side of the KZG layer on gfx950 as one unit: the kernels, workspace layouts and C ABI (include/ozk.h) of
//   kzg.cuh        openings at one point,
//   kzg_set.cuh    openings at a set of points (section 23),
//   kzg_multi.cuh  grouped row sums and values at a set (section 28),
// each a section of this unit, and the evaluation of polynomials at a point, whose kernels (fr_tables.cuh) BACE
// launches too.  What the sections share is fr_rows.cuh's.
#include "host_ctx.h"   // pad256
#include "kzg.cuh"
#include "kzg_set.cuh"
#include "kzg_multi.cuh"

using namespace ozk;

extern "C" {

size_t ozk_fr_poly_eval_workspace_bytes(int32_t npolys) { return npolys > 0 ? pad256((size_t)npolys * 256 * 32) + 512 : 0; }

int ozk_fr_poly_eval_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, const uint8_t* r_host32,
                         void* d_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_coeffs || !r_host32 || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  if (npolys <= 0 || npolys > FR_POLY_EVAL_MAX || len <= 0 || poly_stride < 0 || (npolys > 1 && poly_stride < len))
    return fail(OZK_E_INVALID, "bad shape: %d polynomials of %d coefficients, stride %lld", npolys, len, (long long)poly_stride);
  if (workspace_bytes < ozk_fr_poly_eval_workspace_bytes(npolys)) return fail(OZK_E_INVALID, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  u32* partial = (u32*)d_workspace;
  u32* r = (u32*)((uint8_t*)d_workspace + pad256((size_t)npolys * 256 * 32));
  fr_put_element(r_host32, r, st);
  hipLaunchKernelGGL(k_to_mont_inplace, dim3(1), dim3(64), 0, st, r, 1);
  fr_poly_eval((const u32*)d_coeffs, (size_t)poly_stride * 8, len, npolys, r, partial, (u32*)d_out, st);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
