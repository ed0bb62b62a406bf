// Sums of products of points and scalars, one sum per lane (points_mac.cuh): the prepared form of the
// points once per key, then per call one recoding kernel and the multiply-accumulate kernel.
#include "ozk_common.h"
#include "curve.cuh"
#include "points_mac.cuh"

using namespace ozk;

static bool mac_shape_ok(int terms, int n) { return terms >= 1 && terms <= MAC_MAX_TERMS && n >= 1 && n <= (1 << 24); }
static int mac_check_shape(int terms, int n, int type) {
  if (type != OZK_G1) return fail(OZK_E_INVALID, "points mac: G1 only (type %d)", type);
  if (!mac_shape_ok(terms, n))
    return fail(OZK_E_INVALID, "points mac: terms = %d, n = %d out of range [1, %d] x [1, 2^24]", terms, n, MAC_MAX_TERMS);
  return OZK_OK;
}

extern "C" {

size_t ozk_points_mac_prepared_bytes(int32_t terms, int32_t n, int32_t type) {
  if (type != OZK_G1 || !mac_shape_ok(terms, n)) return 0;
  return (size_t)terms * n * MAC_ELEMS * 32;
}

size_t ozk_points_mac_workspace_bytes(int32_t terms, int32_t n, int32_t type) {
  if (type != OZK_G1 || !mac_shape_ok(terms, n)) return 0;
  return (size_t)terms * n * MAC_SCHED_WORDS * 4;
}

int ozk_points_mac_prepare_dev(const void* d_in, int32_t terms, int32_t n, int32_t type, void* d_prepared,
                               size_t prepared_bytes, void* stream) {
  hip_clear_stale();
  if (int rc = mac_check_shape(terms, n, type)) return rc;
  if (!d_in || !d_prepared) return fail(OZK_E_INVALID, "null pointer argument");
  if (misaligned(d_in) || misaligned(d_prepared)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  if (prepared_bytes < ozk_points_mac_prepared_bytes(terms, n, type))
    return fail(OZK_E_INVALID, "points mac: prepared buffer of %zu bytes, %zu needed", prepared_bytes,
                ozk_points_mac_prepared_bytes(terms, n, type));
  const size_t total = (size_t)terms * n;
  const dim3 grid((unsigned)((total + MAC_LANES - 1) / MAC_LANES)), block(MAC_LANES);
  hipLaunchKernelGGL(k_points_mac_prepare, grid, block, 0, (hipStream_t)stream, (const u32*)d_in, (int)terms, (int)n,
                     MacTable{(u32*)d_prepared, (size_t)n});
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_points_mac_dev(const void* d_prepared, const void* d_scalars, int32_t terms, int32_t n, int32_t type,
                       void* d_out, int32_t* d_codes, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (int rc = mac_check_shape(terms, n, type)) return rc;
  if (!d_prepared || !d_scalars || !d_out || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  if (misaligned(d_prepared) || misaligned(d_scalars) || misaligned(d_out) || misaligned(d_codes) ||
      misaligned(d_workspace))
    return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  if (workspace_bytes < ozk_points_mac_workspace_bytes(terms, n, type))
    return fail(OZK_E_INVALID, "points mac: workspace of %zu bytes, %zu needed", workspace_bytes,
                ozk_points_mac_workspace_bytes(terms, n, type));
  const MacSched sched{(u32*)d_workspace, (size_t)n, (int)terms};
  const size_t total = (size_t)terms * n;
  const dim3 block(MAC_LANES);
  hipLaunchKernelGGL(k_points_mac_recode, dim3((unsigned)((total + MUL_LANES - 1) / MUL_LANES)), dim3(MUL_LANES), 0,
                     (hipStream_t)stream, (const u32*)d_scalars, (int)n, sched);
  OZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_points_mac, dim3((unsigned)((n + MAC_LANES - 1) / MAC_LANES)), block, 0, (hipStream_t)stream,
                     MacTable{(u32*)d_prepared, (size_t)n}, sched, (int)n, (u32*)d_out, d_codes);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
