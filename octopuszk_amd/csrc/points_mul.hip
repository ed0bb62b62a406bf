// n points times n scalars on the device (points_mul.cuh): the scalars stay in device memory, every
// lane checks and recodes its own inside the one kernel this launches.
#include "ozk_common.h"
#include "curve.cuh"
#include "points_mul.cuh"

using namespace ozk;

extern "C" {

int ozk_points_mul_dev(const void* d_in, const void* d_scalars, int32_t n, int32_t type, void* d_out,
                       int32_t* d_codes, void* stream) {
  hip_clear_stale();
  if (!d_in || !d_scalars || !d_out || n <= 0 || n > (1 << 24)) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (misaligned(d_in) || misaligned(d_scalars) || misaligned(d_out) || misaligned(d_codes))
    return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  const dim3 grid((n + MUL_LANES - 1) / MUL_LANES), block(MUL_LANES);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_points_mul<decltype(t)::TYPE>, grid, block, 0, (hipStream_t)stream, (const u32*)d_in,
                       (const u32*)d_scalars, (int)n, (u32*)d_out, d_codes);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

}  // extern "C"
