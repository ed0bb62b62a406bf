// n points times one scalar on the device (points_scale.cuh): the scalar is checked and recoded on
// the host, the digit schedule rides in the kernel arguments, and one launch does the rest.
#include "ozk_common.h"
#include "curve.cuh"
#include "points_scale.cuh"

using namespace ozk;

namespace {
constexpr int SCALE_MAX_N = 1 << 24;
}  // namespace

extern "C" {

int ozk_points_scale_dev(const void* d_in, int32_t n, int32_t type, const uint8_t* k_host32, void* d_out,
                         void* stream) {
  hip_clear_stale();
  if (!d_in || !d_out || !k_host32 || n <= 0 || n > SCALE_MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (misaligned(d_in) || misaligned(d_out)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  u32 k[8];
  for (int i = 0; i < 8; i++)
    k[i] = (u32)k_host32[4 * i] | (u32)k_host32[4 * i + 1] << 8 | (u32)k_host32[4 * i + 2] << 16 |
           (u32)k_host32[4 * i + 3] << 24;
  if (!scale_scalar_ok(k)) return fail(OZK_E_INVALID, "the scalar is not below r");
  ScaleSchedule s;
  scale_recode(k, type == OZK_G1, s);
  const dim3 grid((n + 63) / 64), block(64);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_points_scale<decltype(t)::TYPE>, grid, block, 0, (hipStream_t)stream, (const u32*)d_in, (int)n,
                       s, (u32*)d_out);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

}  // extern "C"
