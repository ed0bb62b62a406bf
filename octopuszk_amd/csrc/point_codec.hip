// Point compression and decompression on the device (point_codec.cuh): typed batches of G1 or G2
// points, and K compressed Groth16 proofs (128 bytes each) straight into the 768-byte records that
// ozk_groth16_verify_dev and ozk_groth16_verify_rlc_dev take.
#include "ozk_common.h"
#include "curve.cuh"
#include "point_codec.cuh"

using namespace ozk;

namespace {

constexpr int CODEC_MAX_N = 1 << 24;
constexpr int CODEC_PREPARED_MAX_N = 1 << 23;   // the GLV plan of the variable-base MSM (msm_var_driver.cuh GLV_MAX_N)

// words per coordinate of a wire format: 0 wire-in (32-byte coordinates), 1 wire-out (64-byte)
int coord_words(int32_t format) { return format == 0 ? 8 : format == 1 ? 16 : 0; }

}  // namespace

extern "C" {

int ozk_points_decompress_dev(const void* d_in, int32_t n, int32_t type, int32_t out_format, void* d_out,
                              int32_t* d_codes, void* stream) {
  hip_clear_stale();
  const int S = coord_words(out_format);
  if (!d_in || !d_out || !d_codes || n <= 0 || n > CODEC_MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (!S) return fail(OZK_E_INVALID, "unknown point format %d", (int)out_format);
  if (misaligned(d_in) || misaligned(d_out)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  const dim3 grid((n + 63) / 64), block(64);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_codec_decompress<decltype(t)::TYPE>, grid, block, 0, (hipStream_t)stream, (const u32*)d_in,
                       (int)n, S, (u32*)d_out, d_codes);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

int ozk_points_decompress_prepared_dev(const void* d_in, int32_t n, int32_t type, void* d_prepared,
                                       size_t prepared_bytes, int32_t* d_codes, int32_t check_subgroup, void* stream) {
  hip_clear_stale();
  if (!d_in || !d_prepared || !d_codes || n <= 0) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (n > CODEC_PREPARED_MAX_N || !ozk_var_msm_glv(n))
    return fail(OZK_E_INVALID, "%d points: only the two-record GLV form of the prepared bases is written (n <= 2^23)", (int)n);
  if (prepared_bytes < ozk_var_msm_prepared_bytes(n, type))
    return fail(OZK_E_INVALID, "prepared buffer too small: %zu < %zu", prepared_bytes, ozk_var_msm_prepared_bytes(n, type));
  if (misaligned(d_in) || misaligned(d_prepared)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((n + 63) / 64), block(64);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_codec_decompress_prepared<decltype(t)::TYPE>, grid, block, 0, s, (const u32*)d_in, (int)n,
                       (u32*)d_prepared, d_codes);
    if (check_subgroup && decltype(t)::TYPE == OZK_G2)   // G1 has cofactor 1: nothing to check there
      hipLaunchKernelGGL(k_codec_subgroup_g2, grid, block, 0, s, (u32*)d_prepared, (int)n, d_codes);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

int ozk_points_compress_dev(const void* d_in, int32_t n, int32_t type, int32_t in_format, void* d_out,
                            void* stream) {
  hip_clear_stale();
  const int S = coord_words(in_format);
  if (!d_in || !d_out || n <= 0 || n > CODEC_MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (!S) return fail(OZK_E_INVALID, "unknown point format %d", (int)in_format);
  if (misaligned(d_in) || misaligned(d_out)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  const dim3 grid((n + 63) / 64), block(64);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_codec_compress<decltype(t)::TYPE>, grid, block, 0, (hipStream_t)stream, (const u32*)d_in, (int)n,
                       S, (u32*)d_out);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

int ozk_groth16_proofs_decompress_dev(const void* d_in128, int32_t k, void* d_records768, int32_t* d_codes,
                                      void* stream) {
  hip_clear_stale();
  if (!d_in128 || !d_records768 || !d_codes || k <= 0 || k > CODEC_MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (misaligned(d_in128) || misaligned(d_records768)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int32_t* d_codes3 = nullptr;
  OZK_HIP(hipMallocAsync((void**)&d_codes3, (size_t)3 * k * sizeof(int32_t), s));
  const int g1_blocks = (int)((2L * k + 63) / 64), g2_blocks = (k + 63) / 64;
  hipLaunchKernelGGL(k_codec_proofs, dim3(g1_blocks + g2_blocks), dim3(64), 0, s, (const u32*)d_in128, (int)k,
                     g1_blocks, (u32*)d_records768, d_codes3);
  hipLaunchKernelGGL(k_codec_proof_codes, dim3((k + 255) / 256), dim3(256), 0, s, (const int32_t*)d_codes3, (int)k,
                     d_codes);
  const hipError_t e = hipGetLastError();
  OZK_HIP(hipFreeAsync(d_codes3, s));
  OZK_HIP(e);
  return OZK_OK;
}

}  // extern "C"
