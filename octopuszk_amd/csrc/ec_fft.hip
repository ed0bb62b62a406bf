// Entry points of the point kernels of ec_fft.cuh: the transform over curve points, the sparse matrix
// times a vector of points, and the pointwise sum.  Arguments are checked on the host; nothing is enqueued for a bad one.
#include "ozk_common.h"
#include "curve.cuh"
#include "ec_fft.cuh"

using namespace ozk;

namespace {
constexpr int ECFFT_MAX_LOGN = 22;
constexpr int EC_MAX_N = 1 << 24;
using Fr32 = Fe<FrParams, 32>;

size_t pad256(size_t v) { return (v + 255) & ~(size_t)255; }
int log2_exact(int n) {
  if (n <= 0 || (n & (n - 1))) return -1;
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}
void load_le(const uint8_t* b, u32 (&w)[8]) {
  for (int i = 0; i < 8; i++)
    w[i] = (u32)b[4 * i] | (u32)b[4 * i + 1] << 8 | (u32)b[4 * i + 2] << 16 | (u32)b[4 * i + 3] << 24;
}
bool is_one(const Fr32& a) {
  u32 o[8];
  from_mont(a, o);
  u32 d = o[0] ^ 1u;
  for (int i = 1; i < 8; i++) d |= o[i];
  return d == 0;
}
size_t point_bytes(int type) { return type == OZK_G1 ? 96 : 192; }

template <int TYPE>
void ec_fft_run(const u32* in, int logn, const EcFftTwiddle& last, const EcFftTwiddle& inner, bool inverse, u32* out,
               uint8_t* ws, hipStream_t st) {
  const int n = 1 << logn;
  hipLaunchKernelGGL(k_ecfft_permute<TYPE>, dim3((n + 63) / 64), dim3(64), 0, st, in, n, logn, out);
  if (logn == 0) return;
  const int n_last = n / 2, n_inner = n / 4;
  ScaleSchedule* t_last = (ScaleSchedule*)ws;
  ScaleSchedule* t_inner = (ScaleSchedule*)(ws + pad256((size_t)n_last * sizeof(ScaleSchedule)));
  hipLaunchKernelGGL(k_ecfft_recode<TYPE>, dim3((n_last + 63) / 64), dim3(64), 0, st, last, n_last, t_last);
  if (n_inner)
    hipLaunchKernelGGL(k_ecfft_recode<TYPE>, dim3((n_inner + 63) / 64), dim3(64), 0, st, inner, n_inner, t_inner);
  const dim3 grid((n / 2 + 63) / 64), block(64);
  for (int logh = 0; logh < logn; logh++) {
    const bool is_last = logh == logn - 1;
    // blocks B = n / 2h; an inner pass reads omega^(j B) = (omega^2)^(j B / 2)
    const int stride = is_last ? 1 : 1 << (logn - 2 - logh);
    hipLaunchKernelGGL(k_ecfft_pass<TYPE>, grid, block, 0, st, out, logn, logh,
                       (const ScaleSchedule*)(is_last ? t_last : t_inner), stride, (int)!(is_last && inverse),
                       (const ScaleSchedule*)(is_last && inverse ? t_last : nullptr));
  }
}
}  // namespace

extern "C" {

size_t ozk_ec_fft_workspace_bytes(int32_t n, int32_t type) {
  const int logn = log2_exact(n);
  if (logn < 0 || logn > ECFFT_MAX_LOGN || check_point_type(type)) return 0;
  return pad256((size_t)(n / 2) * sizeof(ScaleSchedule)) + pad256((size_t)(n / 4) * sizeof(ScaleSchedule)) + 256;
}

int ozk_ec_fft_dev(const void* d_in, int32_t n, int32_t type, const uint8_t* omega_host32, int32_t inverse,
                   void* d_out, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_in || !d_out || !omega_host32 || !d_workspace) return fail(OZK_E_INVALID, "null pointer argument");
  if (int rc = check_point_type(type)) return rc;
  const int logn = log2_exact(n);
  if (logn < 0 || logn > ECFFT_MAX_LOGN) return fail(OZK_E_INVALID, "size %d is not a power of two in [1, 2^22]", (int)n);
  if (misaligned(d_in) || misaligned(d_out) || misaligned(d_workspace))
    return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
  const size_t bytes = (size_t)n * point_bytes(type);
  if (a < b + bytes && b < a + bytes) return fail(OZK_E_INVALID, "d_out overlaps d_in: the transform is out of place");
  if (workspace_bytes < ozk_ec_fft_workspace_bytes(n, type))
    return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", ozk_ec_fft_workspace_bytes(n, type),
                workspace_bytes);
  u32 w[8];
  load_le(omega_host32, w);
  if (!scale_scalar_ok(w)) return fail(OZK_E_INVALID, "omega is not below r");
  // omega must have order exactly n: omega^(n/2) != 1 and its square is 1
  const Fr32 om = Fr32(to_mont<FrParams>(w));
  Fr32 half = om;
  for (int i = 0; i + 1 < logn; i++) half = Fr32(sqr(half));
  const Fr32 full = logn ? Fr32(sqr(half)) : om;
  if (!is_one(full) || (logn && is_one(half))) return fail(OZK_E_INVALID, "omega is not a primitive root of unity of order %d", (int)n);
  EcFftTwiddle last, inner;
  Fr32 base = om, k = Fr32(fe_one<FrParams>());
  if (inverse) {
    base = Fr32(inv(om));
    const u32 nw[8] = {(u32)n, 0, 0, 0, 0, 0, 0, 0};
    k = Fr32(inv(Fr32(to_mont<FrParams>(nw))));
  }
  from_mont(base, last.base);
  from_mont(k, last.k);
  from_mont(Fr32(sqr(base)), inner.base);
  from_mont(Fr32(fe_one<FrParams>()), inner.k);
  return by_point_type(type, [&](auto t) {
    ec_fft_run<decltype(t)::TYPE>((const u32*)d_in, logn, last, inner, inverse != 0, (u32*)d_out, (uint8_t*)d_workspace,
                                  (hipStream_t)stream);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

size_t ozk_sparse_mat_points_workspace_bytes(int32_t n_long, int32_t type) {
  if (n_long <= 0 || check_point_type(type)) return 0;
  return (size_t)n_long * (EC_LONG_LANES + 64) * point_bytes(type) + 256;
}

int ozk_sparse_mat_points_dev(const void* d_row_ptr, const void* d_index, const void* d_coeff, const void* d_points,
                              int32_t rows, int32_t type, const void* d_long_rows, int32_t n_long, void* d_out,
                              void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!d_row_ptr || !d_index || !d_points || !d_out || (n_long > 0 && (!d_long_rows || !d_workspace)))
    return fail(OZK_E_INVALID, "null pointer argument");
  if (int rc = check_point_type(type)) return rc;
  if (rows <= 0 || rows > EC_MAX_N || n_long < 0 || n_long > rows || n_long > (1 << 16))
    return fail(OZK_E_INVALID, "row counts out of range");
  if (misaligned(d_row_ptr) || misaligned(d_index) || misaligned(d_coeff) || misaligned(d_points) || misaligned(d_out) ||
      misaligned(d_long_rows) || misaligned(d_workspace))
    return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  if (n_long > 0 && workspace_bytes < ozk_sparse_mat_points_workspace_bytes(n_long, type))
    return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu",
                ozk_sparse_mat_points_workspace_bytes(n_long, type), workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const u32 *ptr = (const u32*)d_row_ptr, *idx = (const u32*)d_index, *co = (const u32*)d_coeff, *pts = (const u32*)d_points;
  const u32* lr = (const u32*)d_long_rows;
  u32* part1 = (u32*)d_workspace;
  u32* part2 = n_long > 0 ? (u32*)((uint8_t*)d_workspace + (size_t)n_long * EC_LONG_LANES * point_bytes(type)) : nullptr;
  const dim3 block(64), grid((rows + 63) / 64);
  return by_point_type(type, [&](auto t) {
    constexpr int T = decltype(t)::TYPE;
    hipLaunchKernelGGL(k_sparse_points<T>, grid, block, 0, st, ptr, idx, co, pts, (int)rows, (u32*)d_out);
    if (n_long > 0) {
      hipLaunchKernelGGL(k_sparse_points_long<T>, dim3(n_long * (EC_LONG_LANES / 64)), block, 0, st, ptr, idx, co, pts, lr, part1);
      hipLaunchKernelGGL(k_points_sum64<T>, dim3(n_long), block, 0, st, (const u32*)part1, n_long * 64, (const u32*)nullptr, part2);
      hipLaunchKernelGGL(k_points_sum64<T>, dim3((n_long + 63) / 64), block, 0, st, (const u32*)part2, (int)n_long, lr, (u32*)d_out);
    }
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

int ozk_points_add_dev(const void* d_a, const void* d_b, int32_t n, int32_t type, int32_t negate_b, void* d_out,
                       void* stream) {
  hip_clear_stale();
  if (!d_a || !d_b || !d_out || n <= 0 || n > EC_MAX_N) return fail(OZK_E_INVALID, "bad argument");
  if (int rc = check_point_type(type)) return rc;
  if (misaligned(d_a) || misaligned(d_b) || misaligned(d_out)) return fail(OZK_E_INVALID, "buffers must be 4-byte aligned");
  const dim3 grid((n + 63) / 64), block(64);
  return by_point_type(type, [&](auto t) {
    hipLaunchKernelGGL(k_points_add<decltype(t)::TYPE>, grid, block, 0, (hipStream_t)stream, (const u32*)d_a,
                       (const u32*)d_b, (int)n, (int)negate_b, (u32*)d_out);
    OZK_HIP(hipGetLastError());
    return OZK_OK;
  });
}

}  // extern "C"
