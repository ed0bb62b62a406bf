// n points, each multiplied by ITS OWN scalar: out_i = [k_i] P_i.  What a phase-1 contribution does
// to a powers-of-tau string: tau_g1[i] times s^i, alpha_tau_g1[i] times a s^i, and so on.
//
// One point per lane.  The lane checks k_i < r, recodes it with scale_recode (points_scale.cuh: G1 the GLV halves in
// joint sparse form, G2 the non-adjacent form of k without the endomorphism, exact on the whole twist) and runs
// scale_ladder over its own schedule.  A wave then doubles at every step and adds whenever ANY lane's column is
// non-zero, which is almost always; the lanes whose column is zero idle through that addition.
//
// The schedule is 32 words read at an index that depends on the loop counter, so in registers it would be scratch
// (what k_ecfft_recode pays), and through HBM it would be 132 bytes per point.  It lives in LDS instead: a lane owns
// words [MUL_STRIDE * lane, +32) of its workgroup's block.  MUL_STRIDE = 33 is odd, so the 64 lanes of a wave that
// read the same word index of their schedules hit different banks (distinct modulo 64, and modulo 32 within either
// half of the wave).  No lane reads another's words: no barrier.
// The length stays in a register.
// The header compiles for the host too (tests/native/points_mul_hostcheck.cpp), the kernel only in points_mul.hip.
#pragma once
#include "points_scale.cuh"

namespace ozk {

constexpr int MUL_LANES = 64;                        // one wave per workgroup, as k_points_scale
constexpr int MUL_STRIDE = SCALE_MAX_STEPS / 8 + 1;  // words between two lanes' schedules
constexpr int MUL_LDS_WORDS = MUL_LANES * MUL_STRIDE;

// a schedule whose words lie where the caller says (LDS on the device, an array on the host)
struct LaneSchedule {
  u32* w;
  int32_t len;
};

// in: one wire-in point, k: 8 words little-endian, sched: SCALE_MAX_STEPS / 8 words of the lane's own ->
// out: [k] of the point as wire-in with Z = 1 and 0, or O and 1 for k >= r.  in and k are read whole before out is
// written, so out may be in.
template <class CV, bool GLV>
OZK_HD int mul_point(const u32* in, const u32* k_in, u32* sched, u32* out) {
  u32 k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_in[i];
  if (!scale_scalar_ok(k)) {
    CurveIO<CV>::template write_inf<WireIn>(out);
    return 1;
  }
  LaneSchedule s{sched, 0};
  scale_recode(k, GLV, s);
  scale_point<CV, GLV>(in, s, out);
  return 0;
}

#if defined(__HIPCC__)
// in and out may be the same buffer: no __restrict__, and a lane touches its own record only.
template <int TYPE>   // 1: G1, 2: G2
__global__ __launch_bounds__(MUL_LANES) void k_points_mul(const u32* in, const u32* scalars, int n, u32* out,
                                                          int32_t* codes) {
  __shared__ u32 sched[MUL_LDS_WORDS];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32* mine = sched + MUL_STRIDE * threadIdx.x;
  int code;
  if constexpr (TYPE == 1)
    code = mul_point<G1Cfg, true>(in + 24L * i, scalars + 8L * i, mine, out + 24L * i);
  else
    code = mul_point<G2Cfg, false>(in + 48L * i, scalars + 8L * i, mine, out + 48L * i);
  if (codes) codes[i] = code;
}
#endif

}  // namespace ozk
