// Shared-base batched MSM (msm_multi.hip): the table plan and the scalar recoding, header-only and free of
// device intrinsics so that the host check (tests/native/multi_msm_hostcheck.cpp) compiles exactly the code
// the evaluation kernel runs.  The Python model tests/multi_msm_ref.py restates both rules.
//
// Table of one base P, window size ws, half = 2^(ws-1), oc = ceil(128 / ws) windows:
//     T[w][d - 1] = d * 2^(w*ws) * P          for w < oc, 1 <= d <= half
// as 64-byte affine Montgomery records (x | y; (0, 0) = infinity).  A scalar s is reduced mod r and split by
// the GLV endomorphism (glv.cuh) into s = +-|k1| +- |k2| lambda with |k1|, |k2| < 2^127; each half is recoded
// into oc signed digits d_w in [-(half - 1), half] with sum_w d_w 2^(w*ws) = |k|, and
//     s P = sum_w sgn1 * d1_w-th entry  +  phi(sum_w sgn2 * d2_w-th entry),     phi(x, y) = (beta x, y).
// The recoding carries upwards: raw_w = bits [w*ws, w*ws + ws) of |k| + carry; raw_w > half gives
// d_w = raw_w - 2^ws and a carry of 1.  The top window takes no carry OUT: for oc*ws > 128 its raw value is
// a few bits wide, and for oc*ws == 128 (ws = 8, 4) it is at most 127 + 1 = half because |k| < 2^127
// (tests/test_glv.py proves the bound 2^126.97).
#pragma once
#include <stddef.h>

#include "glv.cuh"

namespace ozk {

constexpr int MM_MAX_N = 4096;
constexpr long long MM_MAX_KN = 1ll << 28;
constexpr int MM_WS_MIN = 4, MM_WS_MAX = 8;
constexpr size_t MM_TABLE_BUDGET = (size_t)160 << 20;   // bytes: the table should stay inside the 256 MiB Infinity Cache

OZK_HD int mm_windows(int ws) { return (128 + ws - 1) / ws; }
OZK_HD size_t mm_records_per_base(int ws) { return (size_t)mm_windows(ws) << (ws - 1); }
// widest window whose table of n bases fits the budget: 8 up to n = 1280, 7 up to 2155, 6 up to 3723, 5 above
OZK_HD int mm_window_bits(int n) {
  for (int ws = MM_WS_MAX; ws > MM_WS_MIN; ws--)
    if ((size_t)n * mm_records_per_base(ws) * 64 <= MM_TABLE_BUDGET) return ws;
  return MM_WS_MIN;
}

// digit w of the recoding of the 128-bit magnitude k (4 words), given the carry into the window; updates carry
OZK_HD int mm_signed_digit(u32 k0, u32 k1, u32 k2, u32 k3, int w, int ws, u32& carry) {
  const int bit = w * ws;
  u32 raw = carry;
  if (bit < 128) {
    const int wi = bit >> 5, sh = bit & 31;
    const u32 lo = wi == 0 ? k0 : wi == 1 ? k1 : wi == 2 ? k2 : k3;
    const u32 hi = wi == 0 ? k1 : wi == 1 ? k2 : wi == 2 ? k3 : 0u;
    const u64 v = (u64)lo | ((u64)hi << 32);
    raw += (u32)(v >> sh) & ((1u << ws) - 1u);
  }
  const u32 half = 1u << (ws - 1);
  carry = raw > half ? 1u : 0u;
  return (int)raw - (int)(carry << ws);
}

}  // namespace ozk
