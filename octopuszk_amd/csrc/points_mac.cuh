// n sums of `terms` products: out_i = sum_v [k_v[i]] P_v[i], G1.  The middle step of the FK20
// construction for KZG openings at every coset: the P_v are fixed per key, the k_v change with every polynomial.
//
// Done with the entry points there were, a sum is `terms` ladders of points_mul.cuh and `terms - 1` additions: the
// 128-step doubling chain and the final inversion `terms` times over, and one inversion more per ladder for the GLV
// difference point.  Here a lane keeps ONE Jacobian accumulator for its output (Straus): per ladder step one jac_dbl,
// then for every term whose column is non-zero one complete jac_madd, and one normalisation at the end.
//
// Three kernels:
//   prepare   once per set of points: a wire-in point becomes the six field elements a ladder step can ask for,
//             x, beta x, beta^2 x, y, T.x, T.y with T = P - phi(P), canonical Montgomery words.  scale_ladder
//             recomputes the last two with an inversion per call; here the hot kernel runs no inversion per term.
//             O is six zero elements: whatever a step selects is then (0, 0), which jac_madd takes as O.
//             Layout: element e of term v of lane i at words [((6 v + e) n + i) 8, +8): the lanes of a wave read
//             consecutive 32-byte elements whichever element each of them selects.
//   recode    one (lane, term) per thread: the check k < r and scale_recode (the GLV halves in joint sparse form)
//             into LDS at the stride of points_mul.cuh, then out to the workspace.  |k1|, |k2| < 2^127
//             (tests/test_glv.py), so a schedule has at most MAC_STEPS = 128 columns: MAC_WORDS = 16 words and the
//             length as a 17th, word j of term v of lane i at word (j terms + v) n + i: again consecutive lanes,
//             consecutive words.  A scalar >= r writes the length -1.
//   mac       one output per lane.  The schedules are STREAMED from the workspace, one word per term per step (8 steps
//             share a word, which the cache serves), so the kernel holds no schedule in LDS or registers and there is
//             no term-group size: 1 to 32 terms run the same loop, the doubling chain once.  At 33 words per (lane,
//             term) 32 terms would not have fitted LDS beside a useful occupancy.  (A variant that kept the current
//             word of every term in LDS and fetched the addend of term v + 1 before adding term v, loads in flight
//             over a whole addition, measured the same 34 ms at 16 terms over 2^17 lanes: the kernel does not wait for
//             these loads, and the simpler loop stayed.)
// Every addition is jac_madd (complete: P == Q doubles, P == -Q gives O, O on either side) and jac_dbl is exact for
// every point, so equal points among the terms, P with -P, O among the terms, k = 0 and k = r - 1 are all exact.
// The per-lane functions compile for the host too (tests/native/points_mac_hostcheck.cpp), the kernels only in
// points_mac.hip.
#pragma once
#include "points_mul.cuh"

namespace ozk {

constexpr int MAC_MAX_TERMS = 32;
constexpr int MAC_LANES = 64;
constexpr int MAC_ELEMS = 6;
constexpr int MAC_X = 0, MAC_BX = 1, MAC_B2X = 2, MAC_Y = 3, MAC_TX = 4, MAC_TY = 5;
constexpr int MAC_STEPS = 128;
constexpr int MAC_WORDS = MAC_STEPS / 8;
constexpr int MAC_SCHED_WORDS = MAC_WORDS + 1;   // the columns, then the length
constexpr u32 MAC_BAD_SCALAR = 0xffffffffu;      // the length of a scalar >= r

// the prepared points of `n` lanes (device: the caller's buffer; host: an array)
struct MacTable {
  u32* p;
  size_t n;
  OZK_HD u32* at(int v, int e, size_t i) const { return p + (((size_t)v * MAC_ELEMS + e) * n + i) * 8; }
};
// the schedules of `terms` x `n` scalars
struct MacSched {
  u32* p;
  size_t n;
  int terms;
  OZK_HD u32& at(int j, int v, size_t i) const { return p[((size_t)j * terms + v) * n + i]; }
};

// in: one wire-in point (any Z, Z = 0 is O) -> its six elements at (v, i)
template <class CV>
OZK_HD void mac_prepare_point(const u32* in, const MacTable& t, int v, size_t i) {
  using EA = typename CV::EA;
  const Aff<EA> q = CurveIO<CV>::aff_from_wire(in);
  EA e[MAC_ELEMS];
#pragma unroll
  for (int k = 0; k < MAC_ELEMS; k++) e[k] = EA(el_zero(q.x));
  if (!is_inf(q)) {
    e[MAC_X] = q.x;
    e[MAC_Y] = q.y;
    e[MAC_BX] = EA(canonical(scale(q.x, glv_beta<CV>())));
    e[MAC_B2X] = EA(canonical(scale(e[MAC_BX], glv_beta<CV>())));
    // T = q + (beta x, -y): slope -2 y / (beta x - x), as scale_ladder
    const auto sl = mul(dbl(neg(q.y)), inv(sub(e[MAC_BX], q.x)));
    e[MAC_TX] = EA(canonical(sub(sqr(sl), add(q.x, e[MAC_BX]))));
    e[MAC_TY] = EA(canonical(sub(mul(sl, sub(q.x, e[MAC_TX])), q.y)));
  }
#pragma unroll
  for (int k = 0; k < MAC_ELEMS; k++) ElemTraits<EA>::store(e[k], t.at(v, k, i));
}

// k: 8 words little-endian, tmp: SCALE_MAX_STEPS / 8 words of the lane's own -> the schedule of (v, i)
OZK_HD void mac_recode_scalar(const u32* k_in, u32* tmp, const MacSched& s, int v, size_t i) {
  u32 k[8];
#pragma unroll
  for (int j = 0; j < 8; j++) k[j] = k_in[j];
  if (!scale_scalar_ok(k)) {
    s.at(MAC_WORDS, v, i) = MAC_BAD_SCALAR;
    return;
  }
  LaneSchedule ls{tmp, 0};
  scale_recode(k, true, ls);
  for (int j = 0; j < MAC_WORDS; j++) s.at(j, v, i) = tmp[j];
  // (the bound on the GLV halves rules a longer schedule out; were there one, the lane would be refused, not wrong)
  s.at(MAC_WORDS, v, i) = ls.len <= MAC_STEPS ? (u32)ls.len : MAC_BAD_SCALAR;
}

// lane i: out = sum_v [k_v] P_v as wire-in with Z = 1 and 0, or O and 1 when one of its scalars was >= r
template <class CV>
OZK_HD int mac_lane(const MacTable& t, const MacSched& s, size_t i, u32* out) {
  using EA = typename CV::EA;
  using IO = CurveIO<CV>;
  int top = 0;
  bool bad = false;
  for (int v = 0; v < s.terms; v++) {
    const int32_t len = (int32_t)s.at(MAC_WORDS, v, i);
    bad |= len < 0;
    top = len > top ? len : top;
  }
  if (bad) {
    IO::template write_inf<WireIn>(out);
    return 1;
  }
  Jac<CV> acc = jac_infinity<CV>();
#pragma unroll 1
  for (int step = top - 1; step >= 0; step--) {
    acc = jac_dbl<CV>(acc);
    const int j = step >> 3, sh = 4 * (step & 7);
#pragma unroll 1
    for (int v = 0; v < s.terms; v++) {
      const u32 c = (s.at(j, v, i) >> sh) & 15u;
      if (c == 0) continue;
      const bool d1 = (c & SCALE_D1) != 0, d2 = (c & SCALE_D2) != 0;
      const bool n1 = (c & SCALE_N1) != 0, n2 = (c & SCALE_N2) != 0;
      const bool same = d1 && d2 && n1 == n2, diff = d1 && d2 && n1 != n2;
      //   (+-1, 0) +-(x, y)      (0, +-1) +-(beta x, y)      +-(1, 1) -+(beta^2 x, y)      +-(1, -1) +-T
      const int xe = same ? MAC_B2X : (diff ? MAC_TX : (d1 ? MAC_X : MAC_BX));
      const bool negate = same ? !n1 : (d1 ? n1 : n2);
      Aff<EA> a;
      a.x = ElemTraits<EA>::load(t.at(v, xe, i));
      a.y = ElemTraits<EA>::load(t.at(v, diff ? MAC_TY : MAC_Y, i));
      if (negate) a.y = EA(canonical(neg(a.y)));
      acc = jac_madd<CV>(acc, a);
    }
  }
  IO::template write<WireIn>(acc, out);
  return 0;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(MAC_LANES) void k_points_mac_prepare(const u32* in, int terms, int n, MacTable t) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // v n + i: the input is term-major
  if (g >= (size_t)terms * n) return;
  mac_prepare_point<G1Cfg>(in + 24 * g, t, (int)(g / n), g % n);
}

__global__ __launch_bounds__(MUL_LANES) void k_points_mac_recode(const u32* scalars, int n, MacSched s) {
  __shared__ u32 tmp[MUL_LDS_WORDS];
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)s.terms * n) return;
  mac_recode_scalar(scalars + 8 * g, tmp + MUL_STRIDE * threadIdx.x, s, (int)(g / n), g % n);
}

__global__ __launch_bounds__(MAC_LANES) void k_points_mac(MacTable t, MacSched s, int n, u32* out, int32_t* codes) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  const int code = mac_lane<G1Cfg>(t, s, i, out + 24 * i);
  if (codes) codes[i] = code;
}
#endif

}  // namespace ozk
