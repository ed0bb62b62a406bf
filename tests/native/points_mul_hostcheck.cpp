// Host build of the per-point function of the points-times-scalars kernel (octopuszk_amd/csrc/points_mul.cuh,
// DESIGN.md §21): the check of the scalar, its recoding into the lane's own schedule words and the ladder, for
// tests/test_srs_phase1_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _points_mul_hostcheck.so points_mul_hostcheck.cpp
#include "../../octopuszk_amd/csrc/points_mul.cuh"
using namespace ozk;

// in: one wire-in point (24 / 48 words), k: 8 words -> out: [k] of it, wire-in; returns the code the kernel writes
// (0, or 1 with out = O for k >= r).  The schedule words sit at the kernel's own stride inside a block poisoned
// before the call, and the words of the two neighbouring lanes must come back untouched: -2 if not.
extern "C" int pmhc_mul(const u32* in, int type, const u32* k, u32* out) {
  u32 block[3 * MUL_STRIDE];
  for (int i = 0; i < 3 * MUL_STRIDE; i++) block[i] = 0xdeadbeefu;
  u32* mine = block + MUL_STRIDE;
  const int code = type == 1 ? mul_point<G1Cfg, true>(in, k, mine, out) : mul_point<G2Cfg, false>(in, k, mine, out);
  for (int i = 0; i < 3 * MUL_STRIDE; i++)
    if ((i < MUL_STRIDE || i >= 2 * MUL_STRIDE - 1) && block[i] != 0xdeadbeefu) return -2;
  return code;
}
// the same with out == in
extern "C" int pmhc_mul_in_place(u32* point, int type, const u32* k) { return pmhc_mul(point, type, k, point); }
