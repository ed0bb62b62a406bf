// Host build of the shared-scalar point multiplication (octopuszk_amd/csrc/points_scale.cuh): the
// recoding the entry point runs on the host and the per-point function the kernel runs, for tests/test_ceremony_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _ceremony_hostcheck.so ceremony_hostcheck.cpp
#include "../../octopuszk_amd/csrc/points_scale.cuh"
using namespace ozk;

// k: 8 words, type 1 (G1: GLV halves jointly) or 2 (G2: k alone) -> steps[0 .. len) least significant first, 4 bits
// each in a byte; returns len, or -1 for k >= r
extern "C" int cmhc_recode(const u32* k_in, int type, uint8_t* steps) {
  u32 k[8];
  for (int i = 0; i < 8; i++) k[i] = k_in[i];
  if (!scale_scalar_ok(k)) return -1;
  ScaleSchedule s;
  scale_recode(k, type == 1, s);
  for (int i = 0; i < s.len; i++) steps[i] = (uint8_t)scale_step(s, i);
  return s.len;
}
// in: one wire-in point (24 / 48 words), k: 8 words < r -> out: [k] of it, wire-in; returns 0, or -1 for k >= r
extern "C" int cmhc_scale(const u32* in, int type, const u32* k_in, u32* out) {
  u32 k[8];
  for (int i = 0; i < 8; i++) k[i] = k_in[i];
  if (!scale_scalar_ok(k)) return -1;
  ScaleSchedule s;
  scale_recode(k, type == 1, s);
  if (type == 1)
    scale_point<G1Cfg, true>(in, s, out);
  else
    scale_point<G2Cfg, false>(in, s, out);
  return 0;
}
