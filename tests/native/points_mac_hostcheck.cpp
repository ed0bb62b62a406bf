// Host build of the per-lane functions of the multiply-accumulate kernel over points (octopuszk_amd/csrc/
// points_mac.cuh): the prepared form of a point, the recoding of a scalar into the streamed schedule
// and the lane's accumulation, for tests/test_kzg_all_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _points_mac_hostcheck.so points_mac_hostcheck.cpp
#include <vector>

#include "../../octopuszk_amd/csrc/points_mac.cuh"
using namespace ozk;

// points: terms wire-in G1 points (24 words each), scalars: terms x 8 words -> out: sum_v [k_v] P_v, wire-in; returns
// the code the kernel writes (0, or 1 with out = O when a scalar is >= r).  The lane is the middle one of three: the
// table and the schedules have the kernel's own layout for n = 3, the neighbours' words are poisoned before the call
// and must come back untouched: -2 if not.
extern "C" int pmac_run(const u32* points, const u32* scalars, int terms, u32* out) {
  const size_t n = 3, lane = 1;
  std::vector<u32> table(terms * MAC_ELEMS * n * 8, 0xdeadbeefu), sched(MAC_SCHED_WORDS * terms * n, 0xdeadbeefu);
  const MacTable t{table.data(), n};
  const MacSched s{sched.data(), n, terms};
  u32 tmp[SCALE_MAX_STEPS / 8];
  for (int v = 0; v < terms; v++) {
    mac_prepare_point<G1Cfg>(points + 24 * v, t, v, lane);
    mac_recode_scalar(scalars + 8 * v, tmp, s, v, lane);
  }
  const int code = mac_lane<G1Cfg>(t, s, lane, out);
  for (int v = 0; v < terms; v++) {
    for (int e = 0; e < MAC_ELEMS; e++)
      for (int w = 0; w < 8; w++)
        if (t.at(v, e, 0)[w] != 0xdeadbeefu || t.at(v, e, 2)[w] != 0xdeadbeefu) return -2;
    for (int j = 0; j < MAC_SCHED_WORDS; j++)
      if (s.at(j, v, 0) != 0xdeadbeefu || s.at(j, v, 2) != 0xdeadbeefu) return -2;
  }
  return code;
}
// the longest schedule among the scalars (what bounds the doubling chain), -1 if one is >= r
extern "C" int pmac_steps(const u32* scalars, int terms) {
  std::vector<u32> sched(MAC_SCHED_WORDS * terms, 0);
  const MacSched s{sched.data(), 1, terms};
  u32 tmp[SCALE_MAX_STEPS / 8];
  int top = 0;
  for (int v = 0; v < terms; v++) {
    mac_recode_scalar(scalars + 8 * v, tmp, s, v, 0);
    const int32_t len = (int32_t)s.at(MAC_WORDS, v, 0);
    if (len < 0) return -1;
    top = len > top ? len : top;
  }
  return top;
}
