// TEST INFRASTRUCTURE: the DEVICE build of the group law (ec.cuh over G1Cfg and G2Cfg, glv.cuh, the lane-group
// conversions of quad.cuh / fq2.cuh), operation by operation.  hostcheck.cpp reaches these functions through chains of
// canonical wire inputs, the kernel tests through whole MSMs, FFTs and codecs; here every entry point of group_ops.h runs
// alone in a kernel of its own, one case per lane (one per lane group for list 3), on raw-limb operands in every
// representative their types admit.  Compiled with the library's own hipcc flags (octopuszk_amd/build.py HIPCC_FLAGS),
// never linked into libozk_hip.so; driven by tests/grouparith.py and tests/test_group_ops_gpu.py.
// groupcheck_host.cpp is the same table under g++.
#include "../../octopuszk_amd/csrc/fq2.cuh"
#include "../../octopuszk_amd/csrc/quad.cuh"
#include "../../octopuszk_amd/csrc/glv.cuh"
#include "devcheck_common.h"
#include "group_ops.h"
using ozk::u32;

// list: 0 = G1Cfg, 1 = G2Cfg, 2 = no curve (the GLV split), 3 = lane-group conversions (device only)
extern "C" int gc_count(int list) {
  return gc::by_list(list, [](auto l) { return (int)dc::Nth<decltype(l)>::N; });
}
// name: at least 32 bytes; v: at least 4 + 2 * (NIN + NOUT) ints (128 hold every operation)
extern "C" int gc_info(int list, int idx, char* name, int* v) {
  return gc::by_list(list, [&](auto l) { return dc::info<decltype(l)>(idx, name, v); });
}
// in: NIN x n records of 9 words, out: n x NOUT records, both device buffers; n a multiple of the operation's group
extern "C" int gc_run(int list, int idx, const void* in, void* out, int n, void* stream) {
  constexpr int BLOCK = 256, LB = 1024;  // as devcheck.hip: 256 lanes per block, the compiler's default launch bound
  if (n <= 0) return -3;
  return gc::by_list(list, [&](auto l) {
    return dc::launch<decltype(l), LB>(idx, (const u32*)in, (u32*)out, nullptr, n, BLOCK, (hipStream_t)stream);
  });
}
extern "C" int gc_is_device() { return 1; }
