// TEST INFRASTRUCTURE: the DEVICE build of the pairing tower (fq12.cuh, gt_pow of batch_verify.cuh), operation by
// operation.  On the device every OZK_BIG function is __noinline__ and passes its arguments and results through the
// private stack, which tests/native/pairing_hostcheck.cpp (g++: everything inlined, the host branch of fp29.cuh)
// cannot reach, and which the pairing tests see only through whole pairings.  One kernel per operation of
// tower_ops.h, 64 lanes per workgroup under __launch_bounds__(64) as pairing.hip launches its own, one case per lane.
// Compiled with the library's own hipcc flags (octopuszk_amd/build.py HIPCC_FLAGS), never linked into libozk_hip.so;
// driven by tests/towerarith.py and tests/test_tower_ops_gpu.py.  towercheck_host.cpp is the same table under g++.
#define OZK_BV_NO_KERNELS
#include "../../octopuszk_amd/csrc/batch_verify.cuh"
#include "devcheck_common.h"
#include "tower_ops.h"
using ozk::u32;

extern "C" int tc_count() { return dc::Nth<tc::List>::N; }
// name: at least 32 bytes; v: at least 4 + 2 * (NIN + NOUT) ints (128 hold every operation)
extern "C" int tc_info(int idx, char* name, int* v) { return dc::info<tc::List>(idx, name, v); }
// words of scratch the operation needs per lane (0: none)
extern "C" int tc_scratch(int idx) { return dc::scratch_words<tc::List>(idx); }
// in: NIN x n records of 9 words, out: n x NOUT records, scratch: n x tc_scratch(idx) words; all device buffers
extern "C" int tc_run(int idx, const void* in, void* out, void* scratch, int n, void* stream) {
  if (n <= 0) return -3;
  return dc::launch<tc::List, 64>(idx, (const u32*)in, (u32*)out, (u32*)scratch, n, 64, (hipStream_t)stream);
}
extern "C" int tc_is_device() { return 1; }
