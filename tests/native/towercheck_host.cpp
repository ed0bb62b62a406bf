// TEST INFRASTRUCTURE: the operation table of towercheck.hip (tower_ops.h) compiled for the HOST with g++, behind the
// same tc_count / tc_info / tc_run, over host memory.  So the cases and expectations of tests/towerarith.py, and the
// host branch of the tower, are checked without a GPU (tests/test_tower_ops_cpu.py).  Not linked into the library.
#include "../../octopuszk_amd/csrc/batch_verify.cuh"
#include "devcheck_common.h"
#include "tower_ops.h"
using namespace dc;

template <class Op>
static void run_lanes(const u32* in, u32* out, u32* scratch, int n) {
  constexpr int NIN = Op::In::N, NOUT = Bnd<OutT<Op>>::N;
  for (int i = 0; i < n; i++) {
    const u32* x[NIN];
    for (int k = 0; k < NIN; k++) x[k] = in + ((size_t)k * n + i) * 9;
    if constexpr (Op::SCRATCH > 0) {
      Raw<OutT<Op>>::st(Op::run(x, scratch + i, n), out + (size_t)i * NOUT * 9);
    } else {
      Raw<OutT<Op>>::st(Op::run(x), out + (size_t)i * NOUT * 9);
    }
  }
}
template <class L, int I = 0>
static int run(int idx, const u32* in, u32* out, u32* scratch, int n) {
  if constexpr (I == Nth<L>::N) {
    return -1;
  } else {
    if (idx != I) return run<L, I + 1>(idx, in, out, scratch, n);
    using Op = typename At<I, L>::type;
    if (Op::SCRATCH > 0 && scratch == nullptr) return -5;
    run_lanes<Op>(in, out, scratch, n);
    return 0;
  }
}

extern "C" int tc_count() { return Nth<tc::List>::N; }
extern "C" int tc_info(int idx, char* name, int* v) { return info<tc::List>(idx, name, v); }
extern "C" int tc_scratch(int idx) { return scratch_words<tc::List>(idx); }
// as towercheck.hip's, with host buffers; the stream is ignored
extern "C" int tc_run(int idx, const void* in, void* out, void* scratch, int n, void*) {
  if (n <= 0) return -3;
  return run<tc::List>(idx, (const u32*)in, (u32*)out, (u32*)scratch, n);
}
extern "C" int tc_is_device() { return 0; }
