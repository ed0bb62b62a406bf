// TEST INFRASTRUCTURE: the operation table of groupcheck.hip (group_ops.h) compiled for the HOST with g++, behind the
// same gc_count / gc_info / gc_run, over host memory.  So the cases and expectations of tests/grouparith.py, and the
// host branch of the group law, are checked without a GPU (tests/test_group_ops_cpu.py).  Not linked into the library.
#include "../../octopuszk_amd/csrc/fq2.cuh"
#include "../../octopuszk_amd/csrc/glv.cuh"
#include "devcheck_common.h"
#include "group_ops.h"
using namespace dc;

template <class Op>
static void run_lanes(const u32* in, u32* out, int n) {
  constexpr int NIN = Op::In::N, NOUT = Bnd<OutT<Op>>::N;
  for (int i = 0; i < n; i++) {
    const u32* x[NIN];
    for (int k = 0; k < NIN; k++) x[k] = in + ((size_t)k * n + i) * 9;
    Raw<OutT<Op>>::st(Op::run(x), out + (size_t)i * NOUT * 9);
  }
}
template <class L, int I = 0>
static int run(int idx, const u32* in, u32* out, int n) {
  if constexpr (I == Nth<L>::N) {
    return -1;
  } else {
    if (idx != I) return run<L, I + 1>(idx, in, out, n);
    run_lanes<typename At<I, L>::type>(in, out, n);
    return 0;
  }
}

extern "C" int gc_count(int list) {
  return gc::by_list(list, [](auto l) { return (int)Nth<decltype(l)>::N; });
}
extern "C" int gc_info(int list, int idx, char* name, int* v) {
  return gc::by_list(list, [&](auto l) { return info<decltype(l)>(idx, name, v); });
}
// as groupcheck.hip's, with host buffers; the stream is ignored
extern "C" int gc_run(int list, int idx, const void* in, void* out, int n, void*) {
  if (n <= 0) return -3;
  return gc::by_list(list, [&](auto l) { return run<decltype(l)>(idx, (const u32*)in, (u32*)out, n); });
}
extern "C" int gc_is_device() { return 0; }
