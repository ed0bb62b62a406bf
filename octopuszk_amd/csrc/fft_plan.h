// What bace.hip takes from fft.hip: a domain's twiddle tables, from the plan cache or built per call, and the tiled
// transform over them.  Everything else of fft.hip is private to that unit.
#pragma once
#include "fr_tables.cuh"

namespace ozk {

// A cached plan stays pinned from domain_tables until the caller has enqueued its last kernel that reads the tables.
struct FftPlan;
struct PlanPin {
  FftPlan* p = nullptr;
  ~PlanPin();
};

// The tables of the domain (n, omega[, g]) for one call: those of the cached plan, pinned in `pin`, else the caller's
// own `*t` (carved from its workspace) with their build enqueued on `st`.  by_value: omega is a temporary of the
// caller and goes up as a kernel argument, not as an asynchronous copy.
int domain_tables(int n, const uint8_t* omega, const uint8_t* g, bool by_value, DomainTables* t, PlanPin& pin,
                  hipStream_t st);

// The transform proper: d_in (n x 8 words) -> d_out (n x out_stride words) over the twiddle pyramid tw, through the
// ping-pong buffers buf0 / buf1.  batch > 1 (n >= 1024 only): `batch` columns, column c from d_in + c in_cs to
// d_out + c out_cs (words), the buffers batch x n x 8 words each.
int fft_core(const u32* d_in, int n, const u32* tw, u32* d_out, int out_stride, u32* buf0, u32* buf1, hipStream_t st,
             const u32* scale = nullptr, int batch = 1, size_t in_cs = 0, size_t out_cs = 0);

}  // namespace ozk
