// The witness of the PLONK prover built on the device: the running sums of a stream of terms
// coeff * vec[index], and the gather of the wire columns from cell descriptors.  A section of the plonk.hip unit, which
// alone includes it, after plonk_lookup.cuh: the sums run the three phases of that file's running sum (its tile sum of
// a lane, its carries kernel and its workspace layout) over the staged tile and the scan of fr_rows.cuh.  Values in
// HBM are 32 bytes LE, plain; inputs are taken mod r, outputs are canonical.
//
// Term sums.  out[t] = sum_{u <= t} coeff[u] vec[index[u]] over the whole stream, not segmented: the accumulator of a
// chain of an imported R1CS is the difference of two elements, which the gather takes.  A workgroup of PLONK_WG lanes
// owns a tile of PLONK_TILE terms, a lane PLONK_L consecutive ones: it reads its indices as two 16-byte words, gathers
// the elements they name and multiplies each by its coefficient, which arrives through the staged tile (coalesced) in
// the form the kernel multiplies by, c R mod r, so that the product with a plain element is plain and no conversion
// is made.  The tile is then free and takes the sums on their way out.  An index >= n_vec is not read: its term is
// zero and it is counted (in the tile pass alone, so once).
//   products per term and pass: 1 with coefficients, else none; bytes per term and pass: 4 + 32 read (+ 32 with
//   coefficients), two passes (one when terms <= PLONK_TILE), 32 written.  LDS: one tile and the scan, 37.5 KiB.
//
// Wires.  One lane per cell of k rows of len: a descriptor (hi, lo) of two u32, read coalesced, names src[hi] - src[lo],
// or src[hi] alone when lo is WIRE_NONE.  Two gathers of 32 bytes, one subtraction, one coalesced write; a descriptor
// that points outside src is not followed: its cell is zero and it is counted.
//   bytes per cell: 8 + 32 (or 64) read, 32 written.
#pragma once
#include "plonk_lookup.cuh"

namespace ozk {

constexpr u32 WIRE_NONE = 0xffffffffu;            // the `lo` of a descriptor that names one element
constexpr int WIRE_WG = 256;
constexpr long long R1CS_MAX_SRC = 0xffffffffll;   // elements of vec / src: every index stays below WIRE_NONE

#if defined(__HIPCC__)
// f[k] = coeff vec[index] (plain, below 2 r) of the lane's terms t PLONK_TILE + PLONK_L threadIdx.x + k, zero for a term
// beyond `terms` and for an index >= n_vec; returns how many of the latter the lane met.  The tile is free on return.
template <bool COEFF>
__device__ __forceinline__ int r1cs_terms(const u32* __restrict__ index, const u32* __restrict__ coeff,
                                          const u32* __restrict__ vec, u32 n_vec, int terms, int t, u32* tile,
                                          KzgV (&f)[PLONK_L]) {
  static_assert(PLONK_L == 8, "a lane's indices are two 16-byte words");
  const int l = threadIdx.x;
  const long long j0 = (long long)t * PLONK_TILE + (long long)l * PLONK_L;
  u32 ix[PLONK_L];
  if (j0 + PLONK_L <= terms) {
    const uint4* p = reinterpret_cast<const uint4*>(index + j0);
    const uint4 a = p[0], b = p[1];
    ix[0] = a.x, ix[1] = a.y, ix[2] = a.z, ix[3] = a.w, ix[4] = b.x, ix[5] = b.y, ix[6] = b.z, ix[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < PLONK_L; k++) ix[k] = j0 + k < terms ? index[j0 + k] : 0u;
  }
  if (COEFF) {
    fr_tile_fill<PLONK_WG, PLONK_L>(coeff, terms, t, tile);
    block_sync();
  }
  int wrong = 0;
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    f[k] = KzgV(fe_zero<FrP>());
    if (j0 + k >= terms) continue;
    if (ix[k] >= n_vec) {
      wrong++;
      continue;
    }
    const KzgV v = KzgV(reduce_to<32>(fr_load<85>(vec + (size_t)ix[k] * 8)));
    if (COEFF) f[k] = KzgV(mul(v, fr_tile_get(tile, l * PLONK_L + k)));
    else f[k] = v;
  }
  if (COEFF) block_sync();
  return wrong;
}

// first pass (several tiles): the sum of tile t to agg[t]
template <bool COEFF>
__global__ void __launch_bounds__(PLONK_WG) k_fr_term_sums_tiles(const u32* __restrict__ index, const u32* __restrict__ coeff,
                                                                const u32* __restrict__ vec, u32 n_vec, int terms,
                                                                u32* __restrict__ agg) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  KzgV f[PLONK_L];
  r1cs_terms<COEFF>(index, coeff, vec, n_vec, terms, blockIdx.x, tile, f);
  const KzgV s = fr_wg_scan<PLONK_WG, false>(plonk_lane_sum(f), FrScanSum{}, part);
  if (threadIdx.x == PLONK_WG - 1) fr_store(canonical(s), agg + (size_t)blockIdx.x * 8);
}
// (second pass: k_plonk_lookup_sum_carries, carry[t] = the sum of the tiles below t)
// the tile pass: the sums and the count of indices outside vec.  carry: null when the stream is one tile.
template <bool COEFF>
__global__ void __launch_bounds__(PLONK_WG) k_fr_term_sums_apply(const u32* __restrict__ index, const u32* __restrict__ coeff,
                                                                const u32* __restrict__ vec, u32 n_vec, int terms,
                                                                const u32* __restrict__ carry, u32* __restrict__ out,
                                                                int* __restrict__ bad) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  const int t = blockIdx.x, l = threadIdx.x;
  KzgV f[PLONK_L];
  const int wrong = r1cs_terms<COEFF>(index, coeff, vec, n_vec, terms, t, tile, f);
  if (wrong) atomicAdd(bad, wrong);
  KzgV below = KzgV(fe_zero<FrP>());
  if (carry) below = KzgV(fr_load<16>(carry + (size_t)t * 8));
  KzgV sum = plonk_lane_sum(f);
  if (l == 0) sum = KzgV(reduce_to<32>(add(sum, below)));
  fr_wg_scan<PLONK_WG, false>(sum, FrScanSum{}, part);
  // the sum below the lane's first term, then the lane's own terms one by one
  KzgV run = fr_scan_neighbour<PLONK_WG, false>(part, below);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    run = KzgV(reduce_to<32>(add(run, f[k])));
    fr_tile_put(tile, l * PLONK_L + k, canonical(run));
  }
  block_sync();
  fr_tile_store<PLONK_WG, PLONK_L>(tile, t, terms, 0, nullptr, 0, out);
}

// ---- the gather of the wire columns: cell g % len of row g / len
__global__ void __launch_bounds__(WIRE_WG) k_plonk_wires(const u32* __restrict__ src, u32 n_src, const u32* __restrict__ cells,
                                                         unsigned cells_total, unsigned len, size_t cell_cs,
                                                         u32* __restrict__ out, size_t out_cs, int* __restrict__ bad) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= cells_total) return;
  const unsigned y = g / len, i = g - y * len;
  const uint2 d = *reinterpret_cast<const uint2*>(cells + (size_t)y * cell_cs + (size_t)i * 2);
  u32* o = out + (size_t)y * out_cs + (size_t)i * 8;
  if (d.x >= n_src || (d.y != WIRE_NONE && d.y >= n_src)) {
    const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    fr_store_words(zero, o);
    atomicAdd(bad, 1);
    return;
  }
  const KzgV hi = KzgV(reduce_to<32>(fr_load<85>(src + (size_t)d.x * 8)));
  if (d.y == WIRE_NONE) {
    fr_store(canonical(hi), o);
  } else {
    const KzgV lo = KzgV(reduce_to<32>(fr_load<85>(src + (size_t)d.y * 8)));
    fr_store(canonical(sub(hi, lo)), o);
  }
}

// ---- host side ----
static bool r1cs_src_ok(long long n) { return n >= 1 && n <= R1CS_MAX_SRC; }
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

size_t ozk_fr_term_sums_workspace_bytes(int32_t terms) {
  if (!plonk_perm_shape_ok(terms)) return 0;
  return plonk_lookup_sum_layout(terms, nullptr).bytes;
}

int ozk_fr_term_sums_dev(const void* d_index, const void* d_coeff, const void* d_vec, int64_t n_vec, int32_t terms,
                         void* d_out, int32_t* d_bad, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!plonk_perm_shape_ok(terms)) return fail(OZK_E_INVALID, "bad shape: %d terms (1 <= terms <= 2^28)", terms);
  if (!r1cs_src_ok(n_vec)) return fail(OZK_E_INVALID, "bad shape: n_vec %lld (1 <= n_vec < 2^32)", (long long)n_vec);
  if (int rc = fr_check_pointers(d_index, d_vec, d_out, d_bad, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_index, d_vec, d_out)) return rc;
  if (d_coeff && kzg_misaligned16(d_coeff)) return fail(OZK_E_INVALID, "elements must be 16-byte aligned");
  if (lookup_misaligned4(d_bad)) return fail(OZK_E_INVALID, "d_bad must be 4-byte aligned");
  const size_t row = (size_t)terms * 32;
  const struct { const void* p; size_t n; } in[3] = {{d_index, (size_t)terms * 4}, {d_vec, (size_t)n_vec * 32},
                                                    {d_coeff, d_coeff ? row : 0}};
  for (const auto& r : in)
    if (r.n && (kzg_overlap(r.p, r.n, d_out, row) || kzg_overlap(r.p, r.n, d_bad, 4)))
      return fail(OZK_E_INVALID, "an output overlaps d_index, d_coeff or d_vec");
  if (kzg_overlap(d_out, row, d_bad, 4)) return fail(OZK_E_INVALID, "d_out and d_bad overlap");
  const PlonkLookupSumLayout L = plonk_lookup_sum_layout(terms, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  for (const auto& r : in)
    if (r.n && kzg_overlap(r.p, r.n, d_workspace, L.bytes))
      return fail(OZK_E_INVALID, "d_workspace overlaps d_index, d_coeff or d_vec");
  if (kzg_overlap(d_out, row, d_workspace, L.bytes) || kzg_overlap(d_bad, 4, d_workspace, L.bytes))
    return fail(OZK_E_INVALID, "d_workspace overlaps d_out or d_bad");
  hipStream_t st = (hipStream_t)stream;
  const u32 *ix = (const u32*)d_index, *co = (const u32*)d_coeff, *v = (const u32*)d_vec;
  const u32* carry = L.nt > 1 ? L.carry : nullptr;
  OZK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
  if (L.nt > 1) {
    if (co) hipLaunchKernelGGL(k_fr_term_sums_tiles<true>, dim3(L.nt), dim3(PLONK_WG), 0, st, ix, co, v, (u32)n_vec, terms, L.agg);
    else hipLaunchKernelGGL(k_fr_term_sums_tiles<false>, dim3(L.nt), dim3(PLONK_WG), 0, st, ix, co, v, (u32)n_vec, terms, L.agg);
    hipLaunchKernelGGL(k_plonk_lookup_sum_carries, dim3(1), dim3(PLONK_SCAN_WG), 0, st, (const u32*)L.agg, L.nt, L.carry);
  }
  if (co) hipLaunchKernelGGL(k_fr_term_sums_apply<true>, dim3(L.nt), dim3(PLONK_WG), 0, st, ix, co, v, (u32)n_vec, terms, carry,
                             (u32*)d_out, (int*)d_bad);
  else hipLaunchKernelGGL(k_fr_term_sums_apply<false>, dim3(L.nt), dim3(PLONK_WG), 0, st, ix, co, v, (u32)n_vec, terms, carry,
                          (u32*)d_out, (int*)d_bad);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_plonk_wires_dev(const void* d_src, int64_t n_src, const void* d_cells, int32_t k, int32_t len, int64_t cell_stride,
                        void* d_out, int64_t out_stride, int32_t* d_bad, void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(k, len)) return fail(OZK_E_INVALID, "bad shape: %d rows of %d cells (1 <= k, 1 <= len, k len <= 2^28)", k, len);
  if (!r1cs_src_ok(n_src)) return fail(OZK_E_INVALID, "bad shape: n_src %lld (1 <= n_src < 2^32)", (long long)n_src);
  if (cell_stride < len || out_stride < len)
    return fail(OZK_E_INVALID, "bad strides: cell_stride %lld, out_stride %lld (both >= len %d)", (long long)cell_stride,
                (long long)out_stride, len);
  if (int rc = fr_check_pointers(d_src, d_cells, d_out, d_bad)) return rc;
  if (int rc = fr_check_aligned16(d_src, d_out)) return rc;
  if (((uintptr_t)d_cells & 7) != 0) return fail(OZK_E_INVALID, "d_cells must be 8-byte aligned");
  if (lookup_misaligned4(d_bad)) return fail(OZK_E_INVALID, "d_bad must be 4-byte aligned");
  const size_t src_bytes = (size_t)n_src * 32, out_bytes = kzg_span(k, len, out_stride);
  const size_t cell_bytes = ((size_t)(k - 1) * (size_t)cell_stride + (size_t)len) * 8;
  if (kzg_overlap(d_src, src_bytes, d_out, out_bytes) || kzg_overlap(d_cells, cell_bytes, d_out, out_bytes))
    return fail(OZK_E_INVALID, "d_out overlaps d_src or d_cells");
  if (kzg_overlap(d_src, src_bytes, d_bad, 4) || kzg_overlap(d_cells, cell_bytes, d_bad, 4) ||
      kzg_overlap(d_out, out_bytes, d_bad, 4))
    return fail(OZK_E_INVALID, "d_bad overlaps d_src, d_cells or d_out");
  hipStream_t st = (hipStream_t)stream;
  const unsigned total = (unsigned)((long long)k * len);
  OZK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
  hipLaunchKernelGGL(k_plonk_wires, dim3((total + WIRE_WG - 1) / WIRE_WG), dim3(WIRE_WG), 0, st, (const u32*)d_src, (u32)n_src,
                     (const u32*)d_cells, total, (unsigned)len, (size_t)cell_stride * 2, (u32*)d_out, (size_t)out_stride * 8,
                     (int*)d_bad);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
