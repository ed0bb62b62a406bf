// The Fr kernels of KZG openings: the quotient (p(X) - p(z)) / (X - z) with the value p(z),
// in coefficient form and in evaluation form, and a weighted sum of rows.  A section of the kzg.hip unit, which alone
// includes it for the device: kernels, layouts and entry points.  The per-lane pieces, the staged tile, the scan and the
// entry checks are fr_rows.cuh's, element I/O, power table and block sum fr_tables.cuh's; what is outside __HIPCC__
// compiles for the host too (tests/native/kzg_hostcheck.cpp).
//
// Every value in HBM is 32 bytes LE, plain (non-Montgomery); inputs are taken mod r, outputs are canonical.
//
// Coefficient form.  h_j = p_j + z h_{j+1}, h_len = 0 is Horner's rule run from the top: y = h_0 and q_{j-1} = h_j.
// A workgroup stages a tile of KZG_TILE coefficients in LDS (coalesced 32-byte reads), a lane runs the recurrence over
// its KZG_L consecutive elements of the tile (kzg_piece, carry 0), and the carry into every lane,
// S_l = a_l + z^L S_{l+1}, is a suffix scan over the workgroup (fr_wg_scan: log2 256 steps, one product each).  The
// lane then runs the recurrence again from its carry and the tile goes out through LDS, coalesced.  With more than
// one tile per row a first pass leaves every tile's value at z in the workspace, one workgroup per row scans them
// (the same scan with z^T), and the tile pass starts from the carry into its tile.
//   products per coefficient: 2 (the two runs of the recurrence) + 16 / KZG_L (the scan) per tile pass,
//   1 + 16 / KZG_L in the first pass; bytes: 32 read + 32 written, and 32 read again when a row has several tiles.
//
// Evaluation form.  With inv_i = 1 / (omega^i - z): y = (z^n - 1) / n * sum_i f_i omega^i / (z - omega^i) and
// q_i = (f_i - y) inv_i.  A lane inverts KZG_INV_BATCH interleaved differences with one safegcd inversion
// (kzg_chunk_inverses: a zero difference is left out of the running product and gets inverse 0, the convention of
// inv) and leaves the inverses in the quotient row; the sums go through the block sum and per-workgroup partials.
// z = omega^k is found by the lane that meets the zero difference, which leaves k + 1 in the row's flag: then
// y = f_k and q_k = -omega^-k sum_{i != k} q_i omega^i, finished by one workgroup per row.  No host round trip.
//   products per evaluation: 6 + an inversion per KZG_INV_BATCH (first pass), 1 (second pass; 3 with z in the
//   domain); bytes: 32 read + 32 written in the first pass, 64 read + 32 written in the second.
#pragma once
#include "fp29.cuh"
#include "fr_rows.cuh"

namespace ozk {

#if defined(__HIPCC__)
// ---- coefficient form ----
__global__ void __launch_bounds__(64) k_kzg_open_consts(const u32* __restrict__ points, int npolys, KzgRow* __restrict__ rows) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= npolys) return;
  kzg_row_consts(ElemTraits<Fe<FrP, 17>>::from_wire(points + (size_t)y * 8), rows + y, nullptr);
}

// the tile's coefficients (canonical; zero beyond len) into LDS, then the lane's own KZG_L of them
__device__ __forceinline__ void kzg_tile_load(const u32* __restrict__ row, int len, int t, u32* tile, Fe<FrP, 16> (&p)[KZG_L]) {
  fr_tile_fill<KZG_WG, KZG_L>(row, len, t, tile);
  block_sync();
#pragma unroll
  for (int i = 0; i < KZG_L; i++) p[i] = fr_tile_get(tile, threadIdx.x * KZG_L + i);
}

// first pass (rows of several tiles): the value of tile t of row y at z, to agg[y nt + t]
__global__ void __launch_bounds__(KZG_WG) k_kzg_open_tiles(const u32* __restrict__ coeffs, size_t poly_cs, int len, int nt,
                                                          const KzgRow* __restrict__ rows, u32* __restrict__ agg) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * KZG_WG];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const int y = blockIdx.x / nt, t = blockIdx.x % nt;
  Fe<FrP, 16> p[KZG_L];
  kzg_tile_load(coeffs + (size_t)y * poly_cs, len, t, tile, p);
  const KzgV a = kzg_piece<KZG_L, false>(p, KZG_L, E16::load(rows[y].z), KzgV(fe_zero<FrP>()), nullptr);
  const KzgV s = fr_wg_scan<KZG_WG, true>(a, FrScanAffine{KzgV(E16::load(rows[y].zl))}, part);
  if (threadIdx.x == 0) fr_store(canonical(s), agg + (size_t)blockIdx.x * 8);
}
// second pass, one workgroup per row: carry[y nt + t] = h at the first coefficient of tile t + 1, 256 tiles at a time
// from the top
__global__ void __launch_bounds__(KZG_WG) k_kzg_open_carries(const u32* __restrict__ agg, int nt, const KzgRow* __restrict__ rows,
                                                            u32* __restrict__ carry) {
  __shared__ u32 part[9 * KZG_WG];
  const size_t y = blockIdx.x;
  const FrScanAffine op{KzgV(ElemTraits<Fe<FrP, 16>>::load(rows[y].zt))};
  fr_carries_scan<KZG_WG, true>(agg + y * nt * 8, nt, op, carry + y * nt * 8, part);
}
// the tile pass: quotient and value.  carry: null when every row is one tile.
__global__ void __launch_bounds__(KZG_WG) k_kzg_open_apply(const u32* __restrict__ coeffs, size_t poly_cs, int len, int nt,
                                                          const KzgRow* __restrict__ rows, const u32* __restrict__ carry,
                                                          u32* __restrict__ quot, size_t quot_cs, u32* __restrict__ values) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * KZG_WG];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const int y = blockIdx.x / nt, t = blockIdx.x % nt, l = threadIdx.x;
  Fe<FrP, 16> p[KZG_L];
  kzg_tile_load(coeffs + (size_t)y * poly_cs, len, t, tile, p);
  const auto z = E16::load(rows[y].z);
  const KzgV zl = KzgV(E16::load(rows[y].zl));
  KzgV above = KzgV(fe_zero<FrP>());
  if (carry) above = KzgV(fr_load<16>(carry + (size_t)blockIdx.x * 8));
  KzgV a = kzg_piece<KZG_L, false>(p, KZG_L, z, KzgV(fe_zero<FrP>()), nullptr);
  if (l == KZG_WG - 1) a = kzg_compose(a, zl, above);
  fr_wg_scan<KZG_WG, true>(a, FrScanAffine{zl}, part);
  KzgV h[KZG_L];
  kzg_piece<KZG_L, true>(p, KZG_L, z, fr_scan_neighbour<KZG_WG, true>(part, above), h);
  // (a lane overwrites the elements it alone has read)
#pragma unroll
  for (int i = 0; i < KZG_L; i++) fr_tile_put(tile, l * KZG_L + i, canonical(h[i]));
  block_sync();
  // q_j = h_{j+1}: element e of the tile receives h of element e + 1, the last one what lies above the tile
  u32 top[8];
  pack(canonical(above), top);
  fr_tile_store<KZG_WG, KZG_L>(tile, t, len, 1, top, 0, quot + (size_t)y * quot_cs);
  if (t == 0 && l == 0) fr_store(canonical(h[0]), values + (size_t)y * 8);
}

// ---- evaluation form ----
struct KzgEvRow {
  u32 z[8];      // z, Montgomery form
  u32 c[8];      // (z^n - 1) / n, Montgomery form
  u32 y[8];      // the value, plain canonical (k_kzg_ev_value)
};
__global__ void __launch_bounds__(64) k_kzg_ev_consts(const u32* __restrict__ points, int npolys, int n,
                                                      KzgEvRow* __restrict__ rows, u32* __restrict__ flags) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= npolys) return;
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const auto z = ElemTraits<Fe<FrP, 17>>::from_wire(points + (size_t)y * 8);
  const u32 nw[8] = {(u32)n, 0, 0, 0, 0, 0, 0, 0};
  const auto Z = sub(fe_pow_u32(z, (unsigned)n), fe_one<FrP>());
  E16::store(canonical(z), rows[y].z);
  E16::store(canonical(mul(Z, inv(to_mont<FrP>(nw)))), rows[y].c);
  flags[y] = 0;
}
// first pass: inv_i to quot[i] (Montgomery form), the workgroup's part of sum_i f_i omega^i inv_i to partial, and
// flags[y] = k + 1 where omega^k = z
__global__ void __launch_bounds__(KZG_WG) k_kzg_ev_inv(const u32* __restrict__ evals, size_t ev_cs, int n, int nb,
                                                      const KzgEvRow* __restrict__ rows, const u32* __restrict__ pw, int lo,
                                                      u32* __restrict__ flags, u32* __restrict__ quot, size_t quot_cs,
                                                      u32* __restrict__ partial) {
  __shared__ u32 part[9 * 256];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const int y = blockIdx.x / nb, blk = blockIdx.x % nb;
  const int lanes = (n + KZG_INV_BATCH - 1) / KZG_INV_BATCH;
  const auto z = E16::load(rows[y].z);
  const u32* f = evals + (size_t)y * ev_cs;
  u32* q = quot + (size_t)y * quot_cs;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  const int t = blk * KZG_WG + threadIdx.x;
  if (t < lanes) {
    KzgV w[KZG_INV_BATCH], d[KZG_INV_BATCH], di[KZG_INV_BATCH];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < KZG_INV_BATCH; k++) {
      const int i = k * lanes + t;   // (interleaved: once i >= n, every later k is too)
      if (i < n) {
        w[k] = KzgV(pow_at(pw, lo, i));
        d[k] = KzgV(reduce_to<32>(sub(w[k], z)));
        if (is_zero(d[k])) flags[y] = (u32)i + 1;
        cnt = k + 1;
      }
    }
    kzg_chunk_inverses<KZG_INV_BATCH>(d, cnt, di);
#pragma unroll
    for (int k = 0; k < KZG_INV_BATCH; k++) {
      const int i = k * lanes + t;
      if (i < n) {
        fr_store(canonical(di[k]), q + (size_t)i * 8);
        acc = FrAcc(reduce_to<32>(add(acc, mul(fr_load<85>(f + (size_t)i * 8), mul(w[k], di[k])))));
      }
    }
  }
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x == 0) fr_store(canonical(sum), partial + (size_t)blockIdx.x * 8);
}
// one workgroup per row: y = -c sum, or f_k for z = omega^k
__global__ void __launch_bounds__(256) k_kzg_ev_value(const u32* __restrict__ partial, int nb, const u32* __restrict__ evals,
                                                      size_t ev_cs, KzgEvRow* __restrict__ rows, const u32* __restrict__ flags,
                                                      u32* __restrict__ values) {
  __shared__ u32 part[9 * 256];
  const int y = blockIdx.x;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = threadIdx.x; i < nb; i += 256)
    acc = FrAcc(reduce_to<32>(add(acc, fr_load<16>(partial + ((size_t)y * nb + i) * 8))));
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x != 0) return;
  u32 o[8];
  const u32 k1 = flags[y];
  if (k1) pack(canonical(fr_load<85>(evals + (size_t)y * ev_cs + (size_t)(k1 - 1) * 8)), o);
  else pack(canonical(neg(mul(sum, ElemTraits<Fe<FrP, 16>>::load(rows[y].c)))), o);
  fr_store_words(o, values + (size_t)y * 8);
#pragma unroll
  for (int i = 0; i < 8; i++) rows[y].y[i] = o[i];
}
// second pass: q_i = (f_i - y) inv_i in place of inv_i; for z in the domain also the workgroup's part of
// sum_i q_i omega^i (inv_k = 0, so the term of k is 0)
__global__ void __launch_bounds__(KZG_WG) k_kzg_ev_quot(const u32* __restrict__ evals, size_t ev_cs, int n, int nb,
                                                       const KzgEvRow* __restrict__ rows, const u32* __restrict__ pw, int lo,
                                                       const u32* __restrict__ flags, u32* __restrict__ quot, size_t quot_cs,
                                                       u32* __restrict__ partial) {
  __shared__ u32 part[9 * 256];
  const int y = blockIdx.x / nb, blk = blockIdx.x % nb;
  const bool inside = flags[y] != 0;   // (uniform over the workgroup)
  const auto yv = ElemTraits<Fe<FrP, 16>>::load(rows[y].y);
  const u32* f = evals + (size_t)y * ev_cs;
  u32* q = quot + (size_t)y * quot_cs;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  const int i = blk * KZG_WG + threadIdx.x;
  if (i < n) {
    const auto v = mul(sub(fr_load<85>(f + (size_t)i * 8), yv), fr_load<16>(q + (size_t)i * 8));
    fr_store(canonical(v), q + (size_t)i * 8);
    if (inside) acc = FrAcc(reduce_to<32>(add(acc, mul(v, pow_at(pw, lo, i)))));
  }
  if (!inside) return;
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x == 0) fr_store(canonical(sum), partial + (size_t)blockIdx.x * 8);
}
// z = omega^k: q_k = -omega^(n - k) sum_i q_i omega^i, one workgroup per row
__global__ void __launch_bounds__(256) k_kzg_ev_inside(const u32* __restrict__ partial, int nb, int n,
                                                       const u32* __restrict__ pw, int lo, const u32* __restrict__ flags,
                                                       u32* __restrict__ quot, size_t quot_cs) {
  __shared__ u32 part[9 * 256];
  const int y = blockIdx.x;
  const u32 k1 = flags[y];
  if (!k1) return;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = threadIdx.x; i < nb; i += 256)
    acc = FrAcc(reduce_to<32>(add(acc, fr_load<16>(partial + ((size_t)y * nb + i) * 8))));
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x != 0) return;
  const int k = (int)(k1 - 1);
  fr_store(canonical(neg(mul(sum, pow_at(pw, lo, n - k)))), quot + (size_t)y * quot_cs + (size_t)k * 8);
}

// ---- out_j = sum_i w_i rows[i][j]: one lane per column; out may be the first row (a lane writes the column it read)
__global__ void __launch_bounds__(256) k_fr_rows_combine(const u32* rows, int k, int len, size_t row_cs,
                                                         const u32* __restrict__ weights, u32* out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len) return;
  // x w / R per term; the sum times R^2 / R at the end
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = 0; i < k; i++)
    acc = FrAcc(reduce_to<32>(add(acc, mul(fr_load<85>(rows + (size_t)i * row_cs + (size_t)j * 8),
                                           fr_load<85>(weights + (size_t)i * 8)))));
  fr_store(canonical(mul(acc, fe_const<FrP, 16>(FrP::R2))), out + (size_t)j * 8);
}

// ---- host side ----
struct KzgOpenLayout {
  KzgRow* rows;
  u32 *agg, *carry;
  int nt;
  size_t bytes;
};
static KzgOpenLayout kzg_open_layout(int npolys, int len, void* wsp) {
  KzgOpenLayout L;
  Bump b(wsp, ~(size_t)0);
  L.nt = (len + KZG_TILE - 1) / KZG_TILE;
  L.rows = b.take<KzgRow>(npolys);
  const size_t per = L.nt > 1 ? (size_t)npolys * L.nt * 8 : 0;
  L.agg = b.take<u32>(per);
  L.carry = b.take<u32>(per);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
struct KzgEvLayout {
  KzgEvRow* rows;
  u32 *flags, *omega, *pw, *partial;
  int nb_inv, nb_quot;
  size_t bytes;
};
static int kzg_ev_blocks(int items) { return (items + KZG_WG - 1) / KZG_WG; }
static KzgEvLayout kzg_ev_layout(int npolys, int n, void* wsp) {
  KzgEvLayout L;
  Bump b(wsp, ~(size_t)0);
  L.nb_inv = kzg_ev_blocks((n + KZG_INV_BATCH - 1) / KZG_INV_BATCH);
  L.nb_quot = kzg_ev_blocks(n);
  L.rows = b.take<KzgEvRow>(npolys);
  L.flags = b.take<u32>(npolys);
  L.omega = b.take<u32>(8);
  L.pw = b.take<u32>(PowTable::upto(n).words());
  L.partial = b.take<u32>((size_t)npolys * L.nb_quot * 8);   // (nb_quot >= nb_inv: both passes use it in turn)
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

size_t ozk_fr_poly_open_workspace_bytes(int32_t npolys, int32_t len) {
  if (!kzg_shape_ok(npolys, len)) return 0;
  return kzg_open_layout(npolys, len, nullptr).bytes;
}

int ozk_fr_poly_open_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, const void* d_points,
                         void* d_quot, int64_t quot_stride, void* d_values, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(npolys, len))
    return fail(OZK_E_INVALID, "bad shape: %d polynomials of %d coefficients (1 <= both, product <= 2^28)", npolys, len);
  if ((poly_stride != 0 && poly_stride < len) || quot_stride < len)
    return fail(OZK_E_INVALID, "bad strides: poly_stride %lld (0 or >= len), quot_stride %lld (>= len), len %d",
                (long long)poly_stride, (long long)quot_stride, len);
  if (int rc = fr_check_pointers(d_coeffs, d_points, d_quot, d_values, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_coeffs, d_points, d_quot, d_values)) return rc;
  if (kzg_overlap(d_coeffs, kzg_span(npolys, len, poly_stride), d_quot, kzg_span(npolys, len, quot_stride)))
    return fail(OZK_E_INVALID, "d_quot overlaps d_coeffs");
  const KzgOpenLayout L = kzg_open_layout(npolys, len, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const u32* c = (const u32*)d_coeffs;
  const size_t pcs = (size_t)poly_stride * 8, qcs = (size_t)quot_stride * 8;
  const unsigned grid = (unsigned)((long long)npolys * L.nt);
  hipLaunchKernelGGL(k_kzg_open_consts, dim3((npolys + 63) / 64), dim3(64), 0, st, (const u32*)d_points, npolys, L.rows);
  if (L.nt > 1) {
    hipLaunchKernelGGL(k_kzg_open_tiles, dim3(grid), dim3(KZG_WG), 0, st, c, pcs, len, L.nt, (const KzgRow*)L.rows, L.agg);
    hipLaunchKernelGGL(k_kzg_open_carries, dim3(npolys), dim3(KZG_WG), 0, st, (const u32*)L.agg, L.nt,
                       (const KzgRow*)L.rows, L.carry);
  }
  hipLaunchKernelGGL(k_kzg_open_apply, dim3(grid), dim3(KZG_WG), 0, st, c, pcs, len, L.nt, (const KzgRow*)L.rows,
                     (const u32*)(L.nt > 1 ? L.carry : nullptr), (u32*)d_quot, qcs, (u32*)d_values);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_fr_evals_open_workspace_bytes(int32_t npolys, int32_t n) {
  if (!kzg_shape_ok(npolys, n) || n < 2 || (n & (n - 1))) return 0;
  return kzg_ev_layout(npolys, n, nullptr).bytes;
}

int ozk_fr_evals_open_dev(const void* d_evals, int32_t npolys, int32_t n, int64_t evals_stride, const uint8_t* omega_host32,
                          const void* d_points, void* d_quot, int64_t quot_stride, void* d_values, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(npolys, n))
    return fail(OZK_E_INVALID, "bad shape: %d rows of %d evaluations (1 <= both, product <= 2^28)", npolys, n);
  if (int rc = check_pow2(n, 2, "domain size")) return rc;
  if ((evals_stride != 0 && evals_stride < n) || quot_stride < n)
    return fail(OZK_E_INVALID, "bad strides: evals_stride %lld (0 or >= n), quot_stride %lld (>= n), n %d",
                (long long)evals_stride, (long long)quot_stride, n);
  if (int rc = fr_check_pointers(d_evals, omega_host32, d_points, d_quot, d_values, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_evals, d_points, d_quot, d_values)) return rc;
  if (kzg_overlap(d_evals, kzg_span(npolys, n, evals_stride), d_quot, kzg_span(npolys, n, quot_stride)))
    return fail(OZK_E_INVALID, "d_quot overlaps d_evals");
  if (!fr_omega_has_order(omega_host32, n))
    return fail(OZK_E_INVALID, "omega does not have order %d (omega^(n/2) != -1)", n);
  const KzgEvLayout L = kzg_ev_layout(npolys, n, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const u32* f = (const u32*)d_evals;
  const size_t ecs = (size_t)evals_stride * 8, qcs = (size_t)quot_stride * 8;
  fr_put_element(omega_host32, L.omega, st);
  const PowTable pt = PowTable::upto(n);
  pt.build(L.omega, L.pw, st);
  hipLaunchKernelGGL(k_kzg_ev_consts, dim3((npolys + 63) / 64), dim3(64), 0, st, (const u32*)d_points, npolys, n, L.rows,
                     L.flags);
  hipLaunchKernelGGL(k_kzg_ev_inv, dim3((unsigned)((long long)npolys * L.nb_inv)), dim3(KZG_WG), 0, st, f, ecs, n, L.nb_inv,
                     (const KzgEvRow*)L.rows, (const u32*)L.pw, pt.lo, L.flags, (u32*)d_quot, qcs, L.partial);
  hipLaunchKernelGGL(k_kzg_ev_value, dim3(npolys), dim3(256), 0, st, (const u32*)L.partial, L.nb_inv, f, ecs, L.rows,
                     (const u32*)L.flags, (u32*)d_values);
  hipLaunchKernelGGL(k_kzg_ev_quot, dim3((unsigned)((long long)npolys * L.nb_quot)), dim3(KZG_WG), 0, st, f, ecs, n,
                     L.nb_quot, (const KzgEvRow*)L.rows, (const u32*)L.pw, pt.lo, (const u32*)L.flags, (u32*)d_quot, qcs,
                     L.partial);
  hipLaunchKernelGGL(k_kzg_ev_inside, dim3(npolys), dim3(256), 0, st, (const u32*)L.partial, L.nb_quot, n,
                     (const u32*)L.pw, pt.lo, (const u32*)L.flags, (u32*)d_quot, qcs);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_fr_rows_combine_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const void* d_weights,
                            void* d_out, void* stream) {
  hip_clear_stale();
  if (k < 1 || len < 1 || row_stride < len || (long long)k * len > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad shape: %d rows of %d elements, stride %lld", k, len, (long long)row_stride);
  if (int rc = fr_check_pointers(d_rows, d_weights, d_out)) return rc;
  if (int rc = fr_check_aligned16(d_rows, d_weights, d_out)) return rc;
  if (d_out != d_rows && kzg_overlap(d_rows, kzg_span(k, len, row_stride), d_out, (size_t)len * 32))
    return fail(OZK_E_INVALID, "d_out overlaps d_rows (it may only be the first row itself)");
  hipLaunchKernelGGL(k_fr_rows_combine, dim3((len + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const u32*)d_rows, k,
                     len, (size_t)row_stride * 8, (const u32*)d_weights, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
