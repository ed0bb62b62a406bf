// The lookup argument of the PLONK prover: logUp in its univariate running-sum form over one
// table of three-column tuples.  A section of the plonk.hip unit, which alone includes it, after plonk.cuh: it uses that
// file's scalars in kernel arguments and vanilla terms of the quotient, the element I/O of fr_tables.cuh and the staged
// tile, scan, chunked inversion and entry checks of fr_rows.cuh.  Values in HBM are 32 bytes LE, plain; inputs are taken mod r, outputs are canonical.
//
// Index.  An open-addressing table of uint32 row numbers over the first n_rows table rows, capacity the power of two
// >= 2 n_rows, empty = 0xffffffff.  The key is the 24 words of the canonical tuple.  A row claims an empty slot with a
// compare-and-swap; a row that meets a slot whose row holds an equal tuple lowers it with atomicMin and stops.  Slots
// never empty again and equal tuples walk the same slots, so a tuple owns one slot, which ends on its lowest row
// number whatever the order of arrival.
//   bytes per row: 96 read + a probe (4 B and, on a collision, 96 B of the resident's tuple).
//
// Counts.  m is zeroed; a row with qK != 0 probes with its canonical tuple (a probe ends at an empty slot: load <= 1/2)
// and adds 1 to word 0 of m[row] on a hit; the lanes of a wave that hit one row send one add.  A miss is counted and
// the lowest missing row kept.  Integer atomics only: bitwise reproducible.
//   bytes per row: 128 read (32 with qK = 0) + a probe (4 + 96 B per slot visited).
//
// Sum.  S_0 = 0, S_{i+1} = S_i + m_i / (theta + t_i) - qK_i / (theta + f_i), f = a + eta b + eta^2 c, t likewise over
// the table.  The three phases of the grand product: a workgroup of PLONK_WG lanes stages two of the eight rows at a
// time, a lane owns PLONK_L consecutive rows; a row's two fractions go over the common denominator
// (theta + t)(theta + f), so a lane inverts PLONK_L values with one safegcd inversion.  A zero denominator is counted,
// its fraction is 0 (its factor in the common denominator is replaced by 1) and the other fraction stays exact.
//   products per row and pass: 4 (f, t) + 2 under one reduction (numerator) + 1 (denominator) + 3 (chunk inverse)
//   + 1 (term) = 11, + 1 to leave Montgomery form in the tile pass, + an inversion per KZG_INV_BATCH rows;
//   bytes per row: 8 x 32 read in each of the two passes, 32 written.
//
// Quotient.  One point per lane: the vanilla terms of plonk.cuh plus alpha^3 L1 + alpha^4 L2,
//   L1 = (S(omega X) - S)(theta + t)(theta + f) - m (theta + f) + qK (theta + t),   L2 = S L_1.
//   products per point: the vanilla 26 + 3 (t) + 2 (f) + 4 (L1) + 1 (L2) + 2 (the weights) = 38, pairs of them under
//   one reduction; bytes: 23 x 32 read (S and Z twice) + 32 written.
#pragma once
#include "plonk.cuh"

namespace ozk {

constexpr u32 LOOKUP_EMPTY = 0xffffffffu;
constexpr int LOOKUP_WG = 256;
constexpr int LOOKUP_MAX_ROWS = 1 << 28;

#if defined(__HIPCC__)
// the canonical words of one element
__device__ __forceinline__ void lookup_canon(const u32* __restrict__ p, u32 (&o)[8]) { pack(canonical(fr_load<85>(p)), o); }
// the canonical tuple of row i of three rows at stride cs (in words)
__device__ __forceinline__ void lookup_tuple(const u32* __restrict__ rows, size_t cs, unsigned i, u32 (&o)[24]) {
#pragma unroll
  for (int j = 0; j < 3; j++) {
    u32 w[8];
    lookup_canon(rows + (size_t)j * cs + (size_t)i * 8, w);
#pragma unroll
    for (int k = 0; k < 8; k++) o[8 * j + k] = w[k];
  }
}
__device__ __forceinline__ bool lookup_equal(const u32 (&x)[24], const u32 (&y)[24]) {
  u32 d = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) d |= x[k] ^ y[k];
  return d == 0;
}
// every word moves every bit of the state (multiply, rotate, multiply: the round of MurmurHash3)
__device__ __forceinline__ u32 lookup_hash(const u32 (&x)[24]) {
  u32 h = 0x9747b28cu;
#pragma unroll
  for (int k = 0; k < 24; k++) {
    u32 w = x[k] * 0xcc9e2d51u;
    w = (w << 15) | (w >> 17);
    h ^= w * 0x1b873593u;
    h = (h << 13) | (h >> 19);
    h = h * 5u + 0xe6546b64u;
  }
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

__global__ void __launch_bounds__(LOOKUP_WG) k_plonk_lookup_index(const u32* __restrict__ table, size_t cs, unsigned n_rows,
                                                                  u32* index, u32 mask) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  u32 mine[24];
  lookup_tuple(table, cs, i, mine);
  u32 slot = lookup_hash(mine) & mask;
  // at most capacity steps: n_rows <= capacity / 2 rows are ever inserted
  for (u32 step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
    const u32 cur = atomicCAS(index + slot, LOOKUP_EMPTY, i);
    if (cur == LOOKUP_EMPTY) return;
    if (cur >= n_rows) continue;   // (never written by this kernel)
    u32 theirs[24];
    lookup_tuple(table, cs, cur, theirs);
    if (lookup_equal(mine, theirs)) {
      atomicMin(index + slot, i);
      return;
    }
  }
}

// m[row] += 1 for every row i < len with qK_i != 0 whose tuple is table row `row`; the index is read-only here
__global__ void __launch_bounds__(LOOKUP_WG) k_plonk_lookup_counts(const u32* __restrict__ wires, const u32* __restrict__ qk,
                                                                   unsigned len, size_t cs, const u32* __restrict__ table,
                                                                   size_t tcs, unsigned n_rows, const u32* __restrict__ index,
                                                                   u32 mask, u32* m, int* missing, int* first_missing) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = false, miss = false;
  u32 row = 0;
  if (i < len) {
    u32 sel[8];
    lookup_canon(qk + (size_t)i * 8, sel);
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) any |= sel[k];
    if (any) {
      u32 mine[24];
      lookup_tuple(wires, cs, i, mine);
      u32 slot = lookup_hash(mine) & mask;
      miss = true;
      for (u32 step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
        const u32 cur = index[slot];
        if (cur >= n_rows) break;   // an empty slot (or no row of this table): the tuple is absent
        u32 theirs[24];
        lookup_tuple(table, tcs, cur, theirs);
        if (lookup_equal(mine, theirs)) {
          hit = true;
          miss = false;
          row = cur;
          break;
        }
      }
    }
  }
  // the lanes of the wave that hit one row send one add between them
  const unsigned lane = __lane_id();
  bool pending = hit;
  for (;;) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const u32 lead_row = (u32)__shfl((int)row, leader);
    const bool same = pending && row == lead_row;
    const unsigned long long group = __ballot(same);
    if (lane == (unsigned)leader) atomicAdd(m + (size_t)row * 8, (u32)__popcll(group));
    if (same) pending = false;
  }
  const unsigned long long missed = __ballot(miss);
  if (missed && lane == (unsigned)(__ffsll((long long)missed) - 1)) {
    atomicAdd(missing, __popcll(missed));
    atomicMin(first_missing, (int)i);   // the lowest lane of the wave holds its lowest row
  }
}

// ---- the running sum
struct PlonkLookupSumArgs {
  FrArg eta, eta2;   // Montgomery form
  FrArg theta;       // plain
};

// Two rows staged side by side; the caller reads both tiles and calls block_sync() before the next pair.
__device__ __forceinline__ void lookup_stage(const u32* __restrict__ x_row, const u32* __restrict__ y_row, int len, int t,
                                             u32* tile_x, u32* tile_y) {
  fr_tile_fill<PLONK_WG, PLONK_L>(x_row, len, t, tile_x);
  fr_tile_fill<PLONK_WG, PLONK_L>(y_row, len, t, tile_y);
  block_sync();
}
// f[k] = m / (theta + t) - qK / (theta + f), Montgomery form, for the lane's rows t PLONK_TILE + PLONK_L threadIdx.x + k
// (0 for a row beyond len); returns how many of its denominators are zero.  key4: the rows qK, T1, T2, T3.  Both
// tiles are free on return.
//   With plain operands N = (m (theta + f) - qK (theta + t)) / R and D = (theta + t)(theta + f) / R; the inverse of D
//   read as a Montgomery form is R^3 / ((theta + t)(theta + f)), and N (R^3 / ..) / R is the term times R.
__device__ __forceinline__ int plonk_lookup_terms(const u32* __restrict__ wires, size_t cs, const u32* __restrict__ key4,
                                                  size_t kcs, const u32* __restrict__ m, int len, int t,
                                                  const PlonkLookupSumArgs& a, u32* tile_x, u32* tile_y, KzgV (&f)[PLONK_L]) {
  const int l = threadIdx.x;
  const auto eta = plonk_arg(a.eta), eta2 = plonk_arg(a.eta2), theta = plonk_arg(a.theta);
  KzgV dt[PLONK_L], mm[PLONK_L], d[PLONK_L];
  lookup_stage(key4 + kcs, key4 + 2 * kcs, len, t, tile_x, tile_y);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    const int e = l * PLONK_L + k;
    dt[k] = KzgV(reduce_to<32>(add(add(fr_tile_get(tile_x, e), theta), mul(fr_tile_get(tile_y, e), eta))));
  }
  block_sync();
  lookup_stage(key4 + 3 * kcs, m, len, t, tile_x, tile_y);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    const int e = l * PLONK_L + k;
    dt[k] = KzgV(reduce_to<32>(add(dt[k], mul(fr_tile_get(tile_x, e), eta2))));
    mm[k] = KzgV(fr_tile_get(tile_y, e));
  }
  block_sync();
  lookup_stage(wires, wires + cs, len, t, tile_x, tile_y);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    const int e = l * PLONK_L + k;
    d[k] = KzgV(reduce_to<32>(add(add(fr_tile_get(tile_x, e), theta), mul(fr_tile_get(tile_y, e), eta))));
  }
  block_sync();
  lookup_stage(wires + 2 * cs, key4, len, t, tile_x, tile_y);
  int zeros = 0;
  Fe<FrP, 1> one = fe_zero<FrP>();
  one.l[0] = 1;
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    const int e = l * PLONK_L + k;
    const KzgV df = KzgV(reduce_to<32>(add(d[k], mul(fr_tile_get(tile_x, e), eta2))));
    const KzgV qk = KzgV(fr_tile_get(tile_y, e));
    if ((long long)t * PLONK_TILE + e >= len) {
      f[k] = KzgV(fe_zero<FrP>());
      d[k] = KzgV(fe_one<FrP>());
      continue;
    }
    const bool zt = is_zero(dt[k]), zf = is_zero(df);
    zeros += (int)zt + (int)zf;
    const KzgV tt = zt ? KzgV(one) : dt[k], mv = zt ? KzgV(fe_zero<FrP>()) : mm[k];
    const KzgV ff = zf ? KzgV(one) : df, qv = zf ? KzgV(fe_zero<FrP>()) : qk;
    f[k] = KzgV(reduce_to<32>(mul2(mv, ff, neg(qv), tt)));
    d[k] = KzgV(reduce_to<32>(mul(tt, ff)));
  }
  block_sync();
  KzgV di[PLONK_L];
  kzg_chunk_inverses<PLONK_L>(d, PLONK_L, di);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) f[k] = KzgV(mul(f[k], di[k]));
  return zeros;
}
__device__ __forceinline__ KzgV plonk_lane_sum(const KzgV (&f)[PLONK_L]) {
  KzgV a = f[0];
#pragma unroll
  for (int k = 1; k < PLONK_L; k++) a = KzgV(reduce_to<32>(add(a, f[k])));
  return a;
}

// first pass (several tiles): the sum of tile t, Montgomery form, to agg[t]
__global__ void __launch_bounds__(PLONK_WG) k_plonk_lookup_sum_tiles(const u32* __restrict__ wires, size_t cs,
                                                                    const u32* __restrict__ key4, size_t kcs,
                                                                    const u32* __restrict__ m, int len, PlonkLookupSumArgs a,
                                                                    u32* __restrict__ agg) {
  __shared__ __attribute__((aligned(16))) u32 tile_x[KZG_TILE_WORDS];
  __shared__ __attribute__((aligned(16))) u32 tile_y[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  KzgV f[PLONK_L];
  plonk_lookup_terms(wires, cs, key4, kcs, m, len, blockIdx.x, a, tile_x, tile_y, f);
  const KzgV s = fr_wg_scan<PLONK_WG, false>(plonk_lane_sum(f), FrScanSum{}, part);
  if (threadIdx.x == PLONK_WG - 1) fr_store(canonical(s), agg + (size_t)blockIdx.x * 8);
}
// second pass, one workgroup: carry[t] = the sum of the tiles below t
__global__ void __launch_bounds__(PLONK_SCAN_WG) k_plonk_lookup_sum_carries(const u32* __restrict__ agg, int nt,
                                                                           u32* __restrict__ carry) {
  __shared__ u32 part[9 * PLONK_SCAN_WG];
  fr_carries_scan<PLONK_SCAN_WG, false>(agg, nt, FrScanSum{}, carry, part);
}
// the tile pass: S, the count of zero denominators and, from the last tile, the sum over all rows.  carry: null when
// the row is one tile.
__global__ void __launch_bounds__(PLONK_WG) k_plonk_lookup_sum_apply(const u32* __restrict__ wires, size_t cs,
                                                                    const u32* __restrict__ key4, size_t kcs,
                                                                    const u32* __restrict__ m, int len, int nt,
                                                                    PlonkLookupSumArgs a, const u32* __restrict__ carry,
                                                                    u32* __restrict__ s_out, u32* __restrict__ total,
                                                                    int* __restrict__ zero_dens) {
  __shared__ __attribute__((aligned(16))) u32 tile_x[KZG_TILE_WORDS];
  __shared__ __attribute__((aligned(16))) u32 tile_y[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  const int t = blockIdx.x, l = threadIdx.x;
  KzgV f[PLONK_L];
  const int zeros = plonk_lookup_terms(wires, cs, key4, kcs, m, len, t, a, tile_x, tile_y, f);
  if (zeros) atomicAdd(zero_dens, zeros);
  KzgV below = KzgV(fe_zero<FrP>());
  if (carry) below = KzgV(fr_load<16>(carry + (size_t)t * 8));
  KzgV sum = plonk_lane_sum(f);
  if (l == 0) sum = KzgV(reduce_to<32>(add(sum, below)));
  const KzgV s = fr_wg_scan<PLONK_WG, false>(sum, FrScanSum{}, part);
  if (t == nt - 1 && l == PLONK_WG - 1) {
    u32 o[8];
    from_mont(s, o);
    fr_store_words(o, total);
  }
  // the sum below the lane's first row; every S leaves Montgomery form on its way into the tile
  Fe<FrP, 1> one = fe_zero<FrP>();
  one.l[0] = 1;
  KzgV run = fr_scan_neighbour<PLONK_WG, false>(part, below);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    fr_tile_put(tile_x, l * PLONK_L + k, canonical(mul(run, one)));
    if (k + 1 < PLONK_L) run = KzgV(reduce_to<32>(add(run, f[k])));
  }
  block_sync();
  fr_tile_store<PLONK_WG, PLONK_L>(tile_x, t, len, 0, nullptr, 0, s_out);
}

// ---- the quotient with the two lookup terms
struct PlonkLookupQuotArgs {
  FrArg alpha3_r, alpha4_r2;              // alpha^3 R, alpha^4 R^2
  FrArg eta_r, eta2_r, eta_r2, eta2_r2;   // eta R, eta^2 R, eta R^2, eta^2 R^2
  FrArg theta_r;                          // theta R
};
enum { PLONK_LK_M = PLONK_WIT_ROWS, PLONK_LK_S, PLONK_LK_WIT_ROWS };
enum { PLONK_LK_QK = PLONK_KEY_ROWS, PLONK_LK_T1, PLONK_LK_T2, PLONK_LK_T3, PLONK_LK_KEY_ROWS };

// theta + f and theta + t are built in Montgomery form (a, b, c arrive so; the table's values are plain and meet
// eta R^2), so that every product with the plain S, m, qK below is plain, as the vanilla terms are.
__global__ void __launch_bounds__(256) k_plonk_quotient_lookup(const u32* __restrict__ wit, size_t wit_cs,
                                                               const u32* __restrict__ key, size_t key_cs, unsigned n4,
                                                               PlonkQuotArgs q, PlonkLookupQuotArgs lk, u32* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  KzgV a, b, c;
  const auto vanilla = plonk_vanilla_terms(wit, wit_cs, key, key_cs, n4, i, q, a, b, c);
  const auto r2 = fe_const<FrP, 16>(FrP::R2);
  const auto theta_r = plonk_arg(lk.theta_r);
  const KzgV df = KzgV(reduce_to<32>(add(add(a, theta_r), mul2(b, plonk_arg(lk.eta_r), c, plonk_arg(lk.eta2_r)))));
  const KzgV dt = KzgV(reduce_to<32>(
      add(add(mul(plonk_in(key, key_cs, PLONK_LK_T1, i), r2), theta_r),
          mul2(plonk_in(key, key_cs, PLONK_LK_T2, i), plonk_arg(lk.eta_r2), plonk_in(key, key_cs, PLONK_LK_T3, i),
               plonk_arg(lk.eta2_r2)))));
  const KzgV s = plonk_in(wit, wit_cs, PLONK_LK_S, i);
  const KzgV sw = plonk_in(wit, wit_cs, PLONK_LK_S, (i + 4) & (n4 - 1));
  const KzgV m = plonk_in(wit, wit_cs, PLONK_LK_M, i);
  const KzgV qk = plonk_in(key, key_cs, PLONK_LK_QK, i);
  // L1 = (S(omega X) - S)(theta + t)(theta + f) + qK (theta + t) - m (theta + f)
  const KzgV l1 = KzgV(reduce_to<32>(add(mul(mul(sub(sw, s), dt), df), mul2(qk, dt, neg(m), df))));
  // L2 = S L_1, with 1 / R
  const auto l2 = mul(s, plonk_in(key, key_cs, PLONK_L1, i));
  const auto sum = add(vanilla, mul2(l1, plonk_arg(lk.alpha3_r), l2, plonk_arg(lk.alpha4_r2)));
  fr_store(canonical(mul(sum, plonk_arg(q.zh_r[i & 3]))), out + (size_t)i * 8);
}

// ---- host side ----
static u32 lookup_capacity(int n_rows) {
  u32 cap = 2;
  while (cap < 2u * (u32)n_rows) cap <<= 1;
  return cap;
}
static bool lookup_rows_ok(int n_rows) { return n_rows >= 1 && n_rows <= LOOKUP_MAX_ROWS; }
struct PlonkLookupSumLayout {
  u32 *agg, *carry;
  int nt;
  size_t bytes;
};
static PlonkLookupSumLayout plonk_lookup_sum_layout(int len, void* wsp) {
  PlonkLookupSumLayout L;
  Bump b(wsp, ~(size_t)0);
  L.nt = (len + PLONK_TILE - 1) / PLONK_TILE;
  const size_t per = L.nt > 1 ? (size_t)L.nt * 8 : 0;
  L.agg = b.take<u32>(per);
  L.carry = b.take<u32>(per);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static bool lookup_misaligned4(const void* p) { return ((uintptr_t)p & 3) != 0; }
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

size_t ozk_plonk_lookup_index_bytes(int32_t n_rows) {
  if (!lookup_rows_ok(n_rows)) return 0;
  return (size_t)lookup_capacity(n_rows) * 4;
}

int ozk_plonk_lookup_index_dev(const void* d_table, int32_t n_rows, int64_t table_stride, void* d_index, size_t index_bytes,
                               void* stream) {
  hip_clear_stale();
  if (!lookup_rows_ok(n_rows)) return fail(OZK_E_INVALID, "bad shape: %d table rows (1 <= n_rows <= 2^28)", n_rows);
  if (table_stride < n_rows) return fail(OZK_E_INVALID, "bad stride: table_stride %lld (>= n_rows %d)", (long long)table_stride, n_rows);
  if (int rc = fr_check_pointers(d_table, d_index)) return rc;
  if (int rc = fr_check_aligned16(d_table, d_index)) return rc;
  const u32 cap = lookup_capacity(n_rows);
  if (index_bytes < (size_t)cap * 4)
    return fail(OZK_E_INVALID, "index too small: need %zu bytes, got %zu", (size_t)cap * 4, index_bytes);
  if (kzg_overlap(d_table, kzg_span(3, n_rows, table_stride), d_index, (size_t)cap * 4))
    return fail(OZK_E_INVALID, "d_index overlaps d_table");
  hipStream_t st = (hipStream_t)stream;
  OZK_HIP(hipMemsetAsync(d_index, 0xff, (size_t)cap * 4, st));
  hipLaunchKernelGGL(k_plonk_lookup_index, dim3((n_rows + LOOKUP_WG - 1) / LOOKUP_WG), dim3(LOOKUP_WG), 0, st,
                     (const u32*)d_table, (size_t)table_stride * 8, (unsigned)n_rows, (u32*)d_index, cap - 1);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_plonk_lookup_counts_dev(const void* d_wires, const void* d_qk, int32_t len, int64_t stride, const void* d_table,
                                int32_t n_rows, int64_t table_stride, const void* d_index, size_t index_bytes, void* d_m,
                                int32_t m_len, int32_t* d_missing, int32_t* d_first_missing, void* stream) {
  hip_clear_stale();
  if (len < 1 || (long long)len > KZG_MAX_ELEMS) return fail(OZK_E_INVALID, "bad shape: %d rows (1 <= len <= 2^28)", len);
  if (!lookup_rows_ok(n_rows) || m_len < n_rows || (long long)m_len > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad shape: %d table rows, m of %d elements (1 <= n_rows <= m_len <= 2^28)", n_rows, m_len);
  if (stride < len || table_stride < n_rows)
    return fail(OZK_E_INVALID, "bad strides: stride %lld (>= len %d), table_stride %lld (>= n_rows %d)", (long long)stride,
                len, (long long)table_stride, n_rows);
  if (int rc = fr_check_pointers(d_wires, d_qk, d_table, d_index, d_m, d_missing, d_first_missing)) return rc;
  if (int rc = fr_check_aligned16(d_wires, d_qk, d_table, d_index, d_m)) return rc;
  if (lookup_misaligned4(d_missing) || lookup_misaligned4(d_first_missing))
    return fail(OZK_E_INVALID, "d_missing and d_first_missing must be 4-byte aligned");
  const u32 cap = lookup_capacity(n_rows);
  if (index_bytes < (size_t)cap * 4)
    return fail(OZK_E_INVALID, "index too small: need %zu bytes, got %zu", (size_t)cap * 4, index_bytes);
  const size_t m_bytes = (size_t)m_len * 32;
  const struct { const void* p; size_t n; } in[4] = {{d_wires, kzg_span(3, len, stride)}, {d_qk, (size_t)len * 32},
                                                    {d_table, kzg_span(3, n_rows, table_stride)}, {d_index, (size_t)cap * 4}};
  for (const auto& r : in)
    if (kzg_overlap(r.p, r.n, d_m, m_bytes) || kzg_overlap(r.p, r.n, d_missing, 4) || kzg_overlap(r.p, r.n, d_first_missing, 4))
      return fail(OZK_E_INVALID, "an output overlaps d_wires, d_qk, d_table or d_index");
  if (kzg_overlap(d_m, m_bytes, d_missing, 4) || kzg_overlap(d_m, m_bytes, d_first_missing, 4) ||
      kzg_overlap(d_missing, 4, d_first_missing, 4))
    return fail(OZK_E_INVALID, "d_m, d_missing and d_first_missing overlap one another");
  hipStream_t st = (hipStream_t)stream;
  OZK_HIP(hipMemsetAsync(d_m, 0, m_bytes, st));
  OZK_HIP(hipMemsetAsync(d_missing, 0, 4, st));
  OZK_HIP(hipMemsetD32Async((hipDeviceptr_t)d_first_missing, 0x7fffffff, 1, st));
  hipLaunchKernelGGL(k_plonk_lookup_counts, dim3((len + LOOKUP_WG - 1) / LOOKUP_WG), dim3(LOOKUP_WG), 0, st,
                     (const u32*)d_wires, (const u32*)d_qk, (unsigned)len, (size_t)stride * 8, (const u32*)d_table,
                     (size_t)table_stride * 8, (unsigned)n_rows, (const u32*)d_index, cap - 1, (u32*)d_m, (int*)d_missing,
                     (int*)d_first_missing);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_plonk_lookup_sum_workspace_bytes(int32_t len) {
  if (!plonk_perm_shape_ok(len)) return 0;
  return plonk_lookup_sum_layout(len, nullptr).bytes;
}

int ozk_plonk_lookup_sum_dev(const void* d_wires, int64_t stride, const void* d_key4, int64_t key_stride, const void* d_m,
                             int32_t len, const uint8_t* eta_host32, const uint8_t* theta_host32, void* d_s, void* d_total,
                             int32_t* d_zero_dens, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!plonk_perm_shape_ok(len)) return fail(OZK_E_INVALID, "bad shape: %d rows (1 <= len <= 2^28)", len);
  if (stride < len || key_stride < len)
    return fail(OZK_E_INVALID, "bad strides: stride %lld, key_stride %lld (both >= len %d)", (long long)stride,
                (long long)key_stride, len);
  if (int rc = fr_check_pointers(d_wires, d_key4, d_m, eta_host32, theta_host32, d_s, d_total, d_zero_dens, d_workspace))
    return rc;
  if (int rc = fr_check_aligned16(d_wires, d_key4, d_m, d_s, d_total)) return rc;
  if (lookup_misaligned4(d_zero_dens)) return fail(OZK_E_INVALID, "d_zero_dens must be 4-byte aligned");
  const size_t row = (size_t)len * 32;
  const struct { const void* p; size_t n; } in[3] = {{d_wires, kzg_span(3, len, stride)}, {d_key4, kzg_span(4, len, key_stride)},
                                                    {d_m, row}};
  for (const auto& r : in)
    if (kzg_overlap(r.p, r.n, d_s, row) || kzg_overlap(r.p, r.n, d_total, 32) || kzg_overlap(r.p, r.n, d_zero_dens, 4))
      return fail(OZK_E_INVALID, "an output overlaps d_wires, d_key4 or d_m");
  if (kzg_overlap(d_s, row, d_total, 32) || kzg_overlap(d_s, row, d_zero_dens, 4) || kzg_overlap(d_total, 32, d_zero_dens, 4))
    return fail(OZK_E_INVALID, "d_s, d_total and d_zero_dens overlap one another");
  const PlonkLookupSumLayout L = plonk_lookup_sum_layout(len, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  // the first two kernels write the workspace and the third reads it
  for (const auto& r : in)
    if (kzg_overlap(r.p, r.n, d_workspace, L.bytes)) return fail(OZK_E_INVALID, "d_workspace overlaps d_wires, d_key4 or d_m");
  if (kzg_overlap(d_s, row, d_workspace, L.bytes) || kzg_overlap(d_total, 32, d_workspace, L.bytes) ||
      kzg_overlap(d_zero_dens, 4, d_workspace, L.bytes))
    return fail(OZK_E_INVALID, "d_workspace overlaps d_s, d_total or d_zero_dens");
  hipStream_t st = (hipStream_t)stream;
  PlonkLookupSumArgs a;
  const auto eta = plonk_mont(eta_host32);
  a.eta = plonk_words(eta);
  a.eta2 = plonk_words(sqr(eta));
  a.theta = plonk_plain(theta_host32);
  const u32 *w = (const u32*)d_wires, *k4 = (const u32*)d_key4, *m = (const u32*)d_m;
  const size_t cs = (size_t)stride * 8, kcs = (size_t)key_stride * 8;
  OZK_HIP(hipMemsetAsync(d_zero_dens, 0, 4, st));
  if (L.nt > 1) {
    hipLaunchKernelGGL(k_plonk_lookup_sum_tiles, dim3(L.nt), dim3(PLONK_WG), 0, st, w, cs, k4, kcs, m, len, a, L.agg);
    hipLaunchKernelGGL(k_plonk_lookup_sum_carries, dim3(1), dim3(PLONK_SCAN_WG), 0, st, (const u32*)L.agg, L.nt, L.carry);
  }
  hipLaunchKernelGGL(k_plonk_lookup_sum_apply, dim3(L.nt), dim3(PLONK_WG), 0, st, w, cs, k4, kcs, m, len, L.nt, a,
                     (const u32*)(L.nt > 1 ? L.carry : nullptr), (u32*)d_s, (u32*)d_total, (int*)d_zero_dens);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_plonk_quotient_lookup_dev(const void* d_wit, int64_t wit_stride, const void* d_key, int64_t key_stride, int32_t n,
                                  const uint8_t* alpha_host32, const uint8_t* beta_host32, const uint8_t* gamma_host32,
                                  const uint8_t* k_host96, const uint8_t* zh_inv_host128, const uint8_t* eta_host32,
                                  const uint8_t* theta_host32, void* d_out, void* stream) {
  hip_clear_stale();
  if (int rc = plonk_quot_shape(n, wit_stride, key_stride)) return rc;
  if (int rc = fr_check_pointers(d_wit, d_key, alpha_host32, beta_host32, gamma_host32, k_host96, zh_inv_host128, eta_host32,
                                 theta_host32, d_out))
    return rc;
  if (int rc = plonk_quot_buffers(d_wit, PLONK_LK_WIT_ROWS, wit_stride, d_key, PLONK_LK_KEY_ROWS, key_stride, n, d_out))
    return rc;
  const int n4 = 4 * n;
  const PlonkQuotArgs q = plonk_quot_args(alpha_host32, beta_host32, gamma_host32, k_host96, zh_inv_host128);
  PlonkLookupQuotArgs lk;
  const auto r2 = fe_const<FrP, 16>(FrP::R2);
  const auto alpha = plonk_mont(alpha_host32), eta = plonk_mont(eta_host32);
  const auto alpha2 = sqr(alpha), eta2 = sqr(eta);
  lk.alpha3_r = plonk_words(mul(alpha2, alpha));
  lk.alpha4_r2 = plonk_words(mul(sqr(alpha2), r2));
  lk.eta_r = plonk_words(eta);
  lk.eta2_r = plonk_words(eta2);
  lk.eta_r2 = plonk_words(mul(eta, r2));
  lk.eta2_r2 = plonk_words(mul(eta2, r2));
  lk.theta_r = plonk_words(plonk_mont(theta_host32));
  hipLaunchKernelGGL(k_plonk_quotient_lookup, dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const u32*)d_wit,
                     (size_t)wit_stride * 8, (const u32*)d_key, (size_t)key_stride * 8, (unsigned)n4, q, lk, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
