// What the Fr kernels that walk rows of 32-byte elements share: kzg.cuh, kzg_set.cuh,
// kzg_multi.cuh (the kzg.hip unit) and plonk.cuh, plonk_lookup.cuh, plonk_r1cs.cuh (the plonk.hip unit) build on it.
// Stands alone.  The per-lane pieces compile for the host too (tests/native/kzg_hostcheck.cpp, kzg_set_hostcheck.cpp); the device
// parts use the element I/O of fr_tables.cuh and the barrier of curve.cuh, included below for the device compiler.
//
//   - the per-lane pieces: Horner's recurrence over a piece, the composition of carries, the chunk inversion;
//   - a row's constants (KzgRow, KzgSetPows) and its value from tile 0 and the tail above it;
//   - the staged tile: KZG_TILE elements of a row in LDS, filled and stored coalesced, read and written per lane;
//   - the workgroup scan over lanes, in either direction, for any combining operation, and the scan of per-tile
//     aggregates by one workgroup that is built on it;
//   - the checks every entry point makes on the host.
#pragma once
#include "fp29.cuh"
#if defined(__HIPCC__)
#include "fr_tables.cuh"
#endif

namespace ozk {

using FrP = FrParams;

constexpr int KZG_WG = 256;                    // lanes of a workgroup
constexpr int KZG_L = 4;                       // consecutive coefficients of a lane
constexpr int KZG_TILE = KZG_WG * KZG_L;       // coefficients of a workgroup: 33 KiB of LDS + 9 KiB of scan
constexpr int KZG_INV_BATCH = 8;               // differences sharing one inversion
using KzgV = Fe<FrP, 32>;

// ---- the per-lane pieces ----
// h_i = p_i + z h_{i+1} for i = n - 1 .. 0 with h_n = carry; returns h_0.  p, carry, h: plain; z: Montgomery form.
// n <= N, the length the loop is unrolled for (a kernel's lanes run n = N, so that p and h stay in registers).
// KEEP: the h_i are written to h, which may be p itself when E is KzgV (p_i is read before h_i is written); else h is
// not touched (the value alone).
template <int N, bool KEEP, class E>
OZK_HD KzgV kzg_piece(const E* p, int n, const Fe<FrP, 16>& z, const KzgV& carry, KzgV* h) {
  KzgV c = carry;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int i = N - 1 - k;
    if (i < n) {
      c = KzgV(reduce_to<32>(add(p[i], mul(z, c))));
      if (KEEP) h[i] = c;
    }
  }
  return c;
}
// a + m s: the value of a piece followed by what lies above it (m = z^(length of the piece), Montgomery form)
OZK_HD KzgV kzg_compose(const KzgV& a, const KzgV& m, const KzgV& s) {
  return KzgV(reduce_to<32>(add(a, mul(m, s))));
}
// out_k = 1 / d_k for k < n <= BATCH (Montgomery form in and out), 0 for d_k = 0: one inversion for the chunk
template <int BATCH>
OZK_HD void kzg_chunk_inverses(const KzgV* d, int n, KzgV* out) {
  KzgV prefix[BATCH];
  KzgV run = KzgV(fe_one<FrP>());
#pragma unroll
  for (int k = 0; k < BATCH; k++) {
    if (k < n && !is_zero(d[k])) run = KzgV(mul(run, d[k]));
    prefix[k] = run;
  }
  KzgV invrun = inv(run);
#pragma unroll
  for (int k = BATCH - 1; k >= 0; k--) {
    if (k >= n) continue;
    if (is_zero(d[k])) {
      out[k] = KzgV(fe_zero<FrP>());
      continue;
    }
    out[k] = k > 0 ? KzgV(mul(invrun, prefix[k - 1])) : invrun;
    invrun = KzgV(mul(invrun, d[k]));
  }
}

#if defined(__HIPCC__)
// ---- a row's constants ----
constexpr int KZG_SCAN_STEPS = 8;   // log2 KZG_WG
static_assert(1 << KZG_SCAN_STEPS == KZG_WG, "one multiplier per step of the scan");
struct KzgRow {        // per row, Montgomery form, canonical
  u32 z[8], zl[8], zt[8];   // z, z^KZG_L, z^KZG_TILE
};
struct KzgSetPows {   // z^(KZG_L 2^d), d < KZG_SCAN_STEPS: the scan's multipliers; Montgomery form, canonical
  u32 m[KZG_SCAN_STEPS][8];
};
// the constants of the row with point z and, where `pows` is given, the multipliers of its scan
__device__ __forceinline__ void kzg_row_consts(const Fe<FrP, 17>& z, KzgRow* row, KzgSetPows* pows) {
  using E16 = ElemTraits<Fe<FrP, 16>>;
  E16::store(canonical(z), row->z);
  KzgV m = fe_pow_u32(z, KZG_L);
  E16::store(canonical(m), row->zl);
#pragma unroll 1
  for (int d = 0; d < KZG_SCAN_STEPS; d++) {
    if (pows) E16::store(canonical(m), pows->m[d]);
    m = KzgV(sqr(m));
  }
  E16::store(canonical(m), row->zt);
}
// p(z) = (the value of tile 0) + z^KZG_TILE (the tail above it)
__device__ __forceinline__ void kzg_row_value(const u32* __restrict__ agg0, const u32* __restrict__ tail0, const KzgRow& row,
                                              u32* __restrict__ value) {
  fr_store(canonical(kzg_compose(KzgV(fr_load<16>(agg0)), KzgV(ElemTraits<Fe<FrP, 16>>::load(row.zt)),
                                 KzgV(fr_load<16>(tail0)))),
           value);
}

// ---- the staged tile ----
// element e of a staged tile, word w: word-major, a pad word every 32 elements, so that the lanes of a wave hit
// distinct banks both when they touch consecutive elements and when they touch elements KZG_L apart
constexpr int KZG_TILE_PAD = KZG_TILE + KZG_TILE / 32;
constexpr int KZG_TILE_WORDS = 8 * KZG_TILE_PAD;
__device__ __forceinline__ int kzg_at(int e, int w) { return w * KZG_TILE_PAD + e + (e >> 5); }

// Tile t of a row (canonical; zero beyond len) into LDS, coalesced: WG lanes, L elements a lane, WG apart.  The
// caller's barrier follows.
template <int WG, int L>
__device__ __forceinline__ void fr_tile_fill(const u32* __restrict__ row, int len, int t, u32* tile) {
  static_assert(WG * L == KZG_TILE, "the staged tile has one shape in LDS");
#pragma unroll
  for (int i = 0; i < L; i++) {
    const int e = i * WG + threadIdx.x;
    const long long j = (long long)t * KZG_TILE + e;
    u32 o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j < len) pack(canonical(fr_load<85>(row + (size_t)j * 8)), o);
#pragma unroll
    for (int w = 0; w < 8; w++) tile[kzg_at(e, w)] = o[w];
  }
}
__device__ __forceinline__ Fe<FrP, 16> fr_tile_get(const u32* tile, int e) {
  u32 o[8];
#pragma unroll
  for (int w = 0; w < 8; w++) o[w] = tile[kzg_at(e, w)];
  return unpack<FrP, 16>(o);
}
__device__ __forceinline__ void fr_tile_put(u32* tile, int e, const Fe<FrP, 16>& v) {
  u32 o[8];
  pack(v, o);
#pragma unroll
  for (int w = 0; w < 8; w++) tile[kzg_at(e, w)] = o[w];
}
// The staged tile t out to a row, coalesced.  With j = t KZG_TILE + e the place of element e in the row it was filled
// from, index j - down of `row` receives element e + up of the tile, or `top` where that lies past the tile's end, for
// every down <= j < len.  (up = 0: `top` is not read.)
template <int WG, int L>
__device__ __forceinline__ void fr_tile_store(const u32* tile, int t, int len, int up, const u32* top, int down,
                                              u32* __restrict__ row) {
#pragma unroll
  for (int i = 0; i < L; i++) {
    const int e = i * WG + threadIdx.x;
    const long long j = (long long)t * KZG_TILE + e;
    if (j >= len || (down > 0 && j < down)) continue;   // (a literal down = 0 leaves no test: j >= 0 is not known)
    u32 o[8];
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = e + up < KZG_TILE ? tile[kzg_at(e + up, w)] : top[w];
    fr_store_words(o, row + (size_t)(j - down) * 8);
  }
}

// ---- the workgroup scan ----
// An inclusive Hillis-Steele scan over the WG lanes of the workgroup: log2 WG steps, one `apply` each.  UP: lane l
// gathers the lanes above it, S_l = a_l o S_{l+1}; else those below it, S_l = S_{l-1} o a_l.  Op has
//   static KzgV neutral()                                what a lane with no neighbour combines with
//   KzgV apply(const KzgV& a, const KzgV& s, int step)   a combined with s, which lies 2^step lanes away
// and is taken by value: an operation may move its own state from step to step.  Returns the lane's S_l and leaves
// every S in `part` (limb-major, 9 x WG words) behind a barrier.
template <int WG, bool UP, class Op>
__device__ __forceinline__ KzgV fr_wg_scan(KzgV a, Op op, u32* part) {
  const int l = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 9; i++) part[i * WG + l] = a.l[i];
  block_sync();
#pragma unroll 1
  for (int step = 0; (1 << step) < WG; step++) {
    const int from = UP ? l + (1 << step) : l - (1 << step);
    KzgV s = Op::neutral();
    if (UP ? from < WG : from >= 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) s.l[i] = part[i * WG + from];
    }
    block_sync();
    a = op.apply(a, s, step);
#pragma unroll
    for (int i = 0; i < 9; i++) part[i * WG + l] = a.l[i];
    block_sync();
  }
  return a;
}
// the lane's neighbour after the scan: S_{l+1} (UP) or S_{l-1}, or `outside` (what lies beyond the workgroup) for
// the lane at the edge
template <int WG, bool UP>
__device__ __forceinline__ KzgV fr_scan_neighbour(const u32* part, const KzgV& outside) {
  const int from = UP ? (int)threadIdx.x + 1 : (int)threadIdx.x - 1;
  KzgV s = outside;
  if (UP ? from < WG : from >= 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) s.l[i] = part[i * WG + from];
  }
  return s;
}
// S_l = a_l + m S_{l+1}, m in Montgomery form and squared from step to step
struct FrScanAffine {
  KzgV m;
  __device__ __forceinline__ static KzgV neutral() { return KzgV(fe_zero<FrP>()); }
  __device__ __forceinline__ KzgV apply(const KzgV& a, const KzgV& s, int) {
    const KzgV r = kzg_compose(a, m, s);
    m = KzgV(sqr(m));
    return r;
  }
};
// S_l = a_0 a_1 .. a_l, Montgomery form
struct FrScanProduct {
  __device__ __forceinline__ static KzgV neutral() { return KzgV(fe_one<FrP>()); }
  __device__ __forceinline__ KzgV apply(const KzgV& a, const KzgV& s, int) const { return KzgV(mul(a, s)); }
};
// S_l = a_0 + a_1 + .. + a_l, in whichever form the a_l share
struct FrScanSum {
  __device__ __forceinline__ static KzgV neutral() { return KzgV(fe_zero<FrP>()); }
  __device__ __forceinline__ KzgV apply(const KzgV& a, const KzgV& s, int) const { return KzgV(reduce_to<32>(add(a, s))); }
};

// One workgroup scans the nt per-tile aggregates of a row, WG tiles at a time starting from the far end:
// carry[t] = what the tiles above t (UP) or below t combine to.  `op` is the operation between neighbouring tiles.
template <int WG, bool UP, class Op>
__device__ __forceinline__ void fr_carries_scan(const u32* __restrict__ agg, int nt, Op op, u32* __restrict__ carry, u32* part) {
  const int l = threadIdx.x, chunks = (nt + WG - 1) / WG;
  KzgV outside = Op::neutral();
  for (int c = 0; c < chunks; c++) {
    const int t = (UP ? chunks - 1 - c : c) * WG + l;
    KzgV a = Op::neutral();
    if (t < nt) a = KzgV(fr_load<16>(agg + (size_t)t * 8));
    if (l == (UP ? WG - 1 : 0)) a = Op(op).apply(a, outside, 0);
    fr_wg_scan<WG, UP>(a, op, part);
    const KzgV s = fr_scan_neighbour<WG, UP>(part, outside);
    if (t < nt) fr_store(canonical(s), carry + (size_t)t * 8);
#pragma unroll
    for (int i = 0; i < 9; i++) outside.l[i] = part[i * WG + (UP ? 0 : WG - 1)];
    block_sync();
  }
}

// ---- host side: the checks of the entry points ----
constexpr long long KZG_MAX_ELEMS = 1ll << 28;

static bool kzg_shape_ok(int npolys, int len) {
  return npolys >= 1 && len >= 1 && (long long)npolys * len <= KZG_MAX_ELEMS;
}
// rows of `len` elements, row y at base + 32 y stride bytes: the bytes they span
static size_t kzg_span(int npolys, int len, long long stride) {
  return ((size_t)(npolys - 1) * (size_t)stride + (size_t)len) * 32;
}
static bool kzg_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
static bool kzg_misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
// what every entry point words alike: its pointers, the alignment of its element buffers, its workspace
template <class... P>
static int fr_check_pointers(const P*... p) {
  if ((... || !p)) return fail(OZK_E_INVALID, "null pointer argument");
  return OZK_OK;
}
template <class... P>
static int fr_check_aligned16(const P*... p) {
  if ((... || kzg_misaligned16(p))) return fail(OZK_E_INVALID, "elements must be 16-byte aligned");
  return OZK_OK;
}
static int fr_check_workspace(size_t need, size_t got) {
  if (got < need) return fail(OZK_E_INVALID, "workspace too small: need %zu bytes, got %zu", need, got);
  return OZK_OK;
}
// x^n for the plain element x and a power of two n (Montgomery form)
static Fe<FrP, 32> fr_host_pow2(const uint8_t* x_host32, int n) {
  u32 w[8];
  memcpy(w, x_host32, 32);
  Fe<FrP, 32> x = Fe<FrP, 32>(to_mont<FrP>(w));
  for (int k = n; k > 1; k >>= 1) x = Fe<FrP, 32>(sqr(x));
  return x;
}
// omega has order exactly n (a power of two, >= 2) when omega^(n / 2) = -1
static bool fr_omega_has_order(const uint8_t* omega_host32, int n) {
  return is_zero(canonical(add(fr_host_pow2(omega_host32, n / 2), fe_one<FrP>())));
}
// z lies in the domain of n points (a power of two) when z^n = 1
static bool fr_in_domain(const uint8_t* z_host32, int n) {
  return is_zero(canonical(sub(fr_host_pow2(z_host32, n), fe_one<FrP>())));
}
#endif  // __HIPCC__

}  // namespace ozk
