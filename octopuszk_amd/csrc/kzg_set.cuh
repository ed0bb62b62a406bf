// The Fr kernels of KZG set openings: the quotient (p - I) / Z_S for S = (z_0 .. z_{t-1}),
// Z_S = prod (X - z_i) and I the interpolant of p on S, with the values p(z_i), in coefficient form and in evaluation
// form.  A section of the kzg.hip unit, which alone includes it for the device: kernels, layouts and entry points, after
// kzg.cuh, whose tile load and carries kernel it uses; it builds on the tiles, scan and chunk inversion of fr_rows.cuh.
// The per-lane pieces above the kernels compile for the host too (tests/native/kzg_set_hostcheck.cpp).
//
// Coefficient form.  Dividing by (X - z_0), .., (X - z_{t-1}) in turn is t runs of the recurrence of section 22,
// stage s over the output of stage s - 1: h^s_j = h^(s-1)_j + z_s h^s_(j+1), h^(-1) = p.  Position j holds h_j at
// every stage (the junk a stage leaves below position s never reaches a higher position) and q_(j-t) = h^(t-1)_j.
// What enters a stage at a tile boundary B is a divided difference of the tails P_B(X) = sum_{k >= B} p_k X^(k-B):
//   h^s_B = sum_{i <= s} T[s][i] P_B(z_i),   T[s][i] = z_i^s / prod_{k <= s, k != i} (z_i - z_k)
// (h^s_B = sum_k p_k h_(k-B)(z_0..z_s), the complete homogeneous polynomial, which is that sum of powers).  So a first
// pass reads a tile once and leaves its value at every point, the scan of section 22 turns those into P_B(z_i) (one
// workgroup per row and point: k_kzg_open_carries itself), a small kernel mixes them with the table T into the t
// carries of every tile and the t values P_0(z_i), and the tile pass loads the tile once, runs piece / scan / piece
// t times on the lane's registers and stores once, t places down.
//   products per coefficient: t (1 + 8 / KZG_L) in the first pass, t (2 + 8 / KZG_L) in the tile pass (the scan's
//   multipliers z^(KZG_L 2^d) come from a table, not from squarings); bytes: 64 read + 32 written for any t.
//
// Evaluation form, every point outside the domain.  d_ij = omega^i - z_j, Z_i = prod_j d_ij = Z_S(omega^i),
// w_j = 1 / prod_{k != j} (z_j - z_k), y_j = (z_j^n - 1) / n sum_i f_i omega^i / (z_j - omega^i) and
//   q_i = (f_i - sum_j y_j w_j prod_{k != j} d_ik) / Z_i        (I(omega^i) = Z_i sum_j y_j w_j / d_ij)
// Z_i is inverted once per element, KZG_INV_BATCH of them by one inversion (kzg_chunk_inverses), and 1 / d_ij is
// 1 / Z_i times the product of the other differences (kzg_set_others: prefix and suffix products in registers, which is
// what bounds t by KZG_SET_EV_T).  The first pass leaves 1 / Z_i in the quotient row and the t sums in per-workgroup
// partials; one workgroup per row and point finishes y_j; the second pass writes q_i over 1 / Z_i.
//   products per evaluation: 5 t + 2 + an inversion per KZG_INV_BATCH (first pass), 4 t - 1 (second pass); bytes as
//   the single-point form.
#pragma once
#include <cstddef>

#include "kzg.cuh"

namespace ozk {

constexpr int KZG_SET_T = 32;       // points of a set, coefficient form
constexpr int KZG_SET_EV_T = 8;     // points of a set, evaluation form

// ---- the per-lane pieces ----
// a canonical element as 8 packed words, word by word (these pieces compile without the device's element I/O)
OZK_HD Fe<FrP, 16> kzg_set_ld(const u32* p) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = p[i];
  return unpack<FrP, 16>(w);
}
OZK_HD void kzg_set_st(const Fe<FrP, 16>& v, u32* p) {
  u32 w[8];
  pack(v, w);
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = w[i];
}
// z^e for a small e (Montgomery form)
OZK_HD KzgV kzg_set_pow(const Fe<FrP, 16>& z, int e) {
  KzgV r = KzgV(fe_one<FrP>());
  for (int b = 5; b >= 0; b--) {
    r = KzgV(sqr(r));
    if ((e >> b) & 1) r = KzgV(mul(r, z));
  }
  return r;
}
// one stage over a lane's piece, in place or for its value alone: kzg_piece with the piece as its own output
template <int N, bool KEEP>
OZK_HD KzgV kzg_set_piece(KzgV* v, int n, const Fe<FrP, 16>& z, const KzgV& carry) {
  return kzg_piece<N, KEEP>(v, n, z, carry, v);
}
// row s of the table starts at entry s (s + 1) / 2 and has s + 1 entries
OZK_HD int kzg_set_tab_at(int s, int i) { return s * (s + 1) / 2 + i; }
// the entries T[s][i], s = i .. t - 1, of point i.  zs: the t points, tab: the table, both Montgomery form, canonical,
// 8 words an element.  One inversion: 1 / prod_{k != i} (z_i - z_k), then down the stages a factor at a time.
OZK_HD void kzg_set_table_lane(const u32* zs, int t, int i, u32* tab) {
  const Fe<FrP, 16> zi = kzg_set_ld(zs + 8 * i);
  KzgV run = KzgV(fe_one<FrP>());
  for (int k = 0; k < t; k++)
    if (k != i) run = KzgV(mul(run, sub(zi, kzg_set_ld(zs + 8 * k))));
  KzgV invd = inv(run);
  for (int s = t - 1; s >= i; s--) {
    kzg_set_st(canonical(mul(kzg_set_pow(zi, s), invd)), tab + 8 * kzg_set_tab_at(s, i));
    if (s > i) invd = KzgV(mul(invd, sub(zi, kzg_set_ld(zs + 8 * s))));
  }
}
// what enters stage s at a boundary: sum_{i <= s} T[s][i] P(z_i).  tab_s: row s of the table; pv: the plain canonical
// values P(z_i), element i at pv + i pv_stride words.
OZK_HD KzgV kzg_set_carry(const u32* tab_s, int s, const u32* pv, std::size_t pv_stride) {
  KzgV acc = KzgV(fe_zero<FrP>());
  for (int i = 0; i <= s; i++)
    acc = KzgV(reduce_to<32>(add(acc, mul(kzg_set_ld(pv + (std::size_t)i * pv_stride), kzg_set_ld(tab_s + 8 * i)))));
  return acc;
}
// other_j = prod_{k != j} (w - z_k) for j < t <= KZG_SET_EV_T, and the product of all t differences (returned):
// prefix products up, one running suffix product down.  w, zs (8 words a point, canonical): Montgomery form.
OZK_HD KzgV kzg_set_others(const KzgV& w, const u32* zs, int t, KzgV* other) {
  KzgV run = KzgV(fe_one<FrP>());
#pragma unroll
  for (int j = 0; j < KZG_SET_EV_T; j++) {
    if (j < t) {
      other[j] = run;
      run = KzgV(mul(run, sub(w, kzg_set_ld(zs + 8 * j))));
    }
  }
  KzgV suf = KzgV(fe_one<FrP>());
#pragma unroll
  for (int j = KZG_SET_EV_T - 1; j >= 0; j--) {
    if (j < t) {
      if (j < t - 1) other[j] = KzgV(mul(other[j], suf));
      if (j > 0) suf = KzgV(mul(suf, sub(w, kzg_set_ld(zs + 8 * j))));
    }
  }
  return run;
}
// Z = prod_j (w - z_j) alone
OZK_HD KzgV kzg_set_zprod(const KzgV& w, const u32* zs, int t) {
  KzgV run = KzgV(reduce_to<32>(sub(w, kzg_set_ld(zs))));
  for (int j = 1; j < t; j++) run = KzgV(mul(run, sub(w, kzg_set_ld(zs + 8 * j))));
  return run;
}
// pairwise distinct mod r?  pts: n elements of 8 plain words (any value below 2^256)
inline bool kzg_set_distinct(const u32* pts, int n) {
  for (int a = 1; a < n; a++) {
    u32 wa[8], xa[8];
    for (int i = 0; i < 8; i++) wa[i] = pts[8 * a + i];
    pack(canonical(unpack<FrP, 85>(wa)), xa);
    for (int b = 0; b < a; b++) {
      u32 wb[8], xb[8];
      for (int i = 0; i < 8; i++) wb[i] = pts[8 * b + i];
      pack(canonical(unpack<FrP, 85>(wb)), xb);
      bool same = true;
      for (int i = 0; i < 8; i++) same = same && xa[i] == xb[i];
      if (same) return false;
    }
  }
  return true;
}

#if defined(__HIPCC__)
// ---- host points to the device: kernel arguments (k_fr_put), 96 elements a launch ----
constexpr int KZG_SET_PUT = 96;
static void kzg_set_upload(const uint8_t* host, size_t count, u32* dst, hipStream_t st) {
  for (size_t at = 0; at < count; at += KZG_SET_PUT) {
    const size_t m = count - at < (size_t)KZG_SET_PUT ? count - at : (size_t)KZG_SET_PUT;
    FrWords<KZG_SET_PUT> c;
    memcpy(c.w, host + at * 32, m * 32);
    hipLaunchKernelGGL(k_fr_put<KZG_SET_PUT>, dim3(1), dim3(256), 0, st, c, (int)(m * 8), dst + at * 8);
  }
}

// ---- coefficient form ----
// one wave per row, lane i its point i: the constants of section 22 (so that k_kzg_open_carries serves a row and point
// as it serves a row), the scan's multipliers and the point's entries of the table
__global__ void __launch_bounds__(64) k_kzg_set_consts(const u32* __restrict__ points, int t, KzgRow* __restrict__ rows,
                                                       KzgSetPows* __restrict__ pows, u32* __restrict__ zs,
                                                       u32* __restrict__ tab) {
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x;
  const int i = threadIdx.x;
  if (i < t) {
    const size_t g = y * t + i;
    const auto z = ElemTraits<Fe<FrP, 17>>::from_wire(points + g * 8);
    E16::store(canonical(z), zs + g * 8);
    kzg_row_consts(z, rows + g, pows + g);
  }
  __threadfence_block();
  block_sync();
  if (i < t) kzg_set_table_lane(zs + y * t * 8, t, i, tab + y * (size_t)kzg_set_tab_at(t, 0) * 8);
}

// S_l = a_l + m S_{l+1} as FrScanAffine, with the multiplier of every step read from the row's table
struct KzgSetScan {
  const KzgSetPows* pw;
  __device__ __forceinline__ static KzgV neutral() { return KzgV(fe_zero<FrP>()); }
  __device__ __forceinline__ KzgV apply(const KzgV& a, const KzgV& s, int step) const {
    return kzg_compose(a, KzgV(ElemTraits<Fe<FrP, 16>>::load(pw->m[step])), s);
  }
};

// first pass: the value of tile tl of row y at point i, to agg[(y t + i) nt + tl]; the tile is read once
__global__ void __launch_bounds__(KZG_WG) k_kzg_set_tiles(const u32* __restrict__ coeffs, size_t poly_cs, int len, int nt,
                                                         int t, const KzgRow* __restrict__ rows,
                                                         const KzgSetPows* __restrict__ pows, u32* __restrict__ agg) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * KZG_WG];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x / nt;
  const int tl = blockIdx.x % nt;
  Fe<FrP, 16> p[KZG_L];
  kzg_tile_load(coeffs + y * poly_cs, len, tl, tile, p);
#pragma unroll 1
  for (int i = 0; i < t; i++) {
    const size_t g = y * t + i;
    const KzgV a = kzg_piece<KZG_L, false>(p, KZG_L, E16::load(rows[g].z), KzgV(fe_zero<FrP>()), nullptr);
    const KzgV s = fr_wg_scan<KZG_WG, true>(a, KzgSetScan{pows + g}, part);
    if (threadIdx.x == 0) fr_store(canonical(s), agg + (g * nt + tl) * 8);
  }
}
// the carries of every stage from the tails at every point, and the values.  One lane per (row, tile, stage):
// mixed[(y t + s) nt + tl] = sum_{i <= s} T[s][i] tails[(y t + i) nt + tl]; the lanes of tile 0 also leave
// p(z_s) = (the value of tile 0) + z_s^KZG_TILE (the tail above it).
__global__ void __launch_bounds__(256) k_kzg_set_mix(const u32* __restrict__ agg, const u32* __restrict__ tails, int nt, int t,
                                                     long long total, const KzgRow* __restrict__ rows,
                                                     const u32* __restrict__ tab, u32* __restrict__ mixed,
                                                     u32* __restrict__ values) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const int s = (int)(g % t);
  const int tl = (int)(g / t % nt);
  const size_t y = (size_t)(g / t / nt);
  const u32* row_tab = tab + y * (size_t)kzg_set_tab_at(t, 0) * 8;
  const KzgV c = kzg_set_carry(row_tab + 8 * kzg_set_tab_at(s, 0), s, tails + (y * t * nt + tl) * 8, (size_t)nt * 8);
  const size_t at = (y * t + s) * nt + tl;
  fr_store(canonical(c), mixed + at * 8);
  if (tl == 0) kzg_row_value(agg + at * 8, tails + at * 8, rows[y * t + s], values + (y * t + s) * 8);
}
// the tile pass: t stages on the lane's registers, one store t places down; the last tile of a row also writes the
// zeros that close it
__global__ void __launch_bounds__(KZG_WG) k_kzg_set_apply(const u32* __restrict__ coeffs, size_t poly_cs, int len, int nt,
                                                         int t, const KzgRow* __restrict__ rows,
                                                         const KzgSetPows* __restrict__ pows, const u32* __restrict__ mixed,
                                                         u32* __restrict__ quot, size_t quot_cs) {
  __shared__ __attribute__((aligned(16))) u32 tile[KZG_TILE_WORDS];
  __shared__ u32 part[9 * KZG_WG];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x / nt;
  const int tl = blockIdx.x % nt, l = threadIdx.x;
  KzgV v[KZG_L];
  {
    Fe<FrP, 16> p[KZG_L];
    kzg_tile_load(coeffs + y * poly_cs, len, tl, tile, p);
#pragma unroll
    for (int i = 0; i < KZG_L; i++) v[i] = KzgV(p[i]);
  }
#pragma unroll 1
  for (int s = 0; s < t; s++) {
    const size_t g = y * t + s;
    const auto z = E16::load(rows[g].z);
    const KzgV above = KzgV(fr_load<16>(mixed + (g * nt + tl) * 8));
    KzgV a = kzg_set_piece<KZG_L, false>(v, KZG_L, z, KzgV(fe_zero<FrP>()));
    if (l == KZG_WG - 1) a = kzg_compose(a, KzgV(E16::load(pows[g].m[0])), above);
    fr_wg_scan<KZG_WG, true>(a, KzgSetScan{pows + g}, part);
    const KzgV next = fr_scan_neighbour<KZG_WG, true>(part, above);
    block_sync();   // (the next stage's scan overwrites `part`)
    kzg_set_piece<KZG_L, true>(v, KZG_L, z, next);
  }
  // (a lane overwrites the elements it alone has read); q_(j-t) = h_j: element e of the tile goes t places down
#pragma unroll
  for (int i = 0; i < KZG_L; i++) fr_tile_put(tile, l * KZG_L + i, canonical(v[i]));
  block_sync();
  u32* qrow = quot + y * quot_cs;
  fr_tile_store<KZG_WG, KZG_L>(tile, tl, len, 0, nullptr, t, qrow);
  if (tl == nt - 1 && l < t && len - t + l >= 0) {
    const u32 o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    fr_store_words(o, qrow + (size_t)(len - t + l) * 8);
  }
}

// ---- evaluation form ----
struct KzgSetEv {        // per row and point
  u32 c[8];      // (z^n - 1) / n, Montgomery form
  u32 w[8];      // 1 / prod_{k != j} (z_j - z_k), Montgomery form
  u32 u[8];      // y_j w_j, plain (k_kzg_set_ev_value)
};
// one wave per row, lane j its point j
__global__ void __launch_bounds__(64) k_kzg_set_ev_consts(const u32* __restrict__ points, int t, int n,
                                                          KzgSetEv* __restrict__ ev, u32* __restrict__ zs) {
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x;
  const int j = threadIdx.x;
  if (j < t) {
    const size_t g = y * t + j;
    const auto z = ElemTraits<Fe<FrP, 17>>::from_wire(points + g * 8);
    const u32 nw[8] = {(u32)n, 0, 0, 0, 0, 0, 0, 0};
    E16::store(canonical(z), zs + g * 8);
    E16::store(canonical(mul(sub(fe_pow_u32(z, (unsigned)n), fe_one<FrP>()), inv(to_mont<FrP>(nw)))), ev[g].c);
  }
  __threadfence_block();
  block_sync();
  if (j < t) {
    const u32* row = zs + y * t * 8;
    const Fe<FrP, 16> zj = E16::load(row + 8 * j);
    KzgV run = KzgV(fe_one<FrP>());
    for (int k = 0; k < t; k++)
      if (k != j) run = KzgV(mul(run, sub(zj, E16::load(row + 8 * k))));
    E16::store(canonical(inv(run)), ev[y * t + j].w);
  }
}
// first pass: 1 / Z_i to quot[i] (Montgomery form) and the workgroup's part of sum_i f_i omega^i / d_ij for every j,
// to partial[((y nb + blk) t + j)]
__global__ void __launch_bounds__(KZG_WG) k_kzg_set_ev_inv(const u32* __restrict__ evals, size_t ev_cs, int n, int nb, int t,
                                                          const u32* __restrict__ zs, const u32* __restrict__ pw, int lo,
                                                          u32* __restrict__ quot, size_t quot_cs,
                                                          u32* __restrict__ partial) {
  __shared__ u32 part[9 * 256];
  const size_t y = blockIdx.x / nb;
  const int blk = blockIdx.x % nb;
  const int lanes = (n + KZG_INV_BATCH - 1) / KZG_INV_BATCH;
  const u32* z = zs + y * t * 8;
  const u32* f = evals + y * ev_cs;
  u32* q = quot + y * quot_cs;
  FrAcc acc[KZG_SET_EV_T];
#pragma unroll
  for (int j = 0; j < KZG_SET_EV_T; j++) acc[j] = FrAcc(fe_zero<FrP>());
  const int lane = blk * KZG_WG + threadIdx.x;
  if (lane < lanes) {
    KzgV zi[KZG_INV_BATCH];
    {
      KzgV zp[KZG_INV_BATCH];
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < KZG_INV_BATCH; k++) {
        const int i = k * lanes + lane;   // (interleaved: once i >= n, every later k is too)
        if (i < n) {
          zp[k] = kzg_set_zprod(KzgV(pow_at(pw, lo, i)), z, t);
          cnt = k + 1;
        }
      }
      kzg_chunk_inverses<KZG_INV_BATCH>(zp, cnt, zi);
    }
#pragma unroll 1
    for (int k = 0; k < KZG_INV_BATCH; k++) {
      const int i = k * lanes + lane;
      if (i >= n) break;
      KzgV izk = zi[0];
#pragma unroll
      for (int kk = 1; kk < KZG_INV_BATCH; kk++)
        if (kk == k) izk = zi[kk];
      const KzgV w = KzgV(pow_at(pw, lo, i));
      KzgV other[KZG_SET_EV_T];
      kzg_set_others(w, z, t, other);
      fr_store(canonical(izk), q + (size_t)i * 8);
      const KzgV g = KzgV(mul(fr_load<85>(f + (size_t)i * 8), mul(w, izk)));
#pragma unroll
      for (int j = 0; j < KZG_SET_EV_T; j++)
        if (j < t) acc[j] = FrAcc(reduce_to<32>(add(acc[j], mul(g, other[j]))));
    }
  }
#pragma unroll
  for (int j = 0; j < KZG_SET_EV_T; j++) {
    if (j < t) {   // (uniform over the workgroup)
      const FrAcc sum = fr_block_sum(acc[j], part);
      if (threadIdx.x == 0) fr_store(canonical(sum), partial + ((size_t)blockIdx.x * t + j) * 8);
      block_sync();
    }
  }
}
// one workgroup per row and point: y_j = -c_j sum, and u_j = y_j w_j for the second pass
__global__ void __launch_bounds__(256) k_kzg_set_ev_value(const u32* __restrict__ partial, int nb, int t,
                                                          KzgSetEv* __restrict__ ev, u32* __restrict__ values) {
  __shared__ u32 part[9 * 256];
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x / t;
  const int j = blockIdx.x % t;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = threadIdx.x; i < nb; i += 256)
    acc = FrAcc(reduce_to<32>(add(acc, fr_load<16>(partial + ((y * nb + i) * t + j) * 8))));
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x != 0) return;
  KzgSetEv& e = ev[blockIdx.x];
  const Fe<FrP, 16> val = canonical(neg(mul(sum, E16::load(e.c))));
  fr_store(val, values + (size_t)blockIdx.x * 8);
  E16::store(canonical(mul(val, E16::load(e.w))), e.u);
}
// second pass: q_i = (f_i - sum_j u_j prod_{k != j} d_ik) / Z_i in place of 1 / Z_i
__global__ void __launch_bounds__(KZG_WG) k_kzg_set_ev_quot(const u32* __restrict__ evals, size_t ev_cs, int n, int nb, int t,
                                                           const KzgSetEv* __restrict__ ev, const u32* __restrict__ zs,
                                                           const u32* __restrict__ pw, int lo, u32* __restrict__ quot,
                                                           size_t quot_cs) {
  using E16 = ElemTraits<Fe<FrP, 16>>;
  const size_t y = blockIdx.x / nb;
  const int i = (int)(blockIdx.x % nb) * KZG_WG + threadIdx.x;
  if (i >= n) return;
  u32* q = quot + y * quot_cs + (size_t)i * 8;
  KzgV other[KZG_SET_EV_T];
  kzg_set_others(KzgV(pow_at(pw, lo, i)), zs + y * t * 8, t, other);
  KzgV acc = KzgV(reduce_to<32>(fr_load<85>(evals + y * ev_cs + (size_t)i * 8)));
#pragma unroll
  for (int j = 0; j < KZG_SET_EV_T; j++)
    if (j < t) acc = KzgV(reduce_to<32>(sub(acc, mul(E16::load(ev[y * t + j].u), other[j]))));
  fr_store(canonical(mul(acc, fr_load<16>(q))), q);
}

// ---- host side ----
struct KzgSetLayout {
  u32 *pts, *zs, *tab, *agg, *tails, *mixed;
  KzgRow* rows;
  KzgSetPows* pows;
  int nt;
  size_t bytes;
};
static KzgSetLayout kzg_set_layout(int npolys, int len, int t, void* wsp) {
  KzgSetLayout L;
  Bump b(wsp, ~(size_t)0);
  const size_t np = (size_t)npolys * t;
  L.nt = (len + KZG_TILE - 1) / KZG_TILE;
  L.pts = b.take<u32>(np * 8);
  L.zs = b.take<u32>(np * 8);
  L.rows = b.take<KzgRow>(np);
  L.pows = b.take<KzgSetPows>(np);
  L.tab = b.take<u32>((size_t)npolys * kzg_set_tab_at(t, 0) * 8);
  L.agg = b.take<u32>(np * L.nt * 8);
  L.tails = b.take<u32>(np * L.nt * 8);
  L.mixed = b.take<u32>(np * L.nt * 8);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
struct KzgSetEvLayout {
  u32 *pts, *zs, *omega, *pw, *partial;
  KzgSetEv* ev;
  int nb_inv, nb_quot;
  size_t bytes;
};
static KzgSetEvLayout kzg_set_ev_layout(int npolys, int n, int t, void* wsp) {
  KzgSetEvLayout L;
  Bump b(wsp, ~(size_t)0);
  const size_t np = (size_t)npolys * t;
  L.nb_inv = kzg_ev_blocks((n + KZG_INV_BATCH - 1) / KZG_INV_BATCH);
  L.nb_quot = kzg_ev_blocks(n);
  L.pts = b.take<u32>(np * 8);
  L.zs = b.take<u32>(np * 8);
  L.ev = b.take<KzgSetEv>(np);
  L.omega = b.take<u32>(8);
  L.pw = b.take<u32>(PowTable::upto(n).words());
  L.partial = b.take<u32>(np * L.nb_inv * 8);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static bool kzg_set_rows_distinct(const uint8_t* points_host, int npolys, int t) {
  for (int y = 0; y < npolys; y++) {
    u32 w[8 * KZG_SET_T];
    memcpy(w, points_host + (size_t)y * t * 32, (size_t)t * 32);
    if (!kzg_set_distinct(w, t)) return false;
  }
  return true;
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

size_t ozk_fr_poly_open_set_workspace_bytes(int32_t npolys, int32_t len, int32_t t) {
  if (!kzg_shape_ok(npolys, len) || t < 1 || t > KZG_SET_T || (long long)npolys * t > KZG_MAX_ELEMS) return 0;
  return kzg_set_layout(npolys, len, t, nullptr).bytes;
}

int ozk_fr_poly_open_set_dev(const void* d_coeffs, int32_t npolys, int32_t len, int64_t poly_stride, int32_t t,
                             const uint8_t* points_host, void* d_quot, int64_t quot_stride, void* d_values,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(npolys, len))
    return fail(OZK_E_INVALID, "bad shape: %d polynomials of %d coefficients (1 <= both, product <= 2^28)", npolys, len);
  if (t < 1 || t > KZG_SET_T || (long long)npolys * t > KZG_MAX_ELEMS)
    return fail(OZK_E_INVALID, "bad set: %d points a row (1 <= t <= %d, npolys t <= 2^28)", t, KZG_SET_T);
  if ((poly_stride != 0 && poly_stride < len) || quot_stride < len)
    return fail(OZK_E_INVALID, "bad strides: poly_stride %lld (0 or >= len), quot_stride %lld (>= len), len %d",
                (long long)poly_stride, (long long)quot_stride, len);
  if (int rc = fr_check_pointers(d_coeffs, points_host, d_quot, d_values, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_coeffs, d_quot, d_values)) return rc;
  if (kzg_overlap(d_coeffs, kzg_span(npolys, len, poly_stride), d_quot, kzg_span(npolys, len, quot_stride)))
    return fail(OZK_E_INVALID, "d_quot overlaps d_coeffs");
  if (!kzg_set_rows_distinct(points_host, npolys, t))
    return fail(OZK_E_INVALID, "the %d points of a row are not pairwise distinct mod r", t);
  const KzgSetLayout L = kzg_set_layout(npolys, len, t, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const u32* c = (const u32*)d_coeffs;
  const size_t pcs = (size_t)poly_stride * 8, qcs = (size_t)quot_stride * 8;
  const size_t np = (size_t)npolys * t;
  const unsigned grid = (unsigned)((long long)npolys * L.nt);
  const long long mix = (long long)np * L.nt;
  kzg_set_upload(points_host, np, L.pts, st);
  hipLaunchKernelGGL(k_kzg_set_consts, dim3(npolys), dim3(64), 0, st, (const u32*)L.pts, t, L.rows, L.pows, L.zs, L.tab);
  hipLaunchKernelGGL(k_kzg_set_tiles, dim3(grid), dim3(KZG_WG), 0, st, c, pcs, len, L.nt, t, (const KzgRow*)L.rows,
                     (const KzgSetPows*)L.pows, L.agg);
  hipLaunchKernelGGL(k_kzg_open_carries, dim3((unsigned)np), dim3(KZG_WG), 0, st, (const u32*)L.agg, L.nt,
                     (const KzgRow*)L.rows, L.tails);
  hipLaunchKernelGGL(k_kzg_set_mix, dim3((unsigned)((mix + 255) / 256)), dim3(256), 0, st, (const u32*)L.agg,
                     (const u32*)L.tails, L.nt, t, mix, (const KzgRow*)L.rows, (const u32*)L.tab, L.mixed, (u32*)d_values);
  hipLaunchKernelGGL(k_kzg_set_apply, dim3(grid), dim3(KZG_WG), 0, st, c, pcs, len, L.nt, t, (const KzgRow*)L.rows,
                     (const KzgSetPows*)L.pows, (const u32*)L.mixed, (u32*)d_quot, qcs);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_fr_evals_open_set_workspace_bytes(int32_t npolys, int32_t n, int32_t t) {
  if (!kzg_shape_ok(npolys, n) || n < 2 || (n & (n - 1)) || t < 1 || t > KZG_SET_EV_T) return 0;
  return kzg_set_ev_layout(npolys, n, t, nullptr).bytes;
}

int ozk_fr_evals_open_set_dev(const void* d_evals, int32_t npolys, int32_t n, int64_t evals_stride,
                              const uint8_t* omega_host32, int32_t t, const uint8_t* points_host, void* d_quot,
                              int64_t quot_stride, void* d_values, void* d_workspace, size_t workspace_bytes,
                              void* stream) {
  hip_clear_stale();
  if (!kzg_shape_ok(npolys, n))
    return fail(OZK_E_INVALID, "bad shape: %d rows of %d evaluations (1 <= both, product <= 2^28)", npolys, n);
  if (int rc = check_pow2(n, 2, "domain size")) return rc;
  if (t < 1 || t > KZG_SET_EV_T) return fail(OZK_E_INVALID, "bad set: %d points (1 <= t <= %d)", t, KZG_SET_EV_T);
  if ((evals_stride != 0 && evals_stride < n) || quot_stride < n)
    return fail(OZK_E_INVALID, "bad strides: evals_stride %lld (0 or >= n), quot_stride %lld (>= n), n %d",
                (long long)evals_stride, (long long)quot_stride, n);
  if (int rc = fr_check_pointers(d_evals, omega_host32, points_host, d_quot, d_values, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_evals, d_quot, d_values)) return rc;
  if (kzg_overlap(d_evals, kzg_span(npolys, n, evals_stride), d_quot, kzg_span(npolys, n, quot_stride)))
    return fail(OZK_E_INVALID, "d_quot overlaps d_evals");
  if (!fr_omega_has_order(omega_host32, n))
    return fail(OZK_E_INVALID, "omega does not have order %d (omega^(n/2) != -1)", n);
  if (!kzg_set_rows_distinct(points_host, npolys, t))
    return fail(OZK_E_INVALID, "the %d points of a row are not pairwise distinct mod r", t);
  for (size_t g = 0; g < (size_t)npolys * t; g++)
    if (fr_in_domain(points_host + g * 32, n))
      return fail(OZK_E_INVALID, "point %zu of row %zu lies in the domain (z^n = 1): open such a set in coefficient form",
                  g % t, g / t);
  const KzgSetEvLayout L = kzg_set_ev_layout(npolys, n, t, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const u32* f = (const u32*)d_evals;
  const size_t ecs = (size_t)evals_stride * 8, qcs = (size_t)quot_stride * 8;
  const size_t np = (size_t)npolys * t;
  fr_put_element(omega_host32, L.omega, st);
  const PowTable pt = PowTable::upto(n);
  pt.build(L.omega, L.pw, st);
  kzg_set_upload(points_host, np, L.pts, st);
  hipLaunchKernelGGL(k_kzg_set_ev_consts, dim3(npolys), dim3(64), 0, st, (const u32*)L.pts, t, n, L.ev, L.zs);
  hipLaunchKernelGGL(k_kzg_set_ev_inv, dim3((unsigned)((long long)npolys * L.nb_inv)), dim3(KZG_WG), 0, st, f, ecs, n,
                     L.nb_inv, t, (const u32*)L.zs, (const u32*)L.pw, pt.lo, (u32*)d_quot, qcs, L.partial);
  hipLaunchKernelGGL(k_kzg_set_ev_value, dim3((unsigned)np), dim3(256), 0, st, (const u32*)L.partial, L.nb_inv, t, L.ev,
                     (u32*)d_values);
  hipLaunchKernelGGL(k_kzg_set_ev_quot, dim3((unsigned)((long long)npolys * L.nb_quot)), dim3(KZG_WG), 0, st, f, ecs, n,
                     L.nb_quot, t, (const KzgSetEv*)L.ev, (const u32*)L.zs, (const u32*)L.pw, pt.lo, (u32*)d_quot, qcs);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
