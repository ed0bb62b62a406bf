// The Fr kernels of the PLONK prover: rows scaled by the powers of a coset shift, the permutation
// grand product, and the quotient pointwise on the coset of four times the domain.  A section of the plonk.hip unit,
// which alone includes it: kernels, layouts and entry points.  It uses the element I/O and kernel-argument words of
// fr_tables.cuh and the staged tile, scan, chunked inversion and entry checks of fr_rows.cuh; no KZG kernel.
//
// Every value in HBM is 32 bytes LE, plain (non-Montgomery); inputs are taken mod r, outputs are canonical.  The
// scalars of a call arrive in host memory and travel in the kernel arguments, already in the form the kernel
// multiplies by: nothing is uploaded.
//
// Rows by powers.  out[y][i] = c s^i rows[y][i], zero from len to out_len.  A workgroup takes PLONK_CO_TILE elements of
// one row, lane l the elements l, l + 256, ...: its power starts at (c s^(tile t)) s^l, two entries of a table of
// 256 + (number of tiles) elements that a first kernel leaves in the workspace, and moves on by s^256.
//   products per element: 2 + 1 / 4; bytes: 32 read + 32 written (32 written alone past len).
//
// Grand product.  z_0 = 1, z_{i+1} = z_i f_i with f_i = prod_j (w_ji + beta k_j omega^i + gamma) / (w_ji + beta s_ji + gamma).
// A workgroup of PLONK_WG lanes stages the tile of every one of the six rows in LDS (coalesced reads); a lane owns
// PLONK_L = KZG_INV_BATCH consecutive rows of the tile, whose three labels move on by omega from one start power, and
// inverts their denominators with one safegcd inversion (kzg_chunk_inverses: a zero denominator stays out of the
// running product; its row's factor is 1 and it is counted).  Three phases as in kzg.cuh: the product of every tile,
// an exclusive scan of those by one workgroup, and the tile pass, which scans the lanes' products from the carry into
// its tile and writes z through LDS.  A row of one tile runs the tile pass alone.
//   products per row: 33 (factors, inverse, scan) + an inversion per KZG_INV_BATCH per pass;
//   bytes per row: 6 x 32 read in each of the two passes, 32 written.
//
// Quotient.  One point of the coset per lane: t = (gate + alpha P1 + alpha^2 P2) / Z_H from one read of the fifteen
// rows and of Z four places on.  Z_H takes four values on the coset; their inverses come with the call.
//   products per point: 26 (3 conversions, the gate 7, P1 12, P2 2, the weights 2); bytes: 16 x 32 read + 32 written.
#pragma once
#include "fr_rows.cuh"

namespace ozk {

constexpr int PLONK_CO_WG = 256;                        // lanes of a rows-by-powers workgroup
constexpr int PLONK_CO_L = 4;                           // elements of a lane, PLONK_CO_WG apart
constexpr int PLONK_CO_TILE = PLONK_CO_WG * PLONK_CO_L;
constexpr int PLONK_WG = 128;                           // lanes of a grand-product workgroup
constexpr int PLONK_L = KZG_INV_BATCH;                  // consecutive rows of a lane: one inversion
constexpr int PLONK_TILE = PLONK_WG * PLONK_L;          // two staged tiles (66 KiB of LDS) + 4.5 KiB of scan
constexpr int PLONK_SCAN_WG = 256;                      // tile products scanned at a time
static_assert(PLONK_TILE == KZG_TILE, "the staged tile is fr_rows.cuh's (kzg_at)");

#if defined(__HIPCC__)
// one element in the kernel arguments (FrArg): canonical, packed
__device__ __forceinline__ Fe<FrP, 16> plonk_arg(const FrArg& c) { return unpack<FrP, 16>(c.w); }

// tab[l] = base^(l step) for l < ntab (plain when tab_plain, else Montgomery form); start[t] = c base^(t tile) for
// t < nt (Montgomery form).  base, c: Montgomery form.
__global__ void __launch_bounds__(64) k_plonk_pows(FrArg base, FrArg c, int ntab, unsigned step, int tab_plain,
                                                   int nt, unsigned tile, u32* __restrict__ tab, u32* __restrict__ start) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ntab + nt) return;
  const auto b = plonk_arg(base);
  if (g < ntab) {
    const auto v = fe_pow_u32(b, (unsigned)g * step);
    u32 o[8];
    if (tab_plain) from_mont(v, o);
    else pack(canonical(v), o);
    fr_store_words(o, tab + (size_t)g * 8);
  } else {
    fr_store(canonical(mul(fe_pow_u32(b, (unsigned)(g - ntab) * tile), plonk_arg(c))), start + (size_t)(g - ntab) * 8);
  }
}

// ---- rows by powers: tile blockIdx.x % nt of row blockIdx.x / nt.  out may be rows (a lane writes what it alone read)
__global__ void __launch_bounds__(PLONK_CO_WG) k_fr_rows_coset(const u32* rows, int len, size_t row_cs, int nt, FrArg s_wg,
                                                              const u32* __restrict__ tab, const u32* __restrict__ start,
                                                              u32* out, int out_len, size_t out_cs) {
  const int y = blockIdx.x / nt, t = blockIdx.x % nt, l = threadIdx.x;
  const u32* in = rows + (size_t)y * row_cs;
  u32* o = out + (size_t)y * out_cs;
  const long long j0 = (long long)t * PLONK_CO_TILE + l;
  KzgV p = KzgV(fe_zero<FrP>());
  if (j0 < len) p = KzgV(mul(fr_load<16>(start + (size_t)t * 8), fr_load<16>(tab + (size_t)l * 8)));
  const auto step = plonk_arg(s_wg);
#pragma unroll
  for (int i = 0; i < PLONK_CO_L; i++) {
    const long long j = j0 + (long long)i * PLONK_CO_WG;
    if (j >= out_len) break;
    if (j < len) {
      fr_store(canonical(mul(fr_load<85>(in + (size_t)j * 8), p)), o + (size_t)j * 8);
      if (i + 1 < PLONK_CO_L) p = KzgV(mul(p, step));
    } else {
      const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      fr_store_words(zero, o + (size_t)j * 8);
    }
  }
}

// ---- grand product
struct PlonkPermArgs {
  FrArg omega, beta, bk[3];   // Montgomery form: omega, beta, beta k_j
  FrArg gamma;                // plain
};

// Column j of the six rows folded into the lane's running numerators f and denominators d: both tiles are staged,
// read and free again on return.  label: beta k_j omega^i at the lane's first row, plain.
template <bool FIRST>
__device__ __forceinline__ void plonk_column(const u32* __restrict__ w_row, const u32* __restrict__ s_row, int len, int t,
                                             KzgV label, const Fe<FrP, 16>& omega, const Fe<FrP, 16>& beta,
                                             const Fe<FrP, 16>& gamma, u32* tile_w, u32* tile_s, KzgV (&f)[PLONK_L],
                                             KzgV (&d)[PLONK_L]) {
  fr_tile_fill<PLONK_WG, PLONK_L>(w_row, len, t, tile_w);
  fr_tile_fill<PLONK_WG, PLONK_L>(s_row, len, t, tile_s);
  block_sync();
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    const int e = threadIdx.x * PLONK_L + k;
    const auto wg = add(fr_tile_get(tile_w, e), gamma);
    const auto num = add(wg, label);
    const auto den = add(wg, mul(fr_tile_get(tile_s, e), beta));
    if (FIRST) {
      f[k] = KzgV(reduce_to<32>(num));
      d[k] = KzgV(reduce_to<32>(den));
    } else {
      f[k] = KzgV(mul(f[k], num));
      d[k] = KzgV(mul(d[k], den));
    }
    if (k + 1 < PLONK_L) label = KzgV(mul(label, omega));
  }
  block_sync();
}
// f[k], Montgomery form, for the lane's rows t PLONK_TILE + PLONK_L threadIdx.x + k (1 for a row beyond len and for
// a zero denominator); returns how many of its denominators are zero.  Both tiles are free on return.
//   With plain operands a product of three factors carries 1 / R^2, numerator and denominator alike; the inverse
//   of the denominator read as a Montgomery form is then R^4 / D, and (N / R^2) (R^4 / D) / R = (N / D) R.
__device__ __forceinline__ int plonk_factors(const u32* __restrict__ wires, const u32* __restrict__ sigma, int len, size_t cs,
                                             int t, const PlonkPermArgs& a, const u32* __restrict__ tab,
                                             const u32* __restrict__ start, u32* tile_w, u32* tile_s, KzgV (&f)[PLONK_L]) {
  const int l = threadIdx.x;
  const auto omega = plonk_arg(a.omega), beta = plonk_arg(a.beta), gamma = plonk_arg(a.gamma);
  // omega^(first row of the lane), plain
  const KzgV p0 = KzgV(mul(fr_load<16>(start + (size_t)t * 8), fr_load<16>(tab + (size_t)l * 8)));
  KzgV d[PLONK_L];
  plonk_column<true>(wires, sigma, len, t, KzgV(mul(p0, plonk_arg(a.bk[0]))), omega, beta, gamma, tile_w, tile_s, f, d);
  plonk_column<false>(wires + cs, sigma + cs, len, t, KzgV(mul(p0, plonk_arg(a.bk[1]))), omega, beta, gamma, tile_w, tile_s,
                      f, d);
  plonk_column<false>(wires + 2 * cs, sigma + 2 * cs, len, t, KzgV(mul(p0, plonk_arg(a.bk[2]))), omega, beta, gamma, tile_w,
                      tile_s, f, d);
  int zeros = 0;
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    if ((long long)t * PLONK_TILE + l * PLONK_L + k >= len) {
      f[k] = KzgV(fe_one<FrP>());
      d[k] = KzgV(fe_one<FrP>());
    } else if (is_zero(d[k])) {
      zeros++;
    }
  }
  KzgV di[PLONK_L];
  kzg_chunk_inverses<PLONK_L>(d, PLONK_L, di);
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) f[k] = is_zero(d[k]) ? KzgV(fe_one<FrP>()) : KzgV(mul(f[k], di[k]));
  return zeros;
}
__device__ __forceinline__ KzgV plonk_lane_product(const KzgV (&f)[PLONK_L]) {
  KzgV a = f[0];
#pragma unroll
  for (int k = 1; k < PLONK_L; k++) a = KzgV(mul(a, f[k]));
  return a;
}

// first pass (several tiles): the product of tile t, Montgomery form, to agg[t]
__global__ void __launch_bounds__(PLONK_WG) k_plonk_perm_tiles(const u32* __restrict__ wires, const u32* __restrict__ sigma,
                                                              int len, size_t cs, PlonkPermArgs a,
                                                              const u32* __restrict__ tab, const u32* __restrict__ start,
                                                              u32* __restrict__ agg) {
  __shared__ __attribute__((aligned(16))) u32 tile_w[KZG_TILE_WORDS];
  __shared__ __attribute__((aligned(16))) u32 tile_s[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  KzgV f[PLONK_L];
  plonk_factors(wires, sigma, len, cs, blockIdx.x, a, tab, start, tile_w, tile_s, f);
  const KzgV s = fr_wg_scan<PLONK_WG, false>(plonk_lane_product(f), FrScanProduct{}, part);
  if (threadIdx.x == PLONK_WG - 1) fr_store(canonical(s), agg + (size_t)blockIdx.x * 8);
}
// second pass, one workgroup: carry[t] = the product of the tiles below t, PLONK_SCAN_WG tiles at a time from the bottom
__global__ void __launch_bounds__(PLONK_SCAN_WG) k_plonk_perm_carries(const u32* __restrict__ agg, int nt, u32* __restrict__ carry) {
  __shared__ u32 part[9 * PLONK_SCAN_WG];
  fr_carries_scan<PLONK_SCAN_WG, false>(agg, nt, FrScanProduct{}, carry, part);
}
// the tile pass: z, the count of zero denominators and, from the last tile, the product of all rows.  carry: null
// when the row is one tile.
__global__ void __launch_bounds__(PLONK_WG) k_plonk_perm_apply(const u32* __restrict__ wires, const u32* __restrict__ sigma,
                                                              int len, size_t cs, int nt, PlonkPermArgs a,
                                                              const u32* __restrict__ tab, const u32* __restrict__ start,
                                                              const u32* __restrict__ carry, u32* __restrict__ z,
                                                              u32* __restrict__ total, int* __restrict__ zero_dens) {
  __shared__ __attribute__((aligned(16))) u32 tile_w[KZG_TILE_WORDS];
  __shared__ __attribute__((aligned(16))) u32 tile_s[KZG_TILE_WORDS];
  __shared__ u32 part[9 * PLONK_WG];
  const int t = blockIdx.x, l = threadIdx.x;
  KzgV f[PLONK_L];
  const int zeros = plonk_factors(wires, sigma, len, cs, t, a, tab, start, tile_w, tile_s, f);
  if (zeros) atomicAdd(zero_dens, zeros);
  KzgV below = KzgV(fe_one<FrP>());
  if (carry) below = KzgV(fr_load<16>(carry + (size_t)t * 8));
  KzgV prod = plonk_lane_product(f);
  if (l == 0) prod = KzgV(mul(prod, below));
  const KzgV s = fr_wg_scan<PLONK_WG, false>(prod, FrScanProduct{}, part);
  if (t == nt - 1 && l == PLONK_WG - 1) {
    u32 o[8];
    from_mont(s, o);
    fr_store_words(o, total);
  }
  // the product below the lane's first row, out of Montgomery form; a plain value times f stays plain
  Fe<FrP, 1> one = fe_zero<FrP>();
  one.l[0] = 1;
  KzgV run = KzgV(mul(fr_scan_neighbour<PLONK_WG, false>(part, below), one));
#pragma unroll
  for (int k = 0; k < PLONK_L; k++) {
    fr_tile_put(tile_w, l * PLONK_L + k, canonical(run));
    if (k + 1 < PLONK_L) run = KzgV(mul(run, f[k]));
  }
  block_sync();
  fr_tile_store<PLONK_WG, PLONK_L>(tile_w, t, len, 0, nullptr, 0, z);
}

// ---- quotient
struct PlonkQuotArgs {
  FrArg alpha_r, alpha2_r2;   // alpha R, alpha^2 R^2
  FrArg beta_r2, bk_r2[3];    // beta R^2, beta k_j R^2
  FrArg gamma_r;              // gamma R
  FrArg zh_r[4];              // R / (g^n i4^m - 1), m < 4
};
enum { PLONK_A, PLONK_B, PLONK_C, PLONK_Z, PLONK_PI, PLONK_WIT_ROWS };
enum { PLONK_QL, PLONK_QR, PLONK_QO, PLONK_QM, PLONK_QC, PLONK_S1, PLONK_S2, PLONK_S3, PLONK_L1, PLONK_X, PLONK_KEY_ROWS };

// an input element below 2 r
__device__ __forceinline__ KzgV plonk_in(const u32* __restrict__ rows, size_t cs, int row, unsigned i) {
  return KzgV(reduce_to<32>(fr_load<85>(rows + (size_t)row * cs + (size_t)i * 8)));
}
// gate + alpha P1 + alpha^2 P2 at point i of the coset, plain, not yet divided by Z_H: the identity of the vanilla
// circuit, stated here once for k_plonk_quotient and for the lookup quotient of plonk_lookup.cuh.  a, b, c leave in
// Montgomery form for the caller's further terms.
// Plain operands: a product with an operand carrying R (or R^2) comes out plain (or in Montgomery form), so a, b, c
// are brought into Montgomery form once and every term of the sum below is a plain value.
__device__ __forceinline__ auto plonk_vanilla_terms(const u32* __restrict__ wit, size_t wit_cs, const u32* __restrict__ key,
                                                    size_t key_cs, unsigned n4, unsigned i, const PlonkQuotArgs& q, KzgV& a,
                                                    KzgV& b, KzgV& c) {
  const auto r2 = fe_const<FrP, 16>(FrP::R2);
  const auto gamma_r = plonk_arg(q.gamma_r);
  a = KzgV(mul(plonk_in(wit, wit_cs, PLONK_A, i), r2));
  b = KzgV(mul(plonk_in(wit, wit_cs, PLONK_B, i), r2));
  c = KzgV(mul(plonk_in(wit, wit_cs, PLONK_C, i), r2));
  // qL a + qR b + qO c + qM a b + qC + PI
  const auto qma = mul(plonk_in(key, key_cs, PLONK_QM, i), a);
  const auto gate = add(add(mul2(plonk_in(key, key_cs, PLONK_QL, i), a, plonk_in(key, key_cs, PLONK_QR, i), b),
                            mul2(plonk_in(key, key_cs, PLONK_QO, i), c, qma, b)),
                        add(plonk_in(key, key_cs, PLONK_QC, i), plonk_in(wit, wit_cs, PLONK_PI, i)));
  // Z (a + beta x + gamma)(b + beta k1 x + gamma)(c + beta k2 x + gamma)
  const KzgV zv = plonk_in(wit, wit_cs, PLONK_Z, i);
  const KzgV x = plonk_in(key, key_cs, PLONK_X, i);
  const auto ag = add(a, gamma_r), bg = add(b, gamma_r), cg = add(c, gamma_r);
  const auto left = mul(mul(mul(zv, add(ag, mul(x, plonk_arg(q.bk_r2[0])))), add(bg, mul(x, plonk_arg(q.bk_r2[1])))),
                        add(cg, mul(x, plonk_arg(q.bk_r2[2]))));
  // Z(omega X)(a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma): omega = omega_4n^4
  const KzgV zw = plonk_in(wit, wit_cs, PLONK_Z, (i + 4) & (n4 - 1));
  const auto beta_r2 = plonk_arg(q.beta_r2);
  const auto right = mul(mul(mul(zw, add(ag, mul(plonk_in(key, key_cs, PLONK_S1, i), beta_r2))),
                             add(bg, mul(plonk_in(key, key_cs, PLONK_S2, i), beta_r2))),
                         add(cg, mul(plonk_in(key, key_cs, PLONK_S3, i), beta_r2)));
  // (Z - 1) L_1, with 1 / R
  Fe<FrP, 1> one = fe_zero<FrP>();
  one.l[0] = 1;
  const auto p2 = mul(sub(zv, one), plonk_in(key, key_cs, PLONK_L1, i));
  return add(gate, mul2(sub(left, right), plonk_arg(q.alpha_r), p2, plonk_arg(q.alpha2_r2)));
}
__global__ void __launch_bounds__(256) k_plonk_quotient(const u32* __restrict__ wit, size_t wit_cs, const u32* __restrict__ key,
                                                        size_t key_cs, unsigned n4, PlonkQuotArgs q, u32* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  KzgV a, b, c;
  const auto sum = plonk_vanilla_terms(wit, wit_cs, key, key_cs, n4, i, q, a, b, c);
  fr_store(canonical(mul(sum, plonk_arg(q.zh_r[i & 3]))), out + (size_t)i * 8);
}

// ---- host side ----
template <int B>
static FrArg plonk_words(const Fe<FrP, B>& v) {
  FrArg o;
  pack(canonical(v), o.w);
  return o;
}
static Fe<FrP, 17> plonk_mont(const uint8_t* host32) {
  u32 w[8];
  memcpy(w, host32, 32);
  return to_mont<FrP>(w);
}
static FrArg plonk_plain(const uint8_t* host32) {
  u32 w[8];
  memcpy(w, host32, 32);
  return plonk_words(unpack<FrP, 85>(w));
}

struct PlonkPowLayout {
  u32 *tab, *start;
  int nt;
  size_t bytes;
};
static PlonkPowLayout plonk_coset_layout(int out_len, void* wsp) {
  PlonkPowLayout L;
  Bump b(wsp, ~(size_t)0);
  L.nt = (out_len + PLONK_CO_TILE - 1) / PLONK_CO_TILE;
  L.tab = b.take<u32>((size_t)PLONK_CO_WG * 8);
  L.start = b.take<u32>((size_t)L.nt * 8);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static bool plonk_coset_shape_ok(int k, int len, int out_len) {
  return k >= 1 && len >= 1 && out_len >= len && (long long)k * out_len <= KZG_MAX_ELEMS;
}
struct PlonkPermLayout {
  u32 *tab, *start, *agg, *carry;
  int nt;
  size_t bytes;
};
static PlonkPermLayout plonk_perm_layout(int len, void* wsp) {
  PlonkPermLayout L;
  Bump b(wsp, ~(size_t)0);
  L.nt = (len + PLONK_TILE - 1) / PLONK_TILE;
  L.tab = b.take<u32>((size_t)PLONK_WG * 8);
  L.start = b.take<u32>((size_t)L.nt * 8);
  const size_t per = L.nt > 1 ? (size_t)L.nt * 8 : 0;
  L.agg = b.take<u32>(per);
  L.carry = b.take<u32>(per);
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static bool plonk_perm_shape_ok(int len) { return len >= 1 && (long long)len <= KZG_MAX_ELEMS; }
// the checks and the scalars that the quotient's two entry points (this one and plonk_lookup.cuh's) share
static int plonk_quot_shape(int n, long long wit_stride, long long key_stride) {
  if (n < 2 || (n & (n - 1)) || n > (1 << 26))
    return fail(OZK_E_INVALID, "n = %d is not a power of two in [2, 2^26] (the coset has 4 n <= 2^28 points)", n);
  if (wit_stride < 4 * n || key_stride < 4 * n)
    return fail(OZK_E_INVALID, "bad strides: wit_stride %lld, key_stride %lld (both >= 4 n = %d)", wit_stride, key_stride,
                4 * n);
  return OZK_OK;
}
static int plonk_quot_buffers(const void* d_wit, int wit_rows, long long wit_stride, const void* d_key, int key_rows,
                              long long key_stride, int n, const void* d_out) {
  if (int rc = fr_check_aligned16(d_wit, d_key, d_out)) return rc;
  const int n4 = 4 * n;
  if (kzg_overlap(d_wit, kzg_span(wit_rows, n4, wit_stride), d_out, (size_t)n4 * 32) ||
      kzg_overlap(d_key, kzg_span(key_rows, n4, key_stride), d_out, (size_t)n4 * 32))
    return fail(OZK_E_INVALID, "d_out overlaps d_wit or d_key");
  return OZK_OK;
}
static PlonkQuotArgs plonk_quot_args(const uint8_t* alpha_host32, const uint8_t* beta_host32, const uint8_t* gamma_host32,
                                     const uint8_t* k_host96, const uint8_t* zh_inv_host128) {
  PlonkQuotArgs q;
  const auto r2 = fe_const<FrP, 16>(FrP::R2);
  const auto alpha = plonk_mont(alpha_host32), beta = plonk_mont(beta_host32);
  q.alpha_r = plonk_words(alpha);
  q.alpha2_r2 = plonk_words(mul(sqr(alpha), r2));
  q.beta_r2 = plonk_words(mul(beta, r2));
  for (int j = 0; j < 3; j++) q.bk_r2[j] = plonk_words(mul(mul(beta, plonk_mont(k_host96 + 32 * j)), r2));
  q.gamma_r = plonk_words(plonk_mont(gamma_host32));
  for (int m = 0; m < 4; m++) q.zh_r[m] = plonk_words(plonk_mont(zh_inv_host128 + 32 * m));
  return q;
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

size_t ozk_fr_rows_coset_workspace_bytes(int32_t k, int32_t len, int32_t out_len) {
  if (!plonk_coset_shape_ok(k, len, out_len)) return 0;
  return plonk_coset_layout(out_len, nullptr).bytes;
}

int ozk_fr_rows_coset_dev(const void* d_rows, int32_t k, int32_t len, int64_t row_stride, const uint8_t* s_host32,
                          const uint8_t* c_host32, void* d_out, int32_t out_len, int64_t out_stride, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!plonk_coset_shape_ok(k, len, out_len))
    return fail(OZK_E_INVALID, "bad shape: %d rows of %d elements to %d (1 <= k, 1 <= len <= out_len, k out_len <= 2^28)", k,
                len, out_len);
  if (row_stride < len || out_stride < out_len)
    return fail(OZK_E_INVALID, "bad strides: row_stride %lld (>= len %d), out_stride %lld (>= out_len %d)",
                (long long)row_stride, len, (long long)out_stride, out_len);
  if (int rc = fr_check_pointers(d_rows, s_host32, c_host32, d_out, d_workspace)) return rc;
  if (int rc = fr_check_aligned16(d_rows, d_out)) return rc;
  const bool in_place = d_out == d_rows && out_len == len && out_stride == row_stride;
  if (!in_place && kzg_overlap(d_rows, kzg_span(k, len, row_stride), d_out, kzg_span(k, out_len, out_stride)))
    return fail(OZK_E_INVALID, "d_out overlaps d_rows (it may only be d_rows itself, with out_len = len and equal strides)");
  const PlonkPowLayout L = plonk_coset_layout(out_len, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const auto s = plonk_mont(s_host32);
  hipLaunchKernelGGL(k_plonk_pows, dim3((PLONK_CO_WG + L.nt + 63) / 64), dim3(64), 0, st, plonk_words(s),
                     plonk_words(plonk_mont(c_host32)), PLONK_CO_WG, 1u, 0, L.nt, (unsigned)PLONK_CO_TILE, L.tab, L.start);
  hipLaunchKernelGGL(k_fr_rows_coset, dim3((unsigned)((long long)k * L.nt)), dim3(PLONK_CO_WG), 0, st, (const u32*)d_rows, len,
                     (size_t)row_stride * 8, L.nt, plonk_words(fe_pow_u32(s, PLONK_CO_WG)), (const u32*)L.tab,
                     (const u32*)L.start, (u32*)d_out, out_len, (size_t)out_stride * 8);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_fr_perm_product_workspace_bytes(int32_t len) {
  if (!plonk_perm_shape_ok(len)) return 0;
  return plonk_perm_layout(len, nullptr).bytes;
}

int ozk_fr_perm_product_dev(const void* d_wires, const void* d_sigma, int32_t len, int64_t stride, const uint8_t* omega_host32,
                            const uint8_t* k_host96, const uint8_t* beta_host32, const uint8_t* gamma_host32, void* d_z,
                            void* d_total, int32_t* d_zero_dens, void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (!plonk_perm_shape_ok(len)) return fail(OZK_E_INVALID, "bad shape: %d rows (1 <= len <= 2^28)", len);
  if (stride < len) return fail(OZK_E_INVALID, "bad stride: %lld (>= len %d)", (long long)stride, len);
  if (int rc = fr_check_pointers(d_wires, d_sigma, omega_host32, k_host96, beta_host32, gamma_host32, d_z, d_total,
                                 d_zero_dens, d_workspace))
    return rc;
  if (int rc = fr_check_aligned16(d_wires, d_sigma, d_z, d_total)) return rc;
  if (((uintptr_t)d_zero_dens & 3) != 0) return fail(OZK_E_INVALID, "d_zero_dens must be 4-byte aligned");
  const size_t span = kzg_span(3, len, stride);
  if (kzg_overlap(d_wires, span, d_z, (size_t)len * 32) || kzg_overlap(d_sigma, span, d_z, (size_t)len * 32))
    return fail(OZK_E_INVALID, "d_z overlaps d_wires or d_sigma");
  if (kzg_overlap(d_wires, span, d_total, 32) || kzg_overlap(d_sigma, span, d_total, 32) ||
      kzg_overlap(d_z, (size_t)len * 32, d_total, 32))
    return fail(OZK_E_INVALID, "d_total overlaps d_wires, d_sigma or d_z");
  if (kzg_overlap(d_wires, span, d_zero_dens, 4) || kzg_overlap(d_sigma, span, d_zero_dens, 4) ||
      kzg_overlap(d_z, (size_t)len * 32, d_zero_dens, 4) || kzg_overlap(d_total, 32, d_zero_dens, 4))
    return fail(OZK_E_INVALID, "d_zero_dens overlaps d_wires, d_sigma, d_z or d_total");
  const PlonkPermLayout L = plonk_perm_layout(len, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  PlonkPermArgs a;
  const auto omega = plonk_mont(omega_host32), beta = plonk_mont(beta_host32);
  a.omega = plonk_words(omega);
  a.beta = plonk_words(beta);
  for (int j = 0; j < 3; j++) a.bk[j] = plonk_words(mul(beta, plonk_mont(k_host96 + 32 * j)));
  a.gamma = plonk_plain(gamma_host32);
  const u32 *w = (const u32*)d_wires, *s = (const u32*)d_sigma;
  const size_t cs = (size_t)stride * 8;
  OZK_HIP(hipMemsetAsync(d_zero_dens, 0, 4, st));
  hipLaunchKernelGGL(k_plonk_pows, dim3((PLONK_WG + L.nt + 63) / 64), dim3(64), 0, st, a.omega, plonk_words(fe_one<FrP>()),
                     PLONK_WG, (unsigned)PLONK_L, 1, L.nt, (unsigned)PLONK_TILE, L.tab, L.start);
  if (L.nt > 1) {
    hipLaunchKernelGGL(k_plonk_perm_tiles, dim3(L.nt), dim3(PLONK_WG), 0, st, w, s, len, cs, a, (const u32*)L.tab,
                       (const u32*)L.start, L.agg);
    hipLaunchKernelGGL(k_plonk_perm_carries, dim3(1), dim3(PLONK_SCAN_WG), 0, st, (const u32*)L.agg, L.nt, L.carry);
  }
  hipLaunchKernelGGL(k_plonk_perm_apply, dim3(L.nt), dim3(PLONK_WG), 0, st, w, s, len, cs, L.nt, a, (const u32*)L.tab,
                     (const u32*)L.start, (const u32*)(L.nt > 1 ? L.carry : nullptr), (u32*)d_z, (u32*)d_total,
                     (int*)d_zero_dens);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

int ozk_plonk_quotient_dev(const void* d_wit, int64_t wit_stride, const void* d_key, int64_t key_stride, int32_t n,
                           const uint8_t* alpha_host32, const uint8_t* beta_host32, const uint8_t* gamma_host32,
                           const uint8_t* k_host96, const uint8_t* zh_inv_host128, void* d_out, void* stream) {
  hip_clear_stale();
  if (int rc = plonk_quot_shape(n, wit_stride, key_stride)) return rc;
  if (int rc = fr_check_pointers(d_wit, d_key, alpha_host32, beta_host32, gamma_host32, k_host96, zh_inv_host128, d_out))
    return rc;
  if (int rc = plonk_quot_buffers(d_wit, PLONK_WIT_ROWS, wit_stride, d_key, PLONK_KEY_ROWS, key_stride, n, d_out)) return rc;
  const int n4 = 4 * n;
  const PlonkQuotArgs q = plonk_quot_args(alpha_host32, beta_host32, gamma_host32, k_host96, zh_inv_host128);
  hipLaunchKernelGGL(k_plonk_quotient, dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const u32*)d_wit,
                     (size_t)wit_stride * 8, (const u32*)d_key, (size_t)key_stride * 8, (unsigned)n4, q, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
