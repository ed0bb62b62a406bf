// The field side of the batched PLONK verifier: for K proofs under one verifying key, the
// Fiat-Shamir transcripts and the per-proof arithmetic that plonk.verify runs in host integers, one proof per lane.
// A section of the plonk.hip unit, which alone includes it: kernels, layouts and entry points.  It uses the element
// I/O of fr_tables.cuh, the chunked inversion and entry checks of fr_rows.cuh and the lane's SHA-256 of sha256.cuh.
//
// Conventions are the PLONK block's: every value in HBM is 32 bytes LE, plain; outputs are canonical.  kind 0 is a
// vanilla proof (800 bytes under a key of 264), kind 1 a proof with lookups (1088 bytes under a key of 392).
//
// Challenges.  One lane per proof hashes six (vanilla) or eight (lookup) messages and its half of one block of the
// weight stream.  The lane's 64-byte block buffer lies in LDS, the lanes 17 words apart; the multi-opening's message
// (K | per row: t, points, C, values; 1651 bytes for a vanilla proof) is absorbed piece by piece from z, z omega, the
// proof, the key and the values where they lie: it never exists in memory.
//   per proof: 41 (vanilla) or 57 (lookup) compressions at n_public = 0, one product (z omega).
//
// Scalars.  Three launches.  (1) The public-input term, one wave per proof: lane l takes the inputs j = l, l + 64, ..,
// inverts its denominators n (z - omega^j) eight at a time (kzg_chunk_inverses) and the wave's sums meet in a tree in
// LDS: PI(z) = -sum_j x_j L_j(z), and L_1(z) from lane 0.  (2) One proof per lane: the range checks, z^n, the identity
// on the opened values, then the scalars of kzg._multi_terms for the fixed shape of verify's MultiOpening (NSINGLE
// rows at {z}, NTWO rows at {z, z omega}: one inversion, of z omega - z), each times rho_m.  What a proof adds to the
// scalars of the key's commitments and of g1 goes to the workspace, column-major.  (3) One workgroup per column adds
// them: every lane its own fixed stride of proofs, then the tree of fr_block_sum.  No atomics touch field data, so the
// output is the same bytes from run to run.
//   per proof: a few hundred products, z^n, one inversion; per public input 5 products and an eighth of an
//   inversion.
#pragma once
#include "fr_rows.cuh"
#include "sha256.cuh"

namespace ozk {

constexpr int PLONK_VF_WG = 64;                    // lanes of a workgroup: one wave
constexpr int PLONK_VF_K_MAX = 1 << 16;            // proofs of one call
constexpr long long PLONK_VF_ROWS_MAX = 1ll << 24; // K (n_public + 1)
constexpr int PLONK_VF_SUM_WG = 256;               // fr_block_sum's workgroup

// the shape of one kind of proof, of its key and of the MultiOpening that verify builds from them
template <int KIND>
struct PlonkVf;
template <>
struct PlonkVf<0> {
  static constexpr int NABC = 3, NZS = 1;          // [a] [b] [c] | [Z] | [t_lo] [t_mid] [t_hi]
  static constexpr int NC = NABC + NZS + 3, NV = 16, NKEY = 8;
  static constexpr int NSINGLE = 14, NTWO = 1;     // rows opened at {z}, rows opened at {z, z omega}
  static constexpr int REC = 8, Z_AT = 3;          // scalars of a challenge record; where z lies in it
};
template <>
struct PlonkVf<1> {
  static constexpr int NABC = 4, NZS = 2;          // [a] [b] [c] [m] | [Z] [S] | [t_lo] [t_mid] [t_hi]
  static constexpr int NC = NABC + NZS + 3, NV = 23, NKEY = 12;
  static constexpr int NSINGLE = 19, NTWO = 2;
  static constexpr int REC = 12, Z_AT = 5;
};
template <int KIND>
struct PlonkVfShape : PlonkVf<KIND> {
  using S = PlonkVf<KIND>;
  static constexpr int NPS = S::NABC + 3;                          // the proof's own rows among the single ones
  static constexpr int PROOF_WORDS = 8 * (S::NC + S::NV + 2), VK_WORDS = 2 + 8 * S::NKEY;
  static constexpr int OUT = S::NC + 2;                            // scalars a proof owns: its commitments, W, W'
  static_assert(NPS + S::NKEY == S::NSINGLE && S::NABC + 3 + S::NZS == S::NC && S::NZS == S::NTWO, "the rows of verify");
  static_assert(S::NSINGLE + 2 * S::NTWO == S::NV, "one value per point");
};

#if defined(__HIPCC__)
struct PlonkVfSeed {
  u32 w[8];
};
struct PlonkVfArgs {
  FrArg omega, n, k1, k2;   // Montgomery form: the domain's generator, n, the cosets of the columns b and c
  unsigned n_pow;           // the exponent of z^n: n itself
  int n_public, K;
};

template <int N>
__device__ __forceinline__ void vf_tag(Sha256& H, const char (&s)[N]) {
#pragma unroll
  for (int i = 0; i < N - 1; i++) H.absorb_byte((u32)(unsigned char)s[i]);
}
__device__ __forceinline__ void vf_absorb8(Sha256& H, const u32 (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) H.absorb_be32(sha256_bswap(w[i]));
}
__device__ __forceinline__ void vf_absorb_u64(Sha256& H, u32 v) {   // v as 8 bytes little-endian
  H.absorb_be32(sha256_bswap(v));
  H.absorb_be32(0);
}
// half `half` of a digest as a challenge: its 16 bytes little-endian, 1 if they are zero; written to dst and returned
__device__ __forceinline__ void vf_challenge(const u32 (&d)[8], int half, u32* dst, u32 (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = sha256_bswap(half ? d[4 + j] : d[j]);
#pragma unroll
  for (int j = 4; j < 8; j++) w[j] = 0;
  if ((w[0] | w[1] | w[2] | w[3]) == 0) w[0] = 1;
  fr_store_words(w, dst);
}

// ---- challenges: one lane per proof
template <int KIND>
__global__ void __launch_bounds__(PLONK_VF_WG) k_plonk_vf_challenges(const u32* __restrict__ vk, const u32* __restrict__ proofs,
                                                                    const u32* __restrict__ pub, int n_public, int K,
                                                                    FrArg omega, PlonkVfSeed seed, u32* __restrict__ out) {
  using S = PlonkVfShape<KIND>;
  __shared__ u32 blocks[PLONK_VF_WG * SHA256_LDS_STRIDE];
  const int m = blockIdx.x * PLONK_VF_WG + threadIdx.x;
  if (m >= K) return;
  u32* buf = blocks + threadIdx.x * SHA256_LDS_STRIDE;
  const u32* C = proofs + (size_t)m * S::PROOF_WORDS;
  const u32* Y = C + 8 * S::NC;
  const u32* W = Y + 8 * S::NV;
  const u32* T = C + 8 * (S::NABC + S::NZS);
  u32* rec = out + (size_t)m * 8 * S::REC;
  Sha256 H;
  u32 d1[8], d2[8], d[8], w[8], z[8];
  int at = 0;

  H.init(buf);
  if (KIND == 0) vf_tag(H, "OZK-plonk-beta");
  else vf_tag(H, "OZK-plookup-beta");
  H.absorb_le_words(vk, S::VK_WORDS);
  if (n_public > 0) H.absorb_le_words(pub + (size_t)m * 8 * n_public, 8 * n_public);
  H.absorb_le_words(C, 8 * S::NABC);
  H.finish(d1);
  vf_challenge(d1, 0, rec + 8 * at++, w);

  H.init(buf);
  if (KIND == 0) vf_tag(H, "OZK-plonk-gamma");
  else vf_tag(H, "OZK-plookup-gamma");
  H.absorb_digest(d1);
  H.finish(d);
  vf_challenge(d, 0, rec + 8 * at++, w);
  if (KIND == 1) {
    H.init(buf);
    vf_tag(H, "OZK-plookup-eta");
    H.absorb_digest(d1);
    H.finish(d);
    vf_challenge(d, 0, rec + 8 * at++, w);
    H.init(buf);
    vf_tag(H, "OZK-plookup-theta");
    H.absorb_digest(d1);
    H.finish(d);
    vf_challenge(d, 0, rec + 8 * at++, w);
  }

  H.init(buf);
  if (KIND == 0) vf_tag(H, "OZK-plonk-alpha");
  else vf_tag(H, "OZK-plookup-alpha");
  H.absorb_digest(d1);
  H.absorb_le_words(C + 8 * S::NABC, 8 * S::NZS);
  H.finish(d2);
  vf_challenge(d2, 0, rec + 8 * at++, w);

  H.init(buf);
  if (KIND == 0) vf_tag(H, "OZK-plonk-z");
  else vf_tag(H, "OZK-plookup-z");
  H.absorb_digest(d2);
  H.absorb_le_words(T, 24);
  H.finish(d);
  vf_challenge(d, 0, rec + 8 * at++, z);

  // z omega, canonical: a plain z times omega in Montgomery form is plain
  u32 zw[8];
  pack(canonical(mul(unpack<FrP, 16>(z), plonk_arg(omega))), zw);

  // the multi-opening's gamma: K | per row: t, its points, C, its values
  H.init(buf);
  vf_tag(H, "OZK-kzg-multi-gamma");
  vf_absorb_u64(H, S::NSINGLE + S::NTWO);
#pragma unroll 1
  for (int i = 0; i < S::NSINGLE; i++) {
    const u32* c = i < S::NABC ? C + 8 * i : i < S::NPS ? T + 8 * (i - S::NABC) : vk + 2 + 8 * (i - S::NPS);
    vf_absorb_u64(H, 1);
    vf_absorb8(H, z);
    H.absorb_le_words(c, 8);
    H.absorb_le_words(Y + 8 * i, 8);
  }
#pragma unroll 1
  for (int t = 0; t < S::NTWO; t++) {
    vf_absorb_u64(H, 2);
    vf_absorb8(H, z);
    vf_absorb8(H, zw);
    H.absorb_le_words(C + 8 * (S::NABC + t), 8);
    H.absorb_le_words(Y + 8 * (S::NSINGLE + 2 * t), 16);
  }
  H.finish(d1);
  vf_challenge(d1, 0, rec + 8 * at++, w);

  H.init(buf);
  vf_tag(H, "OZK-kzg-multi-z");
  H.absorb_digest(d1);
  H.absorb_le_words(W, 8);
  H.finish(d);
  vf_challenge(d, 0, rec + 8 * at++, w);

  // rho_m: half m % 2 of block m / 2 of the weight stream
  H.init(buf);
  vf_tag(H, "OZK-plonk-rho");
  vf_absorb8(H, seed.w);
  vf_absorb_u64(H, (u32)m >> 1);
  H.finish(d);
  vf_challenge(d, m & 1, rec + 8 * at++, w);

  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (; at < S::REC; at++) fr_store_words(zero, rec + 8 * at);
}

// ---- scalars
using VfV = KzgV;
template <class A, class B>
__device__ __forceinline__ VfV vf_mul(const A& a, const B& b) { return VfV(mul(a, b)); }
template <class A, class B>
__device__ __forceinline__ VfV vf_add(const A& a, const B& b) { return VfV(reduce_to<32>(add(a, b))); }
template <class A, class B>
__device__ __forceinline__ VfV vf_sub(const A& a, const B& b) { return VfV(reduce_to<32>(sub(a, b))); }
// 32 bytes of any value -> Montgomery form
__device__ __forceinline__ VfV vf_mont(const u32* src) { return VfV(mul(fr_load<85>(src), fe_const<FrP, 16>(FrP::R2))); }
// whether the 256-bit word at src is >= r
__device__ __forceinline__ bool vf_ge_r(const u32* src) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  const uint4 a = s[0], b = s[1];
  const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  bool ge = true;   // equal so far, from the bottom: the highest differing word decides
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (w[i] != FrP::P32[i]) ge = w[i] > FrP::P32[i];
  }
  return ge;
}
__device__ __forceinline__ void vf_store_zero(u32* dst) {
  const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  fr_store_words(zero, dst);
}

// (1) PI(z) and L_1(z) of proof blockIdx.x, plain and canonical, to pi[16 m ..]; pi_flag[m] = 2 when a public input
// is >= r.  Both elements are zero when z^n = 1: nothing is inverted then.
template <int KIND>
__global__ void __launch_bounds__(PLONK_VF_WG) k_plonk_vf_pi(const u32* __restrict__ pub, const u32* __restrict__ chal,
                                                            PlonkVfArgs a, u32* __restrict__ pi, int* __restrict__ pi_flag) {
  using S = PlonkVfShape<KIND>;
  __shared__ u32 part[9 * PLONK_VF_WG];
  const int m = blockIdx.x, l = threadIdx.x;
  const int np = a.n_public, count = np > 0 ? np : 1;
  const u32* x = pub + (size_t)m * 8 * np;
  int bad = 0;
  for (int j = l; j < np; j += PLONK_VF_WG) bad |= vf_ge_r(x + (size_t)j * 8) ? 1 : 0;
  bad = __syncthreads_or(bad);

  const VfV z = vf_mont(chal + ((size_t)m * S::REC + S::Z_AT) * 8);
  const VfV zh = vf_sub(fe_pow_u32(z, a.n_pow), fe_one<FrP>());
  const bool in_domain = is_zero(zh);
  VfV acc = VfV(fe_zero<FrP>()), l1 = VfV(fe_zero<FrP>());
  if (!in_domain) {
    const auto omega = plonk_arg(a.omega), n_mont = plonk_arg(a.n);
    VfV wcur = fe_pow_u32(omega, (unsigned)l);
    const VfV w64 = fe_pow_u32(omega, (unsigned)PLONK_VF_WG);
    for (int base = l; base < count; base += PLONK_VF_WG * KZG_INV_BATCH) {
      VfV den[KZG_INV_BATCH], wj[KZG_INV_BATCH], di[KZG_INV_BATCH];
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < KZG_INV_BATCH; k++) {
        const int j = base + k * PLONK_VF_WG;
        wj[k] = wcur;
        den[k] = VfV(fe_one<FrP>());
        if (j < count) {
          den[k] = vf_mul(vf_sub(z, wcur), n_mont);
          wcur = vf_mul(wcur, w64);
          cnt = k + 1;
        }
      }
      kzg_chunk_inverses<KZG_INV_BATCH>(den, cnt, di);
#pragma unroll
      for (int k = 0; k < KZG_INV_BATCH; k++) {
        const int j = base + k * PLONK_VF_WG;
        if (j >= count) continue;
        if (j == 0) l1 = vf_mul(zh, di[k]);
        // x_j omega^j / (n (z - omega^j)), plain: a plain x_j times two factors in Montgomery form
        if (j < np) acc = vf_add(acc, mul(mul(fr_load<85>(x + (size_t)j * 8), wj[k]), di[k]));
      }
    }
  }
  // the wave's sum: a tree over the lanes' partials (limb-major in LDS)
#pragma unroll
  for (int i = 0; i < 9; i++) part[i * PLONK_VF_WG + l] = acc.l[i];
  block_sync();
  for (int o = PLONK_VF_WG / 2; o > 0; o >>= 1) {
    if (l < o) {
      VfV p, q;
#pragma unroll
      for (int i = 0; i < 9; i++) {
        p.l[i] = part[i * PLONK_VF_WG + l];
        q.l[i] = part[i * PLONK_VF_WG + l + o];
      }
      const VfV s = vf_add(p, q);
#pragma unroll
      for (int i = 0; i < 9; i++) part[i * PLONK_VF_WG + l] = s.l[i];
    }
    block_sync();
  }
  if (l == 0) {
    VfV sum;
#pragma unroll
    for (int i = 0; i < 9; i++) sum.l[i] = part[i * PLONK_VF_WG];
    u32* dst = pi + (size_t)m * 16;
    fr_store(canonical(neg(mul(sum, zh))), dst);      // -(zn - 1) sum_j ..: plain
    u32 o[8];
    from_mont(l1, o);
    fr_store_words(o, dst + 8);
    pi_flag[m] = bad ? 2 : 0;
  }
}

// (2) one proof per lane
template <int KIND>
__global__ void __launch_bounds__(PLONK_VF_WG) k_plonk_vf_scalars(const u32* __restrict__ proofs, const u32* __restrict__ chal,
                                                                 const u32* __restrict__ pi, const int* __restrict__ pi_flag,
                                                                 PlonkVfArgs a, u32* __restrict__ scalars,
                                                                 u32* __restrict__ rho_out, int* __restrict__ flags,
                                                                 u32* __restrict__ contrib) {
  using S = PlonkVfShape<KIND>;
  const int m = blockIdx.x * PLONK_VF_WG + threadIdx.x, K = a.K;
  if (m >= K) return;
  const u32* Y = proofs + (size_t)m * S::PROOF_WORDS + 8 * S::NC;
  const u32* ch = chal + (size_t)m * 8 * S::REC;
  u32* own = scalars + (size_t)m * S::NC * 8;                      // the proof's commitments
  u32* s_w = scalars + ((size_t)K * S::NC + m) * 8;                // W
  u32* s_w2 = scalars + ((size_t)K * (S::NC + 1) + m) * 8;         // W'
  auto val = [&](int i) { return vf_mont(Y + 8 * i); };

  int flag = pi_flag[m];
  for (int i = 0; i < S::NV; i++) flag |= vf_ge_r(Y + 8 * i) ? 1 : 0;
  const VfV beta = vf_mont(ch), gamma = vf_mont(ch + 8);
  const VfV alpha = vf_mont(ch + 8 * (S::Z_AT - 1)), z = vf_mont(ch + 8 * S::Z_AT);
  const VfV zn = fe_pow_u32(z, a.n_pow);
  const VfV zh = vf_sub(zn, fe_one<FrP>());
  if (is_zero(zh)) flag |= 4;

  if (flag == 0) {
    // gate + alpha P1 + alpha^2 (Z - 1) L_1 [+ alpha^3 L1 + alpha^4 S L_1] - t Z_H, Montgomery form throughout
    constexpr int T0 = S::NABC, Q0 = T0 + 3, S0 = Q0 + 5, ZZ = S::NSINGLE;
    const VfV va = val(0), vb = val(1), vc = val(2);
    const VfV pi_z = vf_mont(pi + (size_t)m * 16), l1 = vf_mont(pi + (size_t)m * 16 + 8);
    VfV sum = vf_add(vf_add(vf_mul(val(Q0), va), vf_mul(val(Q0 + 1), vb)),
                     vf_add(vf_mul(val(Q0 + 2), vc), vf_mul(vf_mul(val(Q0 + 3), va), vb)));
    sum = vf_add(sum, vf_add(val(Q0 + 4), pi_z));
    const VfV ag = vf_add(va, gamma), bg = vf_add(vb, gamma), cg = vf_add(vc, gamma);
    const VfV bz = vf_mul(beta, z);
    const VfV zz = val(ZZ);
    const VfV left = vf_mul(vf_mul(vf_mul(zz, vf_add(ag, bz)), vf_add(bg, vf_mul(bz, plonk_arg(a.k1)))),
                            vf_add(cg, vf_mul(bz, plonk_arg(a.k2))));
    const VfV right = vf_mul(vf_mul(vf_mul(val(ZZ + 1), vf_add(ag, vf_mul(beta, val(S0)))),
                                    vf_add(bg, vf_mul(beta, val(S0 + 1)))),
                             vf_add(cg, vf_mul(beta, val(S0 + 2))));
    const VfV a2 = vf_mul(alpha, alpha);
    sum = vf_add(sum, vf_mul(alpha, vf_sub(left, right)));
    sum = vf_add(sum, vf_mul(a2, vf_mul(vf_sub(zz, fe_one<FrP>()), l1)));
    if (KIND == 1) {
      const VfV eta = vf_mont(ch + 16), theta = vf_mont(ch + 24);
      const VfV e2 = vf_mul(eta, eta);
      const VfV df = vf_add(vf_add(theta, va), vf_add(vf_mul(eta, vb), vf_mul(e2, vc)));
      const VfV dt = vf_add(vf_add(theta, val(S0 + 4)), vf_add(vf_mul(eta, val(S0 + 5)), vf_mul(e2, val(S0 + 6))));
      const VfV ss = val(ZZ + 2);
      const VfV lk = vf_add(vf_sub(vf_mul(vf_mul(vf_sub(val(ZZ + 3), ss), dt), df), vf_mul(val(3), df)),
                            vf_mul(val(S0 + 3), dt));
      const VfV a3 = vf_mul(a2, alpha);
      sum = vf_add(sum, vf_mul(a3, lk));
      sum = vf_add(sum, vf_mul(vf_mul(a3, alpha), vf_mul(ss, l1)));
    }
    const VfV t = vf_add(val(T0), vf_mul(zn, vf_add(val(T0 + 1), vf_mul(zn, val(T0 + 2)))));
    sum = vf_sub(sum, vf_mul(t, zh));
    if (!is_zero(sum)) flag |= 8;
  }
  flags[m] = flag;

  if (flag != 0) {
    for (int i = 0; i < S::NC; i++) vf_store_zero(own + 8 * i);
    vf_store_zero(s_w);
    vf_store_zero(s_w2);
    vf_store_zero(rho_out + (size_t)m * 8);
    for (int c = 0; c <= S::NKEY; c++) vf_store_zero(contrib + ((size_t)c * K + m) * 8);
    return;
  }

  // kzg._multi_terms for NSINGLE rows at {z} and NTWO rows at {z, z omega}, at the multi-opening's point u:
  //   the union of the sets is {z, z omega}, so c = u - z omega for a row at {z} and 1 for a row at both;
  //   weight_i = g^i c_i; at = sum_i weight_i r_i(u), r_i = y_i or y_i0 + (y_i1 - y_i0)(u - z) / (z omega - z);
  //   the scalars are weight_i of C_i, -at of g1, -(u - z)(u - z omega) of W and u of W'.
  const auto rho = canonical(fr_load<85>(ch + 8 * (S::Z_AT + 3)));   // plain: a Montgomery form times it is plain
  const VfV g = vf_mont(ch + 8 * (S::Z_AT + 1)), u = vf_mont(ch + 8 * (S::Z_AT + 2));
  const VfV zw = vf_mul(z, plonk_arg(a.omega));
  const VfV c0 = vf_sub(u, zw), uz = vf_sub(u, z);
  const VfV slope = vf_mul(uz, inv(vf_sub(zw, z)));
  VfV gp = VfV(fe_one<FrP>()), at_u = VfV(fe_zero<FrP>());
#pragma unroll 1
  for (int i = 0; i < S::NSINGLE; i++) {
    const VfV w = vf_mul(gp, c0);
    at_u = vf_add(at_u, vf_mul(w, val(i)));
    u32* dst = i < S::NPS ? own + 8 * i : contrib + ((size_t)(i - S::NPS) * K + m) * 8;
    fr_store(canonical(mul(w, rho)), dst);
    gp = vf_mul(gp, g);
  }
#pragma unroll 1
  for (int t = 0; t < S::NTWO; t++) {
    const VfV y0 = val(S::NSINGLE + 2 * t), y1 = val(S::NSINGLE + 2 * t + 1);
    at_u = vf_add(at_u, vf_mul(gp, vf_add(y0, vf_mul(vf_sub(y1, y0), slope))));
    fr_store(canonical(mul(gp, rho)), own + 8 * (S::NPS + t));
    gp = vf_mul(gp, g);
  }
  fr_store(canonical(mul(neg(at_u), rho)), contrib + ((size_t)S::NKEY * K + m) * 8);
  fr_store(canonical(mul(neg(vf_mul(uz, c0)), rho)), s_w);
  fr_store(canonical(mul(u, rho)), s_w2);
  fr_store(rho, rho_out + (size_t)m * 8);
}

// (3) column blockIdx.x of the K x (NKEY + 1) contributions -> out[blockIdx.x]
__global__ void __launch_bounds__(PLONK_VF_SUM_WG) k_plonk_vf_sums(const u32* __restrict__ contrib, int K, u32* __restrict__ out) {
  __shared__ u32 part[9 * PLONK_VF_SUM_WG];
  const u32* col = contrib + (size_t)blockIdx.x * K * 8;
  FrAcc acc = FrAcc(fe_zero<FrP>());
  for (int i = threadIdx.x; i < K; i += PLONK_VF_SUM_WG) acc = FrAcc(reduce_to<32>(add(acc, fr_load<16>(col + (size_t)i * 8))));
  const FrAcc sum = fr_block_sum(acc, part);
  if (threadIdx.x == 0) fr_store(canonical(sum), out + (size_t)blockIdx.x * 8);
}

// ---- host side ----
// A primitive 2^28-th root of unity of Fr, plain: FR_ROOT^((r - 1) / 2^28), so that the domain of n = 2^k points has
// the generator W28^(2^28 / n) (fft.root_of_unity)
static const u32 PLONK_VF_W28[8] = {0x88590882u, 0xb8dde849u, 0x0e1a5d5du, 0x67cf5acdu,
                                    0x723d5c5fu, 0xe1ed0cc8u, 0xc8953178u, 0x188c51b4u};
static FrArg plonk_vf_omega(int n) {
  Fe<FrP, 32> w = Fe<FrP, 32>(to_mont<FrP>(PLONK_VF_W28));
  for (long long k = n; k < (1ll << 28); k <<= 1) w = Fe<FrP, 32>(sqr(w));
  return plonk_words(w);
}
static FrArg plonk_vf_small(u32 v) {
  u32 w[8] = {v, 0, 0, 0, 0, 0, 0, 0};
  return plonk_words(to_mont<FrP>(w));
}
static int plonk_vf_shape(int kind, int n, int n_public, int K) {
  if (kind != 0 && kind != 1) return fail(OZK_E_INVALID, "kind = %d: 0 is a vanilla proof, 1 a proof with lookups", kind);
  if (n < 2 || (n & (n - 1)) || n > (1 << 26)) return fail(OZK_E_INVALID, "n = %d is not a power of two in [2, 2^26]", n);
  if (n_public < 0 || n_public > n) return fail(OZK_E_INVALID, "n_public = %d, not in [0, n = %d]", n_public, n);
  if (K < 1 || K > PLONK_VF_K_MAX) return fail(OZK_E_INVALID, "K = %d proofs: 1 <= K <= 2^16", K);
  if ((long long)K * (n_public + 1) > PLONK_VF_ROWS_MAX)
    return fail(OZK_E_INVALID, "K (n_public + 1) = %lld: at most 2^24", (long long)K * (n_public + 1));
  return OZK_OK;
}
struct PlonkVfLayout {
  u32* pi;
  int* pi_flag;
  u32* contrib;
  size_t bytes;
};
static PlonkVfLayout plonk_vf_layout(int kind, int K, void* wsp) {
  PlonkVfLayout L;
  Bump b(wsp, ~(size_t)0);
  L.pi = b.take<u32>((size_t)K * 16);
  L.pi_flag = b.take<int>((size_t)K);
  L.contrib = b.take<u32>((size_t)K * 8 * ((kind ? PlonkVf<1>::NKEY : PlonkVf<0>::NKEY) + 1));
  b.take<u32>(64);
  L.bytes = b.off;
  return L;
}
static size_t plonk_vf_proof_bytes(int kind) { return 4 * (size_t)(kind ? PlonkVfShape<1>::PROOF_WORDS : PlonkVfShape<0>::PROOF_WORDS); }
static size_t plonk_vf_scalars_bytes(int kind, int K) {
  return kind ? ((size_t)K * PlonkVfShape<1>::OUT + PlonkVf<1>::NKEY + 1) * 32
              : ((size_t)K * PlonkVfShape<0>::OUT + PlonkVf<0>::NKEY + 1) * 32;
}
#endif  // __HIPCC__

}  // namespace ozk

#if defined(__HIPCC__)
using namespace ozk;

extern "C" {

int ozk_plonk_verify_challenges_dev(int32_t kind, const void* d_vk_bytes, int32_t n, int32_t n_public, const void* d_proofs,
                                    const void* d_public, int32_t K, const uint8_t* seed_host32, void* d_out, void* stream) {
  hip_clear_stale();
  if (int rc = plonk_vf_shape(kind, n, n_public, K)) return rc;
  if (int rc = fr_check_pointers(d_vk_bytes, d_proofs, seed_host32, d_out)) return rc;
  if (n_public > 0 && !d_public) return fail(OZK_E_INVALID, "null pointer argument");
  if (int rc = fr_check_aligned16(d_vk_bytes, d_proofs, d_out)) return rc;
  if (n_public > 0 && kzg_misaligned16(d_public)) return fail(OZK_E_INVALID, "elements must be 16-byte aligned");
  const size_t rec = (size_t)K * 32 * (kind ? PlonkVf<1>::REC : PlonkVf<0>::REC);
  if (kzg_overlap(d_out, rec, d_proofs, (size_t)K * plonk_vf_proof_bytes(kind)) ||
      (n_public > 0 && kzg_overlap(d_out, rec, d_public, (size_t)K * n_public * 32)) ||
      kzg_overlap(d_out, rec, d_vk_bytes, kind ? 392 : 264))
    return fail(OZK_E_INVALID, "d_out overlaps an input");
  PlonkVfSeed seed;
  memcpy(seed.w, seed_host32, 32);
  const FrArg omega = plonk_vf_omega(n);
  const dim3 grid((K + PLONK_VF_WG - 1) / PLONK_VF_WG), wg(PLONK_VF_WG);
  hipStream_t st = (hipStream_t)stream;
  if (kind)
    hipLaunchKernelGGL(k_plonk_vf_challenges<1>, grid, wg, 0, st, (const u32*)d_vk_bytes, (const u32*)d_proofs,
                       (const u32*)d_public, n_public, K, omega, seed, (u32*)d_out);
  else
    hipLaunchKernelGGL(k_plonk_vf_challenges<0>, grid, wg, 0, st, (const u32*)d_vk_bytes, (const u32*)d_proofs,
                       (const u32*)d_public, n_public, K, omega, seed, (u32*)d_out);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

size_t ozk_plonk_verify_scalars_workspace_bytes(int32_t kind, int32_t K) {
  if ((kind != 0 && kind != 1) || K < 1 || K > PLONK_VF_K_MAX) return 0;
  return plonk_vf_layout(kind, K, nullptr).bytes;
}

int ozk_plonk_verify_scalars_dev(int32_t kind, int32_t n, int32_t n_public, const void* d_proofs, const void* d_public,
                                 const void* d_challenges, int32_t K, void* d_scalars, void* d_rho, int32_t* d_flags,
                                 void* d_workspace, size_t workspace_bytes, void* stream) {
  hip_clear_stale();
  if (int rc = plonk_vf_shape(kind, n, n_public, K)) return rc;
  if (int rc = fr_check_pointers(d_proofs, d_challenges, d_scalars, d_rho, d_flags, d_workspace)) return rc;
  if (n_public > 0 && !d_public) return fail(OZK_E_INVALID, "null pointer argument");
  if (int rc = fr_check_aligned16(d_proofs, d_challenges, d_scalars, d_rho, d_workspace)) return rc;
  if (n_public > 0 && kzg_misaligned16(d_public)) return fail(OZK_E_INVALID, "elements must be 16-byte aligned");
  if (((uintptr_t)d_flags & 3) != 0) return fail(OZK_E_INVALID, "d_flags must be 4-byte aligned");
  const PlonkVfLayout L = plonk_vf_layout(kind, K, d_workspace);
  if (int rc = fr_check_workspace(L.bytes, workspace_bytes)) return rc;
  const size_t sc = plonk_vf_scalars_bytes(kind, K), rec = (size_t)K * 32 * (kind ? PlonkVf<1>::REC : PlonkVf<0>::REC);
  const void* outs[4] = {d_scalars, d_rho, d_flags, d_workspace};
  const size_t out_bytes[4] = {sc, (size_t)K * 32, (size_t)K * 4, L.bytes};
  for (int i = 0; i < 4; i++) {
    if (kzg_overlap(outs[i], out_bytes[i], d_proofs, (size_t)K * plonk_vf_proof_bytes(kind)) ||
        kzg_overlap(outs[i], out_bytes[i], d_challenges, rec) ||
        (n_public > 0 && kzg_overlap(outs[i], out_bytes[i], d_public, (size_t)K * n_public * 32)))
      return fail(OZK_E_INVALID, "an output or the workspace overlaps an input");
    for (int j = i + 1; j < 4; j++)
      if (kzg_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j]))
        return fail(OZK_E_INVALID, "d_scalars, d_rho, d_flags and d_workspace overlap");
  }
  PlonkVfArgs a;
  a.omega = plonk_vf_omega(n);
  a.n = plonk_vf_small((u32)n);
  a.k1 = plonk_vf_small(5);
  a.k2 = plonk_vf_small(25);
  a.n_pow = (unsigned)n;
  a.n_public = n_public;
  a.K = K;
  hipStream_t st = (hipStream_t)stream;
  const dim3 lanes((K + PLONK_VF_WG - 1) / PLONK_VF_WG), wg(PLONK_VF_WG);
  const u32 *p = (const u32*)d_proofs, *x = (const u32*)d_public, *c = (const u32*)d_challenges;
  if (kind) {
    hipLaunchKernelGGL(k_plonk_vf_pi<1>, dim3(K), wg, 0, st, x, c, a, L.pi, L.pi_flag);
    hipLaunchKernelGGL(k_plonk_vf_scalars<1>, lanes, wg, 0, st, p, c, (const u32*)L.pi, (const int*)L.pi_flag, a,
                       (u32*)d_scalars, (u32*)d_rho, (int*)d_flags, L.contrib);
  } else {
    hipLaunchKernelGGL(k_plonk_vf_pi<0>, dim3(K), wg, 0, st, x, c, a, L.pi, L.pi_flag);
    hipLaunchKernelGGL(k_plonk_vf_scalars<0>, lanes, wg, 0, st, p, c, (const u32*)L.pi, (const int*)L.pi_flag, a,
                       (u32*)d_scalars, (u32*)d_rho, (int*)d_flags, L.contrib);
  }
  const int nkey = kind ? PlonkVf<1>::NKEY : PlonkVf<0>::NKEY;
  const size_t own = (size_t)K * (kind ? PlonkVfShape<1>::OUT : PlonkVfShape<0>::OUT);
  hipLaunchKernelGGL(k_plonk_vf_sums, dim3(nkey + 1), dim3(PLONK_VF_SUM_WG), 0, st, (const u32*)L.contrib, K,
                     (u32*)d_scalars + own * 8);
  OZK_HIP(hipGetLastError());
  return OZK_OK;
}

}  // extern "C"
#endif  // __HIPCC__
