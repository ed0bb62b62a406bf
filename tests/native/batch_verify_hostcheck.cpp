// TEST INFRASTRUCTURE: compiles the batch-verification arithmetic (batch_verify.cuh) for the HOST with g++, so the
// well-formedness rule (the subgroup check among it), the GT exponentiation, the Miller-value product and the Fr
// combination are checked against tests/batch_verify_ref.py without a GPU.  Not linked into the product library.
//
// Fq12 values cross this interface as 96 words (the GT wire order, little-endian canonical); points as wire-out
// records (16 words per Fq value); Fr values and exponents as 8 words.
#include "../../octopuszk_amd/csrc/batch_verify.cuh"
#include <string.h>
#include <vector>
using namespace ozk;

extern "C" {

// one 768-byte proof record -> the device's flag
int bv_proof_flag(const u32* rec) { return bv_proof_wellformed(rec); }
// one wire-out G2 point (96 words) -> canonical, on the twist, Z != 0 and [r]Q = O
int bv_g2_flag(const u32* q) { return bv_g2_wellformed(q) ? 1 : 0; }
// one wire-out G1 point (48 words) -> canonical, on the curve, Z != 0
int bv_g1_flag(const u32* p) { return bv_g1_wellformed(p) ? 1 : 0; }
// a^e, a a GT value (wire), e 8 words
void bv_gt_pow(const u32* a, const u32* e, u32* out) { f12_to_wire(gt_pow(f12_from_wire(a), e, 8), out); }
// the product of n Fq12 values (wire, 96 words each) as the device's tree takes it: chunks of `chunk`, level by level
void bv_prod(int n, int chunk, const u32* in, u32* out) {
  std::vector<u32> a((size_t)n * FE12_WORDS), b;
  for (int i = 0; i < n; i++) store_f12(f12_from_wire(in + 96L * i), a.data() + i, n);
  while (n > 1) {
    const int m = (n + chunk - 1) / chunk;
    b.assign((size_t)m * FE12_WORDS, 0);
    for (int i = 0; i < m; i++) {
      const long lo = (long)i * chunk, hi = lo + chunk < n ? lo + chunk : n;
      store_f12(f12_prod_range(a.data(), n, lo, hi), b.data() + i, m);
    }
    a.swap(b);
    n = m;
  }
  f12_to_wire(load_f12(a.data(), 1), out);
}
// k_rlc_combine's arithmetic: lanes lanes stride over the k rows, then a tree of pairwise sums.  x k x n x 8 words,
// r k x 8 words, use k flags; out n x 8 words (s_j) then 8 words (S).
void bv_combine(int k, int n, int lanes, const u32* x, const u32* r, const int* use, u32* out) {
  std::vector<u32> part((size_t)lanes * 8);
  for (int j = 0; j < n; j++) {
    for (int t = 0; t < lanes; t++) {
      BvFr acc = BvFr(fe_zero<FrParams>());
      for (int i = t; i < k; i += lanes)
        if (use[i]) acc = bv_fr_add(acc, bv_fr_term(x + (8L * n) * i + 8L * j, r + 8L * i));
      bv_fr_store(acc, part.data() + 8 * t);
    }
    for (int h = lanes / 2; h > 0; h >>= 1)
      for (int t = 0; t < h; t++)
        bv_fr_store(bv_fr_add(bv_fr_load(part.data() + 8 * t), bv_fr_load(part.data() + 8 * (t + h))),
                    part.data() + 8 * t);
    memcpy(out + 8L * j, part.data(), 32);
  }
  std::vector<BvSum> s(lanes, BvSum{{0, 0, 0}});
  for (int t = 0; t < lanes; t++)
    for (int i = t; i < k; i += lanes)
      if (use[i]) bv_sum_add(s[t], r + 8L * i);
  for (int h = lanes / 2; h > 0; h >>= 1)
    for (int t = 0; t < h; t++) bv_sum_merge(s[t], s[t + h]);
  for (int w = 0; w < 8; w++) out[8L * n + w] = w < 6 ? (u32)(s[0].w[w >> 1] >> (32 * (w & 1))) : 0u;
}
// r P as the affine point miller() takes (canonical x, y), P wire-out G1, r 4 words
void bv_g1_mul(const u32* p, const u32* r, u32* out) {
  BvFq x, y;
  bv_g1_mul_affine(p, r, 4, x, y);
  u32 w[8];
  from_mont(x, w);
  memcpy(out, w, 32);
  from_mont(y, w);
  memcpy(out + 8, w, 32);
}

}  // extern "C"
