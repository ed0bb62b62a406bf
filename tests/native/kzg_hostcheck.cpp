// Host build of the per-lane pieces of the KZG opening kernels (octopuszk_amd/csrc/kzg.cuh): the
// recurrence over a lane's piece, the composition of carries and the chunk inversion, for tests/test_kzg_cpu.py.
//   g++ -std=c++17 -O2 -shared -fPIC -o _kzg_hostcheck.so kzg_hostcheck.cpp
#include "../../octopuszk_amd/csrc/kzg.cuh"
using namespace ozk;

constexpr int HC_MAX = 8;   // the longest piece these checks cut (kzg_piece is unrolled for it)

static Fe<FrP, 16> plain(const u32* w) {
  u32 t[8];
  for (int i = 0; i < 8; i++) t[i] = w[i];
  return canonical(unpack<FrP, 85>(t));
}
static Fe<FrP, 16> mont(const u32* w) {
  u32 t[8];
  for (int i = 0; i < 8; i++) t[i] = w[i];
  return canonical(to_mont<FrP>(t));
}
static void put(const KzgV& v, u32* w) {
  u32 t[8];
  pack(canonical(v), t);
  for (int i = 0; i < 8; i++) w[i] = t[i];
}

// The opening of `len` coefficients cut into pieces of `chunk` (the last one shorter), the way the tile pass does it:
// every piece's value with carry 0, the carries composed from the top, and the recurrence again from each carry.
// coeffs, z: plain words -> quot: len elements (q_j = h_{j+1}, the last one 0), value: one element.
extern "C" void kzghc_open(const u32* coeffs, int len, int chunk, const u32* z_words, u32* quot, u32* value) {
  if (len < 1 || chunk < 1 || chunk > HC_MAX) return;
  const int pieces = (len + chunk - 1) / chunk;
  Fe<FrP, 16>* p = new Fe<FrP, 16>[len];
  KzgV* h = new KzgV[len + 1];
  KzgV* a = new KzgV[pieces];
  KzgV* carry = new KzgV[pieces + 1];
  for (int i = 0; i < len; i++) p[i] = plain(coeffs + 8 * i);
  const Fe<FrP, 16> z = mont(z_words);
  const KzgV zero = KzgV(fe_zero<FrP>());
  auto size = [&](int k) { return k == pieces - 1 ? len - k * chunk : chunk; };
  for (int k = 0; k < pieces; k++) a[k] = kzg_piece<HC_MAX, false>(p + k * chunk, size(k), z, zero, nullptr);
  carry[pieces] = carry[pieces - 1] = zero;
  for (int k = pieces - 2; k >= 0; k--) {
    KzgV m = KzgV(fe_one<FrP>());   // z^(length of piece k + 1)
    for (int i = 0; i < size(k + 1); i++) m = KzgV(mul(m, z));
    carry[k] = kzg_compose(a[k + 1], m, carry[k + 1]);
  }
  for (int k = 0; k < pieces; k++) kzg_piece<HC_MAX, true>(p + k * chunk, size(k), z, carry[k], h + k * chunk);
  h[len] = zero;
  for (int j = 0; j < len; j++) put(h[j + 1], quot + 8 * j);
  put(h[0], value);
  delete[] p;
  delete[] h;
  delete[] a;
  delete[] carry;
}

// d: n <= KZG_INV_BATCH plain words -> out: their inverses mod r, 0 for 0 (plain words)
extern "C" void kzghc_inverses(const u32* d, int n, u32* out) {
  KzgV dm[KZG_INV_BATCH], r[KZG_INV_BATCH];
  for (int k = 0; k < n; k++) dm[k] = KzgV(mont(d + 8 * k));
  kzg_chunk_inverses<KZG_INV_BATCH>(dm, n, r);
  for (int k = 0; k < n; k++) {
    u32 t[8];
    from_mont(r[k], t);
    for (int i = 0; i < 8; i++) out[8 * k + i] = t[i];
  }
}

extern "C" int kzghc_tile() { return KZG_TILE; }
extern "C" int kzghc_batch() { return KZG_INV_BATCH; }
