// TEST INFRASTRUCTURE: the peeled first two entries of the whole-bucket level 1 (ec.cuh xyzz_from_affine_signed,
// xyzz_add_affine2_lazy), compiled for the host and compared with the carried mixed addition xyzz_madd on the same
// points.  Stand-alone (g++ -fsanitize=address,undefined); prints one line per mismatch and exits non-zero on any.
#include "../../octopuszk_amd/csrc/ec.cuh"
#include <stdio.h>
#include <string.h>
using namespace ozk;

typedef G1Cfg CV;
typedef G1Cfg::EA EA;

static Aff<EA> aff_of(const Xyzz<CV>& a) {  // canonical affine coordinates, (0, 0) for infinity
  Aff<EA> r;
  if (is_inf(a)) {
    r.x = EA(el_zero(a.ZZ));
    r.y = EA(el_zero(a.ZZ));
    return r;
  }
  r.x = EA(canonical(mul(a.X, inv(a.ZZ))));
  r.y = EA(canonical(mul(a.Y, inv(a.ZZZ))));
  return r;
}
static bool same(const Aff<EA>& a, const Aff<EA>& b) {
  u32 wa[8], wb[8];
  from_mont(a.x, wa);
  from_mont(b.x, wb);
  if (memcmp(wa, wb, 32)) return false;
  from_mont(a.y, wa);
  from_mont(b.y, wb);
  return memcmp(wa, wb, 32) == 0;
}
static Aff<EA> negated(const Aff<EA>& q) {
  Aff<EA> r = q;
  if (!is_inf(q)) r.y = EA(reduce_to<17>(neg(q.y)));
  return r;
}

int main() {
  // k G for k = 1 .. N from the generator (1, 2), then the infinity marker
  enum { N = 12 };
  Aff<EA> pts[N + 1];
  u32 w[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  Aff<EA> g;
  g.x = to_mont<FqParams>(w);
  w[0] = 2;
  g.y = to_mont<FqParams>(w);
  Xyzz<CV> acc = xyzz_from_affine<CV>(g);
  for (int k = 0; k < N; k++) {
    pts[k] = aff_of(acc);
    acc = xyzz_madd(acc, g);
  }
  pts[N].x = EA(el_zero(g.x));
  pts[N].y = EA(el_zero(g.x));
  int bad = 0, cases = 0, doublings = 0, cancels = 0;
  for (int i = 0; i <= N; i++)
    for (int j = 0; j <= N; j++)
      for (int s = 0; s < 4; s++) {
        const bool n0 = (s & 1) != 0, n1 = (s & 2) != 0;
        // entries 0 and 1 as the kernel runs them, and three more mixed additions on top of the result
        Xyzz<CV> a = xyzz_from_affine_signed<CV>(pts[i], n0);
        a = xyzz_add_affine2_lazy(a, pts[j], n1);
        Xyzz<CV> ref = xyzz_from_affine<CV>(n0 ? negated(pts[i]) : pts[i]);
        ref = xyzz_madd(ref, n1 ? negated(pts[j]) : pts[j]);
        cases++;
        if (i == j && i < N) (n0 == n1 ? doublings : cancels)++;
        if (i == j && i < N && n0 != n1 && !is_inf(a)) {
          printf("no infinity: i %d j %d signs %d\n", i, j, s);
          bad++;
        }
        for (int t = 0; t < 4; t++) {
          if (!same(aff_of(a), aff_of(ref))) {
            printf("mismatch: i %d j %d signs %d after %d further additions\n", i, j, s, t);
            bad++;
            break;
          }
          a = xyzz_madd_lazy(a, pts[(i + t + 1) % N], (t & 1) != 0);
          ref = xyzz_madd(ref, (t & 1) ? negated(pts[(i + t + 1) % N]) : pts[(i + t + 1) % N]);
        }
      }
  printf("cases %d doublings %d cancellations %d bad %d\n", cases, doublings, cancels, bad);
  return bad ? 1 : 0;
}
