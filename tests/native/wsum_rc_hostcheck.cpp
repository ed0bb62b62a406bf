// Stand-alone host program over octopuszk_amd/csrc/wsum_rc.h (tests/test_wsum_rc_cpu.py compiles it with g++ and
// compares its output with a Python model).
//   argv:   cb s chunk
//   stdout: "G rows cols row_parts col_parts row_slots col_slots partial_lanes reduce_lanes"
//           "R t first n"              row part t: n buckets from `first` on, stride 1, summed into row slot t
//           "C t first n stride"       column part t: n buckets from `first` on, `stride` apart, into column slot t
//           "D u col first stride n"   reduce lane u: n slots of the row (col = 0) or column (col = 1) slots
#include <stdio.h>
#include <stdlib.h>

#include "../../octopuszk_amd/csrc/wsum_rc.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int cb = atoi(argv[1]), s = atoi(argv[2]), chunk = atoi(argv[3]);
  if (cb < 1 || cb > 16 || s < 0 || s > cb || chunk < 1) return 2;
  const ozk::RcGeom g = ozk::rc_geom(cb, s, chunk);
  printf("G %d %d %d %d %d %d %d %d\n", g.rows, g.cols, g.row_parts, g.col_parts, ozk::rc_row_slots(g), ozk::rc_col_slots(g),
         ozk::rc_partial_lanes(g), ozk::rc_reduce_lanes(g));
  for (int t = 0; t < ozk::rc_partial_lanes(g); t++) {
    uint32_t first;
    int n;
    if (t < ozk::rc_row_slots(g)) {
      ozk::rc_row_part(g, t, chunk, &first, &n);
      printf("R %d %u %d\n", t, first, n);
    }
    if (t < ozk::rc_col_slots(g)) {
      ozk::rc_col_part(g, t, chunk, &first, &n);
      printf("C %d %u %d %d\n", t, first, n, g.cols);
    }
  }
  for (int u = 0; u < ozk::rc_reduce_lanes(g); u++) {
    int col, first, stride, n;
    ozk::rc_reduce_part(g, u, &col, &first, &stride, &n);
    printf("D %d %d %d %d %d\n", u, col, first, stride, n);
  }
  if (s == (cb + 1) / 2 && chunk == ozk::RC_CHUNK) {   // the geometry the kernels use
    const ozk::RcGeom d = ozk::rc_geom(cb);
    if (d.s != g.s || d.rows != g.rows || d.cols != g.cols || d.row_parts != g.row_parts || d.col_parts != g.col_parts) return 3;
  }
  return 0;
}
