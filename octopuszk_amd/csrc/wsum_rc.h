// Window sums by bucket rows and columns (the THROUGHPUT tail of the G1 variable-base MSM): the index arithmetic.
// Plain C++ (no HIP header needed), so that tests/native/wsum_rc_hostcheck.cpp compiles it with g++ and checks it
// against a Python model; the kernels (msm_var.cuh k_rc_partial, k_rc_reduce, k_rc_wave) and the driver
// (msm_var_driver.cuh var_msm_tail) use exactly these functions.
//
// The 2^cb buckets of one window are read as a matrix: bucket b = r 2^s + q sits in row r, column q, with
// s = ceil(cb / 2): 2^(cb - s) rows of 2^s buckets.  With R_r the plain sum of row r and C_q that of column q,
//     sum_b (b + sd) B_b  =  2^s sum_r r R_r  +  sum_q (q + sd) C_q
// (sd = 1 with signed digits: bucket b weighs b + 1), so every bucket enters two unweighted sums and only the
// 2^(cb - s) + 2^s row and column sums are weighted.
//
// Stage 1 (k_rc_partial): lane t of a window adds row part t, RC_CHUNK consecutive buckets of one row, into row slot
// t, and column part t, RC_CHUNK buckets down one column, into column slot t.  The last part of a row or column
// shorter than a multiple of RC_CHUNK is short.  Lanes adjacent in t take adjacent columns.
// Stage 2 (k_rc_reduce): lane u adds the slots of row u or of column u - rows.
#pragma once
#include <stdint.h>

#if !defined(OZK_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OZK_HD __host__ __device__ __forceinline__
#else
#define OZK_HD inline
#endif
#endif

namespace ozk {

constexpr int RC_CHUNK = 16;   // buckets per partial sum

struct RcGeom {
  int cb;         // bucket-index bits per window
  int s;          // log2 of the row length
  int rows;       // 2^(cb - s)
  int cols;       // 2^s: the row length
  int row_parts;  // parts per row: ceil(cols / chunk)
  int col_parts;  // parts per column: ceil(rows / chunk)
};
OZK_HD RcGeom rc_geom(int cb, int s, int chunk) {
  RcGeom g;
  g.cb = cb;
  g.s = s;
  g.rows = 1 << (cb - s);
  g.cols = 1 << s;
  g.row_parts = (g.cols + chunk - 1) / chunk;
  g.col_parts = (g.rows + chunk - 1) / chunk;
  return g;
}
OZK_HD RcGeom rc_geom(int cb) { return rc_geom(cb, (cb + 1) / 2, RC_CHUNK); }
OZK_HD int rc_row_slots(const RcGeom& g) { return g.rows * g.row_parts; }   // row partial sums per window
OZK_HD int rc_col_slots(const RcGeom& g) { return g.cols * g.col_parts; }   // column partial sums per window
OZK_HD int rc_partial_lanes(const RcGeom& g) {
  return rc_row_slots(g) > rc_col_slots(g) ? rc_row_slots(g) : rc_col_slots(g);
}
OZK_HD int rc_reduce_lanes(const RcGeom& g) { return g.rows + g.cols; }

// row part t < rc_row_slots: buckets first, first + 1, ... (n of them) of row t / row_parts; its sum goes to row slot t
OZK_HD void rc_row_part(const RcGeom& g, int t, int chunk, uint32_t* first, int* n) {
  const int r = t / g.row_parts, k = t - r * g.row_parts;
  const int q0 = k * chunk;
  *first = ((uint32_t)r << g.s) + (uint32_t)q0;
  *n = g.cols - q0 < chunk ? g.cols - q0 : chunk;
}
// column part t < rc_col_slots: buckets first, first + 2^s, ... (n of them) of column t % cols; column slot t
OZK_HD void rc_col_part(const RcGeom& g, int t, int chunk, uint32_t* first, int* n) {
  const int k = t >> g.s, q = t & (g.cols - 1);
  const int r0 = k * chunk;
  *first = ((uint32_t)r0 << g.s) + (uint32_t)q;
  *n = g.rows - r0 < chunk ? g.rows - r0 : chunk;
}
// reduce lane u < rows + cols: `n` slots from `first` on, `stride` apart, of the row slots (*col = 0; the sum is R_u)
// or of the column slots (*col = 1; the sum is C_(u - rows))
OZK_HD void rc_reduce_part(const RcGeom& g, int u, int* col, int* first, int* stride, int* n) {
  if (u < g.rows) {
    *col = 0;
    *first = u * g.row_parts;
    *stride = 1;
    *n = g.row_parts;
  } else {
    *col = 1;
    *first = u - g.rows;
    *stride = g.cols;
    *n = g.col_parts;
  }
}

}  // namespace ozk
