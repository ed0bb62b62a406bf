// Whole-bucket level 1 of the G1 variable-base MSM: the arithmetic of the item order, the lane map and the split of a
// bucket over its lane group.  Plain C++ (no HIP header needed), so that tests/native/l1_items_hostcheck.cpp compiles
// it with g++ and checks it against a Python model; the kernels (msm_var.cuh k_bucket_items, k_l1_whole) and the
// driver (msm_var_driver.cuh var_msm_accum) use exactly these functions.
//
// One ITEM per bucket: (entry offset, count, bucket id).  The buckets of one coarse sort bin (`nb` consecutive bucket
// ids of one window, at most 128) are ranked by descending count, ties by index, and item (rank, bin) lives at index
// rank * nbins + bin: consecutive items are "the r-th largest bucket of neighbouring bins", whose counts are nearly
// equal — the lanes of a wave run the same trip count — and the grid as a whole runs longest-first.
// G adjacent lanes own one item: 2 for an ordinary window, g_top for the top window (4 where a GLV plan's top digits
// have fewer significant bits and its buckets are longer).
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

constexpr int WHOLE_G = 2;            // lanes per bucket, ordinary windows
constexpr int WHOLE_LANE_MAX = 255;   // entries per lane above which a bucket is "too long": the MSM takes the chunked path
constexpr int WHOLE_NB_MAX = 128;     // buckets per coarse bin with signed digits (msm_var_driver.cuh make_layout3: lo_bits <= 7)

struct WholeGeom {
  int W;       // windows
  int NH;      // coarse bins per window
  int nb;      // buckets per coarse bin (power of two, <= WHOLE_NB_MAX)
  int g_top;   // lanes per bucket in window W - 1 (2 or 4)
};
OZK_HD int whole_nbins(const WholeGeom& g) { return g.W * g.NH; }
// Lanes that serve the items of one rank: NH bins of every ordinary window, WHOLE_G lanes each, then the NH bins of
// the top window, g_top lanes each.  Both sections are padded to a multiple of four lanes (lanes without an item), so
// that every lane group lies inside one aligned quad of its wave: the groups exchange by quad permutes.
constexpr uint32_t WHOLE_NO_ITEM = 0xffffffffu;
OZK_HD int whole_pad4(int x) { return (x + 3) & ~3; }
OZK_HD int whole_lanes_per_rank(const WholeGeom& g) {
  return whole_pad4(WHOLE_G * g.NH * (g.W - 1)) + whole_pad4(g.g_top * g.NH);
}
OZK_HD long long whole_lanes(const WholeGeom& g) { return (long long)g.nb * whole_lanes_per_rank(g); }
OZK_HD int whole_group(const WholeGeom& g, int bin) { return bin / g.NH == g.W - 1 ? g.g_top : WHOLE_G; }
OZK_HD uint32_t whole_limit(int G) { return (uint32_t)(G * WHOLE_LANE_MAX); }

// rank of bucket i among the nb counts of its bin: descending count, ties by index
OZK_HD uint32_t whole_rank(const uint32_t* cnt, int nb, int i) {
  const uint32_t c = cnt[i];
  uint32_t r = 0;
  for (int j = 0; j < nb; j++) r += (cnt[j] > c) || (cnt[j] == c && j < i);
  return r;
}
OZK_HD uint32_t whole_item_index(uint32_t rank, uint32_t bin, uint32_t nbins) { return rank * nbins + bin; }

// lane t of the level-1 grid -> its item (WHOLE_NO_ITEM for a padding lane), its place g in the item's lane group
// and the group's size G
OZK_HD void whole_lane_map(const WholeGeom& geo, uint32_t t, uint32_t* item, uint32_t* g, uint32_t* G) {
  const uint32_t per_rank = (uint32_t)whole_lanes_per_rank(geo);
  const uint32_t rank = t / per_rank, q = t - rank * per_rank;
  const uint32_t ordinary = (uint32_t)(WHOLE_G * geo.NH * (geo.W - 1));
  const uint32_t ordinary_pad = (uint32_t)whole_pad4((int)ordinary);
  uint32_t bin;
  bool pad;
  if (q < ordinary_pad) {
    bin = q / WHOLE_G;
    *g = q % WHOLE_G;
    *G = WHOLE_G;
    pad = q >= ordinary;
  } else {
    const uint32_t q2 = q - ordinary_pad;
    bin = (uint32_t)(geo.NH * (geo.W - 1)) + q2 / (uint32_t)geo.g_top;
    *g = q2 % (uint32_t)geo.g_top;
    *G = (uint32_t)geo.g_top;
    pad = q2 >= (uint32_t)(geo.g_top * geo.NH);
  }
  *item = pad ? WHOLE_NO_ITEM : whole_item_index(rank, bin, (uint32_t)whole_nbins(geo));
}

// lane g of G takes entries [first, first + len) of a bucket of `count`: G contiguous parts whose lengths differ by at
// most one, none longer than lane 0's (count 1: lane 0 has the entry, the others are empty)
OZK_HD void whole_part(uint32_t count, uint32_t g, uint32_t G, uint32_t* first, uint32_t* len) {
  const uint32_t a = (count * g + G - 1) / G, b = (count * (g + 1) + G - 1) / G;
  *first = a;
  *len = b - a;
}

}  // namespace ozk
