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

// ---------------------------------------------------------------- items ordered by part length (OZK_MSM_L1_ORDER=1)
// The rank order above makes a wave run "the r-th largest bucket of 32 neighbouring bins": the longest of its 64 parts
// sets its trip count, 4 % above the mean at the workload's shape.  Here an item's KEY is the trip count of its lane 0,
// ceil(count / G) clamped to WHOLE_KEYS - 1 (longer buckets share the last class: only balance suffers), key 0 is the
// empty bucket, and the items of a REGION descend by key over all windows.  Region 0 holds the ordinary windows' items
// (G = 2), region 1 the top window's where g_top is not 2; lane u of a region serves item u / G, and a region's end is
// padded to a whole wave.  A class table T[region][key] (items per key, summed by k_bin_sums) gives every class its
// first item; inside a class the order is free.  The workgroups of region 1 (and the one that straddles the regions)
// are spread among region 0's in proportion, so that the grid as a whole still runs longest-first.
constexpr int WHOLE_KEYS = 128;
constexpr int WHOLE_WAVE = 64, WHOLE_TB = 256;          // lanes per wave and per workgroup of k_l1_whole
constexpr int WHOLE_TABLE_WORDS = 2 * 2 * WHOLE_KEYS;   // T[2][KEYS], then the cursors C[2][KEYS] k_bucket_items takes slots from
OZK_HD uint32_t whole_key(uint32_t count, uint32_t G) {
  const uint32_t k = (count + G - 1) / G;
  return k < (uint32_t)(WHOLE_KEYS - 1) ? k : (uint32_t)(WHOLE_KEYS - 1);
}
OZK_HD int whole_regions(const WholeGeom& g) { return g.g_top == WHOLE_G ? 1 : 2; }
OZK_HD int whole_bin_region(const WholeGeom& g, int bin) { return (whole_regions(g) == 2 && bin / g.NH == g.W - 1) ? 1 : 0; }
OZK_HD uint32_t whole_region_group(const WholeGeom& g, int r) { return r == 0 ? (uint32_t)WHOLE_G : (uint32_t)g.g_top; }
OZK_HD uint32_t whole_region_items(const WholeGeom& g, int r) {
  const uint32_t top = (uint32_t)(g.NH * g.nb), all = (uint32_t)(g.W * g.NH * g.nb);
  if (whole_regions(g) == 1) return r == 0 ? all : 0u;
  return r == 0 ? all - top : top;
}
OZK_HD uint32_t whole_region_lanes(const WholeGeom& g, int r) {
  const uint32_t l = whole_region_group(g, r) * whole_region_items(g, r);
  return (l + (uint32_t)(WHOLE_WAVE - 1)) & ~(uint32_t)(WHOLE_WAVE - 1);
}
OZK_HD long long whole_lanes_len(const WholeGeom& g) { return (long long)whole_region_lanes(g, 0) + whole_region_lanes(g, 1); }
// class bases of one region: base[k] = items with a key above k (the classes descend by key; T has WHOLE_KEYS words)
OZK_HD uint32_t whole_class_base(const uint32_t* T, uint32_t key) {
  uint32_t s = 0;
  for (uint32_t k = (uint32_t)WHOLE_KEYS - 1; k > key; k--) s += T[k];
  return s;
}
OZK_HD void whole_class_bases(const uint32_t* T, uint32_t* base) {
  for (uint32_t k = 0; k < (uint32_t)WHOLE_KEYS; k++) base[k] = whole_class_base(T, k);
}
// the workgroups: nb0 lie wholly in region 0, the other nb1 (the straddling one first) follow in lane order
OZK_HD void whole_len_blocks(const WholeGeom& g, uint32_t* nb0, uint32_t* nb1) {
  const uint32_t all = (uint32_t)((whole_lanes_len(g) + WHOLE_TB - 1) / WHOLE_TB);
  *nb0 = whole_region_lanes(g, 0) / (uint32_t)WHOLE_TB;
  *nb1 = all - *nb0;
}
// launch order -> lane order: workgroup p of the grid runs lanes [b * WHOLE_TB, (b + 1) * WHOLE_TB), the nb1 late
// workgroups spread evenly among the nb0 early ones (a bijection of [0, nb0 + nb1))
OZK_HD uint32_t whole_block_interleave(uint32_t p, uint32_t nb0, uint32_t nb1) {
  const unsigned long long n = (unsigned long long)nb0 + nb1;
  const uint32_t before = (uint32_t)((unsigned long long)p * nb1 / n), upto = (uint32_t)(((unsigned long long)p + 1) * nb1 / n);
  return upto > before ? nb0 + before : p - before;
}
// lane u (lane order) -> its item (WHOLE_NO_ITEM for a padding lane), place g in the lane group, group size G
OZK_HD void whole_lane_map_len(const WholeGeom& geo, uint32_t u, uint32_t* item, uint32_t* g, uint32_t* G) {
  const uint32_t l0 = whole_region_lanes(geo, 0), n0 = whole_region_items(geo, 0);
  if (u < l0) {
    *G = (uint32_t)WHOLE_G;
    *g = u % (uint32_t)WHOLE_G;
    const uint32_t i = u / (uint32_t)WHOLE_G;
    *item = i < n0 ? i : WHOLE_NO_ITEM;
  } else {
    const uint32_t q = u - l0, gt = (uint32_t)geo.g_top;
    *G = gt;
    *g = q % gt;
    const uint32_t i = q / gt;
    *item = i < whole_region_items(geo, 1) ? n0 + i : WHOLE_NO_ITEM;
  }
}

// ---------------------------------------------------------------- dense merges
// A workgroup all of whose lanes are pairs (G = 2) merges its 128 buckets on two full waves through LDS, not on four
// half-used ones by quad permutes.  Whether workgroup `block` (lane order) is such a one, from the geometry alone:
// uniform over the workgroup.  order 1: it lies wholly in region 0; order 0: wholly in one rank's ordinary section.
OZK_HD bool whole_block_dense(const WholeGeom& geo, int order, uint32_t block, uint32_t n_lanes) {
  const unsigned long long t0 = (unsigned long long)block * WHOLE_TB;
  if (t0 + WHOLE_TB > n_lanes) return false;
  if (order == 1) return t0 + WHOLE_TB <= whole_region_lanes(geo, 0);
  const uint32_t per_rank = (uint32_t)whole_lanes_per_rank(geo);
  const uint32_t q0 = (uint32_t)(t0 % per_rank);
  return q0 + (uint32_t)WHOLE_TB <= (uint32_t)whole_pad4(WHOLE_G * geo.NH * (geo.W - 1));
}

}  // namespace ozk
