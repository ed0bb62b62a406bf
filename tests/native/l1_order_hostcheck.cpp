// Stand-alone host program over the length order and the dense-merge test of octopuszk_amd/csrc/l1_whole.h
// (tests/test_l1_order_cpu.py compiles it with g++ and the address / undefined-behaviour sanitizers and compares its
// output with a Python model).
//   stdin:  W NH nb g_top, then 2 x WHOLE_KEYS class-table words (region 0, region 1)
//   stdout: one section per line, numbers only after the tag:
//     "C keys wave tb table_words"
//     "K ..."   whole_key(count, G) for G = 2 then 4, count = 0 .. 1100
//     "R ..."   per region: group size, items, lanes
//     "B ..."   per region: the WHOLE_KEYS class bases of its table
//     "N nb0 nb1 lanes"
//     "V ..."   whole_block_interleave(p, nb0, nb1) for p = 0 .. nb0 + nb1 - 1
//     "L ..."   item g G for every lane of the grid (whole_lane_map_len)
//     "D ..."   per order (0, 1) and workgroup: whole_block_dense, then whether all its 256 lanes exist and have G = 2
//               (by the lane maps, lane by lane)
#include <stdio.h>

#include <vector>

#include "../../octopuszk_amd/csrc/l1_whole.h"

int main() {
  using namespace ozk;
  WholeGeom geo;
  if (scanf("%d %d %d %d", &geo.W, &geo.NH, &geo.nb, &geo.g_top) != 4 || geo.nb < 1 || geo.nb > WHOLE_NB_MAX) return 2;
  std::vector<uint32_t> T(2 * WHOLE_KEYS);
  for (auto& v : T)
    if (scanf("%u", &v) != 1) return 2;
  printf("C %d %d %d %d\n", WHOLE_KEYS, WHOLE_WAVE, WHOLE_TB, WHOLE_TABLE_WORDS);
  printf("K");
  for (uint32_t G = 2; G <= 4; G += 2)
    for (uint32_t c = 0; c <= 1100; c++) printf(" %u", whole_key(c, G));
  printf("\nR");
  for (int r = 0; r < 2; r++) printf(" %u %u %u", whole_region_group(geo, r), whole_region_items(geo, r), whole_region_lanes(geo, r));
  printf("\nB");
  for (int r = 0; r < 2; r++) {
    std::vector<uint32_t> base(WHOLE_KEYS);
    whole_class_bases(T.data() + r * WHOLE_KEYS, base.data());
    for (uint32_t v : base) printf(" %u", v);
  }
  uint32_t nb0, nb1;
  whole_len_blocks(geo, &nb0, &nb1);
  const long long lanes = whole_lanes_len(geo);
  printf("\nN %u %u %lld\nV", nb0, nb1, lanes);
  for (uint32_t p = 0; p < nb0 + nb1; p++) printf(" %u", whole_block_interleave(p, nb0, nb1));
  printf("\nL");
  for (long long u = 0; u < lanes; u++) {
    uint32_t item, g, G;
    whole_lane_map_len(geo, (uint32_t)u, &item, &g, &G);
    printf(" %u %u %u", item, g, G);
  }
  printf("\nD");
  for (int order = 0; order < 2; order++) {
    const long long n = order == 1 ? lanes : whole_lanes(geo);
    const uint32_t blocks = (uint32_t)((n + WHOLE_TB - 1) / WHOLE_TB);
    printf(" %u", blocks);
    for (uint32_t b = 0; b < blocks; b++) {
      bool pairs = true;
      for (long long u = (long long)b * WHOLE_TB; u < (long long)(b + 1) * WHOLE_TB; u++) {
        uint32_t item, g, G = 0;
        if (u < n) (order == 1 ? whole_lane_map_len : whole_lane_map)(geo, (uint32_t)u, &item, &g, &G);
        pairs = pairs && G == 2u;
      }
      printf(" %d %d", whole_block_dense(geo, order, b, (uint32_t)n) ? 1 : 0, pairs ? 1 : 0);
    }
  }
  printf("\n");
  return 0;
}
