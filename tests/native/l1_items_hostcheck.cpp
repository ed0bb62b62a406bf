// Stand-alone host program over octopuszk_amd/csrc/l1_whole.h (tests/test_l1_items_cpu.py compiles it with g++ and
// compares its output with a Python model).
//   stdin:  W NH nb g_top, then W * NH lines of nb bucket counts (one coarse bin per line)
//   stdout: "I bin idx..."            item index of every bucket of the bin (whole_rank + whole_item_index)
//           "L t item g G"            every lane of the level-1 grid (whole_lane_map)
//           "P count g G first len"   the split of a bucket over its lane group (whole_part), counts 0..600
//           "G bin group limit"       lanes per bucket and the longest bucket the group takes
#include <stdio.h>

#include <vector>

#include "../../octopuszk_amd/csrc/l1_whole.h"

int main() {
  ozk::WholeGeom geo;
  if (scanf("%d %d %d %d", &geo.W, &geo.NH, &geo.nb, &geo.g_top) != 4 || geo.nb < 1 || geo.nb > ozk::WHOLE_NB_MAX) return 2;
  const int nbins = ozk::whole_nbins(geo);
  std::vector<uint32_t> cnt((size_t)geo.nb);
  for (int bin = 0; bin < nbins; bin++) {
    for (int i = 0; i < geo.nb; i++)
      if (scanf("%u", &cnt[(size_t)i]) != 1) return 2;
    printf("I %d", bin);
    for (int i = 0; i < geo.nb; i++)
      printf(" %u", ozk::whole_item_index(ozk::whole_rank(cnt.data(), geo.nb, i), (uint32_t)bin, (uint32_t)nbins));
    printf("\n");
    const int G = ozk::whole_group(geo, bin);
    printf("G %d %d %u\n", bin, G, ozk::whole_limit(G));
  }
  const long long lanes = ozk::whole_lanes(geo);
  for (long long t = 0; t < lanes; t++) {
    uint32_t item, g, G;
    ozk::whole_lane_map(geo, (uint32_t)t, &item, &g, &G);
    printf("L %lld %u %u %u\n", t, item, g, G);
  }
  for (uint32_t G = 1; G <= 4; G <<= 1)
    for (uint32_t count = 0; count <= 600; count++)
      for (uint32_t g = 0; g < G; g++) {
        uint32_t first, len;
        ozk::whole_part(count, g, G, &first, &len);
        printf("P %u %u %u %u %u\n", count, g, G, first, len);
      }
  return 0;
}
