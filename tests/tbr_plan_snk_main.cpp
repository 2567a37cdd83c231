// tbr_plan_snk_main.cpp -- the tiles of a TBR visit under the weighted rows of the shape table (mpboot_amd/host/tbr_plan.hpp:
// tile_dims, pick and tiles with the engine kind), as a stand-alone program for tests/test_tbr_plan_snk_host.py.  Device-free.
//
// input : lines "S rows cols tile"
// output: per line  "dims <narrow tf> <narrow tg> <wide tf> <wide tg>"     the weighted tiles
//                   "plain <wide tf> <wide tg> <pick>"                      what the defaulted parameter still gives
//                   "pick <shape>"                                          the weighted pick
//                   "items <ft>:<gt> ..."                                   the visit's items in the picked shape, in launch order
#include <cstdio>
#include <vector>

#include "../mpboot_amd/host/tbr_plan.hpp"

static_assert(tbrplan::tile_dims(20, tbrplan::TILE_WIDE).tf == 32 && tbrplan::tile_dims(20, tbrplan::TILE_WIDE, false).tg == 32, "the Fitch rows");
static_assert(tbrplan::tile_dims(20, tbrplan::TILE_WIDE, true).tf == 64 && tbrplan::tile_dims(20, tbrplan::TILE_WIDE, true).tg == 64, "20 weighted rows");

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *in = std::fopen(argv[1], "r");
  if (!in) return 2;
  int S, tile;
  unsigned long long rows, cols;
  while (std::fscanf(in, "%d %llu %llu %d", &S, &rows, &cols, &tile) == 4) {
    const tbrplan::TileDims a = tbrplan::tile_dims(S, tbrplan::TILE_NARROW, true), w = tbrplan::tile_dims(S, tbrplan::TILE_WIDE, true);
    const tbrplan::TileDims pw = tbrplan::tile_dims(S, tbrplan::TILE_WIDE);
    std::printf("dims %d %d %d %d\n", a.tf, a.tg, w.tf, w.tg);
    std::printf("plain %d %d %d\n", pw.tf, pw.tg, tbrplan::pick(S, (size_t)rows, (size_t)cols, tile));
    const int shape = tbrplan::pick(S, (size_t)rows, (size_t)cols, tile, true);
    std::printf("pick %d\n", shape);
    std::vector<tbrplan::Item> items;
    tbrplan::tiles(7u, (size_t)rows, (size_t)cols, tbrplan::tile_dims(S, shape, true), items);
    std::printf("items");
    for (const tbrplan::Item &it : items) {
      if (it.visit != 7u || it.pad != 0u) return 3;
      std::printf(" %u:%u", it.ft, it.gt);
    }
    std::printf("\n");
  }
  std::fclose(in);
  return 0;
}
