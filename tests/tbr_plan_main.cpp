// tbr_plan_main.cpp -- mpboot_amd/host/tbr_plan.hpp driven without a device (tests/test_tbr_plan_host.py builds this with
// -fsanitize=address,undefined and compares what it prints with tests/tbr_witness.py).
//
// input (text):  n maxtrav cap tile S n_visits n_edits | back[3 (2 n - 1)] | visit records | edits as (p f g)
// output:  per visit  "visit p q" / "F rec:depth ..." / "G rec:depth ..." / "ops side kind:depth:own:sib:out ..." (side 0 = F, 1 = G)
//          "chunks b:e ..."    the sweep of the visits under `cap` vectors
//          per chunk "items shape:visit:ft:gt ..."   the tile list (shape 1 narrow | 2 wide)
//          "best value index" the first minimum of the visits' row counts taken as a matrix (the rule alone)
//          per edit "edit back ..."
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mpboot_amd/host/tbr_plan.hpp"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n, maxtrav, tile, S, n_visits, n_edits;
  long long cap;
  if (std::fscanf(f, "%d %d %lld %d %d %d %d", &n, &maxtrav, &cap, &tile, &S, &n_visits, &n_edits) != 7) return 2;
  std::vector<int32_t> back(3 * (size_t)(2 * n - 1)), recs((size_t)n_visits), edits(3 * (size_t)n_edits);
  for (auto *v : {&back, &recs, &edits})
    for (int32_t &x : *v)
      if (std::fscanf(f, "%d", &x) != 1) return 2;
  std::fclose(f);

  std::vector<tbrplan::Visit> vis((size_t)n_visits);
  std::vector<size_t> need, entries;
  std::vector<uint32_t> rows;
  for (int i = 0; i < n_visits; i++) {
    tbrplan::Visit &v = vis[(size_t)i];
    tbrplan::visit(n, back.data(), recs[(size_t)i], maxtrav, v);
    std::printf("visit %d %d\n", v.p, v.q);
    const tbrplan::Side *sides[2] = {&v.F, &v.G};
    for (int s = 0; s < 2; s++) {
      std::fputs(s ? "G" : "F", stdout);
      for (size_t k = 0; k < sides[s]->rec.size(); k++) std::printf(" %d:%d", sides[s]->rec[k], sides[s]->depth[k]);
      std::printf("\n");
    }
    for (int s = 0; s < 2; s++) {
      std::vector<tbrplan::Op> ops;
      tbrplan::Side again;
      tbrplan::side(n, back.data(), s ? v.p : v.q, maxtrav, again, &ops, 100u * (uint32_t)s);
      if (again.rec != sides[s]->rec || again.max_depth != sides[s]->max_depth) return 3;
      std::printf("ops %d", s);
      for (const tbrplan::Op &o : ops) std::printf(" %u:%u:%u:%u:%u", o.meta >> 16, o.meta & 255u, o.own, o.sib, o.out);
      std::printf("\n");
    }
    need.push_back(v.vectors());
    entries.push_back(v.rows() * v.cols());
    rows.push_back((uint32_t)v.rows());
  }
  const auto chunks = tbrplan::chunks(need, (size_t)cap, entries);
  std::printf("chunks");
  for (const auto &c : chunks) std::printf(" %zu:%zu", c.first, c.second);
  std::printf("\n");
  for (const auto &c : chunks) {
    std::vector<tbrplan::Item> items[2];
    for (size_t i = c.first; i < c.second; i++) {
      const int shape = tbrplan::pick(S, vis[i].rows(), vis[i].cols(), tile);
      tbrplan::tiles((uint32_t)(i - c.first), vis[i].rows(), vis[i].cols(), tbrplan::tile_dims(S, shape), items[shape - 1]);
    }
    std::printf("items");
    for (int s = 0; s < 2; s++)
      for (const tbrplan::Item &it : items[s]) std::printf(" %d:%u:%u:%u", s + 1, it.visit, it.ft, it.gt);
    std::printf("\n");
  }
  const auto best = tbrplan::first_min(rows.data(), rows.size());
  std::printf("best %u %lld\n", best.first, best.second == (size_t)-1 ? -1ll : (long long)best.second);
  for (int i = 0; i < n_edits; i++) {
    std::vector<int32_t> b = back;
    tbrplan::apply(b.data(), edits[3 * (size_t)i], edits[3 * (size_t)i + 1], edits[3 * (size_t)i + 2]);
    std::printf("edit");
    for (int32_t x : b) std::printf(" %d", x);
    std::printf("\n");
  }
  return 0;
}
