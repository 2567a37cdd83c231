// tbr_book_snk_main.cpp -- the device-free half of a tracked TBR sweep's bookings on the weighted engine
// (mpboot_amd/host/tbr_plan.hpp: value_bits and book_cap, the automatic batch cap, and the batches and row lists it leads to) as a
// stand-alone program for tests/test_tbr_book_snk_host.py, which builds it with -fsanitize=address,undefined and compares what it
// prints with a plain restatement in Python.
//
// input:   n_visits modulus npat plane_words samples_p top row_tile limit
//          rows cols              per visit
// top = n_taxa x highest_cost, the bound of every value; an entry takes part iff (its number in the whole sweep) % modulus != 0
// (modulus 0: every entry; 1: none).
// output:  bits K
//          cap C
//          then per batch, as tests/tbr_book_main.cpp prints it:
//          batch  visit:begin:end ...
//          rows N
//          runs   visit:row:col>out,col>out,... per MaskRun
#include <cstdio>
#include <vector>

#include "../mpboot_amd/host/tbr_plan.hpp"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned long nv = 0, mod = 0, npat = 0, pw = 0, sp = 0, tile = 0;
  unsigned long long top = 0, limit = 0;
  if (std::fscanf(f, "%lu %lu %lu %lu %lu %llu %lu %llu", &nv, &mod, &npat, &pw, &sp, &top, &tile, &limit) != 8) return 2;
  std::vector<size_t> entries(nv), first(nv);
  std::vector<uint32_t> ncols(nv);
  size_t total = 0;
  for (size_t v = 0; v < nv; v++) {
    unsigned long r = 0, c = 0;
    if (std::fscanf(f, "%lu %lu", &r, &c) != 2) return 2;
    first[v] = total;
    entries[v] = (size_t)r * c;
    ncols[v] = (uint32_t)c;
    total += entries[v];
  }
  std::fclose(f);
  const int bits = tbrplan::value_bits((uint64_t)top);
  const size_t cap = tbrplan::book_cap(npat, pw, sp, bits, tile, (size_t)limit);
  std::printf("bits %d\ncap %zu\n", bits, cap);
  std::vector<tbrplan::BookRun> runs;
  std::vector<size_t> off;
  tbrplan::book_batches(entries, cap, runs, off);
  std::vector<tbrplan::MaskRun> mr;
  std::vector<tbrplan::MaskCol> mc;
  std::vector<uint32_t> crow, home;
  std::vector<uint8_t> take;
  for (size_t b = 0; b + 1 < off.size(); b++) {
    const tbrplan::BookRun *br = runs.data() + off[b];
    const size_t n_runs = off[b + 1] - off[b];
    take.clear();
    std::printf("batch");
    for (size_t r = 0; r < n_runs; r++) {
      std::printf(" %u:%llu:%llu", br[r].visit, (unsigned long long)br[r].begin, (unsigned long long)br[r].end);
      for (uint64_t e = br[r].begin; e < br[r].end; e++) take.push_back(mod == 0 || (first[br[r].visit] + (size_t)e) % mod != 0);
    }
    const uint32_t rows = tbrplan::mask_rows(br, n_runs, ncols.data(), take.data(), mr, mc, crow, home);
    std::printf("\nrows %u\nruns", rows);
    for (const tbrplan::MaskRun &m : mr) {
      std::printf(" %u:%u:", m.visit, m.row);
      for (uint32_t c = m.begin; c < m.end; c++) std::printf("%s%u>%u", c == m.begin ? "" : ",", mc[c].col, mc[c].out);
    }
    std::printf("\n");
  }
  return 0;
}
