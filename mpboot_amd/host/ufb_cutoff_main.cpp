// ufb_cutoff_main.cpp -- the cut-off filter of ufb_cutoff.hpp as a stand-alone program: no device, no engine.
// tests/test_ufb_cutoff_host.py builds it with -fsanitize=address,undefined, runs it as a child process and compares every line
// of its output with the reference's rule,  -len > logl_cutoff - 1e-4  (iqtree.cpp:3343), evaluated in Python.
//
// stdin:   logl_cutoff (a hexadecimal float, exact)  n_len len_1 .. len_n  n_base base_1 .. base_n
// stdout:  "have_cut none_pass mp_max", then per length "len pass", then per base "base threshold"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ufb_cutoff.hpp"

using namespace mpf;

static bool read_list(std::vector<uint32_t> &v)
{
  int n = 0;
  if (std::scanf("%d", &n) != 1 || n < 0 || n > (1 << 20)) return false;
  v.resize((size_t)n);
  for (uint32_t &x : v)
    if (std::scanf("%" SCNu32, &x) != 1) return false;
  return true;
}

int main()
{
  char word[64];
  if (std::scanf("%63s", word) != 1) return 2;
  char *end = nullptr;
  const double logl_cutoff = std::strtod(word, &end);
  if (end == word || *end) return 2;
  std::vector<uint32_t> lens, bases;
  if (!read_list(lens) || !read_list(bases)) return 2;
  const UfbCutoff cut = ufb_cutoff(logl_cutoff);
  std::printf("%d %d %" PRIu32 "\n", (int)cut.have_cut, (int)cut.none_pass, cut.mp_max);
  for (uint32_t len : lens) std::printf("%" PRIu32 " %d\n", len, (int)cut.passes(len));
  for (uint32_t base : bases) std::printf("%" PRIu32 " %" PRIu32 "\n", base, cut.part_threshold(base));
  return 0;
}
