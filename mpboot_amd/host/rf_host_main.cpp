// rf_host_main.cpp -- the host-only part of the Robinson-Foulds distances (split_sets.hpp) as a stand-alone program: no device, no
// engine, nothing loaded into another process.  tests/test_rf_host.py builds it with -fsanitize=address,undefined and compares its
// output with a Python restatement; tools/rf_timing.py builds it optimised as the CPU yardstick of the device path.
//
//   rf_host rf FILE [quiet]            FILE: binary int32: n, mode (0 all pairs, 1 adjacent, 2 two sets), n_trees, n_trees2,
//                                      backs[n_trees][3 (2n - 1)], backs2[n_trees2][3 (2n - 1)].  Prints the distances in the
//                                      mode's layout and the time they took; "quiet" prints their sum instead (timing runs).
//   rf_host groups FILE                FILE: text, "words m first_col" and then m lines of `words` hex words: the sets of an
//                                      overflow list.  Prints the column of every set (-1: none) and the number of columns.
//   rf_host plan COLUMNS ROWS FORCED BUDGET_BYTES K_STEP    prints the chunk plan: the c0 and the c1 of every chunk.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "split_sets.hpp"

using namespace mpf::splitsets;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class V>
static void print_list(const char *name, const V &v)
{
  std::printf("%s", name);
  for (const auto &x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}

static int run_rf(const char *path, bool quiet)
{
  std::ifstream in(path, std::ios::binary);
  int32_t head[4] = {0, 0, 0, 0};
  in.read(reinterpret_cast<char *>(head), sizeof(head));
  const int n = head[0], mode = head[1], T = head[2], T2 = head[3];
  if (!in || n < 3 || T < 1 || T2 < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  const size_t len = 3 * (size_t)(2 * n - 1);
  std::vector<int32_t> backs((size_t)T * len), backs2((size_t)T2 * len);
  in.read(reinterpret_cast<char *>(backs.data()), (std::streamsize)(backs.size() * sizeof(int32_t)));
  if (T2) in.read(reinterpret_cast<char *>(backs2.data()), (std::streamsize)(backs2.size() * sizeof(int32_t)));
  if (!in) { std::fprintf(stderr, "short file\n"); return 2; }
  std::vector<int32_t> out;
  int bad_tree = -1;
  const double t0 = now_ms();
  if (!host_rf(n, mode, T, backs.data(), T2, backs2.data(), out, &bad_tree)) {
    if (bad_tree >= 0) { std::fprintf(stderr, "tree %d is not a complete tree\n", bad_tree); return 3; }
    std::fprintf(stderr, "unknown mode %d\n", mode);
    return 2;
  }
  const double t1 = now_ms();
  if (quiet) {
    long long sum = 0;
    for (int32_t x : out) sum += x;
    std::printf("entries %zu\nsum %lld\n", out.size(), sum);
  } else
    print_list("rf", out);
  std::printf("ms_rf %.3f\n", t1 - t0);
  return 0;
}

static int run_groups(const char *path)
{
  std::ifstream in(path);
  long long words = 0, m = 0, first = 0;
  in >> words >> m >> first;
  if (!in || words < 1 || m < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<uint32_t> sets;
  for (long long i = 0; i < m * words; i++) {
    std::string hex;
    in >> hex;
    if (!in) { std::fprintf(stderr, "short file\n"); return 2; }
    sets.push_back((uint32_t)std::strtoul(hex.c_str(), nullptr, 16));
  }
  std::vector<int64_t> col;
  const int64_t k = overflow_columns(sets, (size_t)m, (int)words, first, col);
  print_list("col", col);
  std::printf("n_columns %lld\n", (long long)k);
  return 0;
}

static int run_plan(char **a)
{
  const std::vector<RfChunk> plan = rf_chunk_plan(std::atoll(a[0]), std::atoll(a[1]), std::atoll(a[2]), std::atoll(a[3]), std::atoll(a[4]));
  std::vector<int64_t> c0, c1;
  for (const RfChunk &c : plan) { c0.push_back(c.c0); c1.push_back(c.c1); }
  print_list("c0", c0);
  print_list("c1", c1);
  return 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rf" && (argc == 3 || argc == 4)) return run_rf(argv[2], argc == 4 && std::string(argv[3]) == "quiet");
  if (mode == "groups" && argc == 3) return run_groups(argv[2]);
  if (mode == "plan" && argc == 7) return run_plan(argv + 2);
  std::fprintf(stderr, "usage: %s rf FILE [quiet] | groups FILE | plan COLUMNS ROWS FORCED BUDGET_BYTES K_STEP\n", argv[0]);
  return 2;
}
