// splits_host_main.cpp -- the host-only part of the bootstrap summary (split_sets.hpp) as a stand-alone program: no device, no
// engine, nothing loaded into another process.  tests/test_splits_host.py builds it with -fsanitize=address,undefined and compares
// its output with a Python restatement; tools/splits_timing.py builds it optimised as the CPU yardstick of the device path.
//
//   splits_host tables FILE THRESHOLD   FILE: text, "n m total" and then m lines "count word0 word1 ..." (words in hex): a table of
//                                       distinct splits in any order.  Prints the contract order (as input row numbers), the rows the
//                                       consensus rule keeps and the neighbour lists built from them.
//   splits_host trees FILE THRESHOLD    FILE: binary int32: n, n_trees, has_weights, backs[n_trees][3 (2n - 1)], weights[n_trees] if
//                                       has_weights.  The whole summary on the host: the table in the contract order, the supports
//                                       of the first tree's clusters, the consensus lists, and the time each step took.  A fifth
//                                       argument "quiet" leaves the table itself out (timing runs on large sets).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
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

static void print_consensus(const SplitTable &t, double threshold)
{
  const std::vector<int64_t> kept = greedy_compatible(t, threshold);
  ListTree lt;
  build_lists(t, kept, lt);
  print_list("kept", kept);
  print_list("first", lt.first);
  print_list("nbr", lt.nbr);
  print_list("support", lt.support);
}

static int run_tables(const char *path, double threshold)
{
  std::ifstream in(path);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
  SplitTable t;
  long long m = 0, total = 0;
  in >> t.n >> m >> total;
  if (!in || t.n < 4 || m < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  t.words = words_of(t.n);
  t.total = total;
  for (long long i = 0; i < m; i++) {
    long long c = 0;
    in >> c;
    t.count.push_back(c);
    for (int w = 0; w < t.words; w++) {
      std::string hex;
      in >> hex;
      t.bits.push_back((uint32_t)std::strtoul(hex.c_str(), nullptr, 16));
    }
    if (!in) { std::fprintf(stderr, "bad row %lld\n", i); return 2; }
  }
  const std::vector<int64_t> p = order_splits(t);
  print_list("order", p);
  apply_order(t, p);
  print_consensus(t, threshold);
  return 0;
}

static int run_trees(const char *path, double threshold, bool quiet)
{
  std::ifstream in(path, std::ios::binary);
  int32_t head[3] = {0, 0, 0};
  in.read(reinterpret_cast<char *>(head), sizeof(head));
  const int n = head[0], T = head[1];
  if (!in || n < 4 || T < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
  const size_t len = 3 * (size_t)(2 * n - 1);
  std::vector<int32_t> backs((size_t)T * len), weights;
  in.read(reinterpret_cast<char *>(backs.data()), (std::streamsize)(backs.size() * sizeof(int32_t)));
  if (head[2]) {
    weights.resize((size_t)T);
    in.read(reinterpret_cast<char *>(weights.data()), (std::streamsize)(weights.size() * sizeof(int32_t)));
  }
  if (!in) { std::fprintf(stderr, "short file\n"); return 2; }
  SplitTable t;
  const double t0 = now_ms();
  if (!count_splits(n, T, backs.data(), head[2] ? weights.data() : nullptr, t)) { std::fprintf(stderr, "a tree is not a complete tree\n"); return 3; }
  const double t1 = now_ms();
  // the supports of the first tree's branches: its clusters looked up in the table
  TreeClusters c;
  std::vector<int64_t> sup;
  {
    SetIndex idx(t.words);
    for (size_t i = 0; i < t.size(); i++) idx.insert(t.row(i), (int64_t)i);
    walk_clusters(backs.data(), n, c);
    std::vector<uint32_t> w((size_t)t.words);
    for (int ci = 0; ci < n - 3; ci++) {
      cluster_bits(c, ci, t.words, w.data());
      const int64_t k = idx.find(t.bits, w.data());
      sup.push_back(k < 0 ? 0 : t.count[(size_t)k]);
    }
  }
  const double t2 = now_ms();
  apply_order(t, order_splits(t));
  const double t3 = now_ms();
  std::printf("n_distinct %zu\ntotal %lld\n", t.size(), (long long)t.total);
  if (!quiet) {
    print_list("count", t.count);
    std::printf("bits");
    for (uint32_t w : t.bits) std::printf(" %08x", w);
    std::printf("\n");
  }
  print_list("target_node", c.node);
  print_list("target_support", sup);
  const double t4 = now_ms();
  print_consensus(t, threshold);
  const double t5 = now_ms();
  std::printf("ms_count %.3f\nms_support %.3f\nms_order %.3f\nms_consensus %.3f\n", t1 - t0, t2 - t1, t3 - t2, t5 - t4);
  return 0;
}

int main(int argc, char **argv)
{
  if (argc != 4 && argc != 5) { std::fprintf(stderr, "usage: %s tables|trees FILE THRESHOLD [quiet]\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  const double threshold = std::atof(argv[3]);
  if (mode == "tables") return run_tables(argv[2], threshold);
  if (mode == "trees") return run_trees(argv[2], threshold, argc == 5 && std::string(argv[4]) == "quiet");
  std::fprintf(stderr, "unknown mode %s\n", argv[1]);
  return 2;
}
