// split_lists_host_main.cpp -- the host-only part of the split products on trees given as neighbour lists (split_sets.hpp: lists_ok,
// walk_clusters_lists, count_splits and host_rf on mixed sets) as a stand-alone program: no device, no engine, nothing loaded into
// another process.  tests/test_split_lists_host.py builds it with -fsanitize=address,undefined and compares its output with a Python
// restatement; tools/split_lists_timing.py builds it optimised as the CPU yardstick of the device path.
//
// FILE: binary int32.  Header n, mode (0 all pairs, 1 adjacent, 2 two sets), has_weights, n_records, n_lists, n_records2, n_lists2;
// then the first set -- backs[n_records][3 (2n - 1)], n_inner[n_lists], the trees' first[] one behind the other, their nbr[] one
// behind the other --, the second set in the same form, and, if has_weights, weights[n_records + n_lists] of the first set.
//
//   split_lists_host check FILE        lists_ok of every list tree of the first set: "list k ok" or "list k bad: <why>"
//   split_lists_host walk FILE         walk_clusters_lists of every list tree of the first set: "list k order ...", "list k pos ...",
//                                      and "list k cluster lo hi node" per cluster ("list k bad" if the walk refuses it)
//   split_lists_host counts FILE       count_splits of the first set, in the contract order: "total W", then "split COUNT hex words"
//   split_lists_host rf FILE [quiet]   host_rf in the mode's layout and the time it took; "quiet" prints the sum instead
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "split_sets.hpp"

using namespace mpf::splitsets;

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Stored {
  std::vector<int32_t> backs, n_inner, first, nbr;
  TreeSet set;
};

struct Input {
  int n = 0, mode = 0;
  Stored a, b;
  std::vector<int32_t> weights;
  bool has_weights = false;
};

static bool read_ints(std::ifstream &in, std::vector<int32_t> &v, size_t k)
{
  v.assign(k, 0);
  if (k) in.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(k * sizeof(int32_t)));
  return (bool)in;
}

static bool read_set(std::ifstream &in, int n, int n_records, int n_lists, Stored &s)
{
  if (!read_ints(in, s.backs, (size_t)n_records * 3 * (size_t)(2 * n - 1)) || !read_ints(in, s.n_inner, (size_t)n_lists)) return false;
  size_t nf = 0;
  for (int32_t m : s.n_inner) {
    if (m < 0 || m > (1 << 20)) return false;
    nf += (size_t)m + 1;
  }
  if (!read_ints(in, s.first, nf)) return false;
  // the file says how long every nbr[] is: the last entry of the tree's first[]
  size_t nn = 0, at = 0;
  for (int32_t m : s.n_inner) {
    const int32_t e = s.first[at + (size_t)m];
    if (e < 0 || e > (1 << 24)) return false;
    nn += (size_t)e;
    at += (size_t)m + 1;
  }
  if (!read_ints(in, s.nbr, nn)) return false;
  s.set.n_records = n_records;
  s.set.backs = n_records ? s.backs.data() : nullptr;
  s.set.n_lists = n_lists;
  s.set.n_inner = n_lists ? s.n_inner.data() : nullptr;
  s.set.first = n_lists ? s.first.data() : nullptr;
  s.set.nbr = n_lists ? s.nbr.data() : nullptr;
  return true;
}

static bool read_input(const char *path, Input &x)
{
  std::ifstream in(path, std::ios::binary);
  int32_t head[7] = {0, 0, 0, 0, 0, 0, 0};
  in.read(reinterpret_cast<char *>(head), sizeof(head));
  if (!in || head[0] < 3 || head[0] > (1 << 20) || head[3] < 0 || head[4] < 0 || head[5] < 0 || head[6] < 0) { std::fprintf(stderr, "bad header\n"); return false; }
  x.n = head[0];
  x.mode = head[1];
  x.has_weights = head[2] != 0;
  if (!read_set(in, x.n, head[3], head[4], x.a) || !read_set(in, x.n, head[5], head[6], x.b) ||
      (x.has_weights && !read_ints(in, x.weights, (size_t)head[3] + (size_t)head[4]))) {
    std::fprintf(stderr, "short file\n");
    return false;
  }
  return true;
}

template <class V>
static void print_list(const std::string &name, const V &v)
{
  std::printf("%s", name.c_str());
  for (const auto &e : v) std::printf(" %lld", (long long)e);
  std::printf("\n");
}

// the list trees of the first set one by one; a tree whose sizes cannot be those of a tree ends the loop (the next one cannot be found)
static int each_list(const Input &x, bool walk)
{
  std::vector<TreeRef> refs;
  const int stop = set_refs(x.n, x.a.set, refs);
  for (size_t t = (size_t)x.a.set.n_records; t < refs.size(); t++) {
    const TreeRef &r = refs[t];
    const std::string name = "list " + std::to_string(t - (size_t)x.a.set.n_records);
    if (!walk) {
      std::string why;
      if (lists_ok(x.n, r.n_inner, r.first, r.nbr, &why)) std::printf("%s ok\n", name.c_str());
      else std::printf("%s bad: %s\n", name.c_str(), why.c_str());
      continue;
    }
    TreeClusters c;
    if (!walk_clusters_lists(x.n, r.n_inner, r.first, r.nbr, c)) { std::printf("%s bad\n", name.c_str()); continue; }
    print_list(name + " order", c.order);
    print_list(name + " pos", c.pos);
    for (int ci = 0; ci < c.size(); ci++) std::printf("%s cluster %d %d %d\n", name.c_str(), c.lo[(size_t)ci], c.hi[(size_t)ci], c.node[(size_t)ci]);
  }
  if (stop >= 0) std::printf("list %d bad: n_inner or first[] are not those of a tree\n", stop);
  return 0;
}

static int run_counts(const Input &x)
{
  SplitTable t;
  int bad_tree = -1;
  if (!count_splits(x.n, x.a.set, x.has_weights ? x.weights.data() : nullptr, t, &bad_tree)) {
    std::fprintf(stderr, "tree %d is not a complete tree\n", bad_tree);
    return 3;
  }
  apply_order(t, order_splits(t));
  std::printf("total %lld\n", (long long)t.total);
  for (size_t i = 0; i < t.size(); i++) {
    std::printf("split %lld", (long long)t.count[i]);
    for (int j = 0; j < t.words; j++) std::printf(" %08x", t.row(i)[j]);
    std::printf("\n");
  }
  return 0;
}

static int run_rf(const Input &x, bool quiet)
{
  std::vector<int32_t> out;
  int bad_tree = -1;
  const double t0 = now_ms();
  if (!host_rf(x.n, x.mode, x.a.set, x.b.set, out, &bad_tree)) {
    if (bad_tree >= 0) { std::fprintf(stderr, "tree %d is not a complete tree\n", bad_tree); return 3; }
    std::fprintf(stderr, "unknown mode %d\n", x.mode);
    return 2;
  }
  const double t1 = now_ms();
  if (quiet) {
    long long sum = 0;
    for (int32_t v : out) sum += v;
    std::printf("entries %zu\nsum %lld\n", out.size(), sum);
  } else
    print_list("rf", out);
  std::printf("ms_rf %.3f\n", t1 - t0);
  return 0;
}

int main(int argc, char **argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  const bool known = cmd == "check" || cmd == "walk" || cmd == "counts" || cmd == "rf";
  if (!known || argc < 3 || argc > 4 || (argc == 4 && (cmd != "rf" || std::string(argv[3]) != "quiet"))) {
    std::fprintf(stderr, "usage: %s check FILE | walk FILE | counts FILE | rf FILE [quiet]\n", argv[0]);
    return 2;
  }
  Input x;
  if (!read_input(argv[2], x)) return 2;
  if (cmd == "check") return each_list(x, false);
  if (cmd == "walk") return each_list(x, true);
  if (cmd == "counts") return run_counts(x);
  return run_rf(x, argc == 4);
}
