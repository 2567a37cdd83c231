// place_host_main.cpp -- the device-free part of taxon insertion (place_tree.hpp) as a stand-alone program: the tests build it with
// -fsanitize=address,undefined and run it as a child process; tools/place_timing.py builds it at -O2 for the one-core host costs.
//
//   place_host check FILE      the relaxed check: "ok" + the branches in walk order, or "invalid: ..." / "unsupported: ..."
//   place_host costs FILE      host costs of every query on every branch: "length L", "row q c c c ..", "best q i", "seconds s"
//   place_host grow FILE       the query array holds (tip, node1, node2) triples: the lists after inserting them one by one
//   place_host firstmin FILE   the query array is one row of scores: the index addTaxonMPFast keeps
//   place_host shuffle N STATE my_random_shuffle over the identity: "order ..", "state s"
// FILE: int32 n, S, W, n_inner, root, Q, first[n_inner + 1], nbr[first[n_inner]], query[Q], then (costs) uint32 tips[n][S][W].
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "place_tree.hpp"

using namespace mpf::placetree;

namespace {

struct Input {
  int32_t n = 0, S = 0, W = 0, n_inner = 0, root = 0, Q = 0;
  std::vector<int32_t> first, nbr, query;
  std::vector<uint32_t> tips;
};

bool read_input(const char *path, bool want_tips, Input &in)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t h[6];
  bool ok = std::fread(h, sizeof(int32_t), 6, f) == 6;
  if (ok) {
    in.n = h[0]; in.S = h[1]; in.W = h[2]; in.n_inner = h[3]; in.root = h[4]; in.Q = h[5];
    ok = in.n >= 0 && in.n < (1 << 24) && in.n_inner >= 0 && in.n_inner < (1 << 24) && in.Q >= 0 && in.Q < (1 << 24) && in.S >= 0 && in.S <= 32 &&
         in.W >= 0 && in.W < (1 << 24);
  }
  if (ok) {
    in.first.resize((size_t)in.n_inner + 1);
    ok = std::fread(in.first.data(), sizeof(int32_t), in.first.size(), f) == in.first.size();
  }
  if (ok) {
    const int32_t E = in.first.back();
    ok = E >= 0 && E < (1 << 26);
    if (ok) {
      in.nbr.resize((size_t)E);
      ok = std::fread(in.nbr.data(), sizeof(int32_t), in.nbr.size(), f) == in.nbr.size();
    }
  }
  if (ok) {
    in.query.resize((size_t)in.Q);
    ok = std::fread(in.query.data(), sizeof(int32_t), in.query.size(), f) == in.query.size();
  }
  if (ok && want_tips) {
    in.tips.resize((size_t)in.n * (size_t)in.S * (size_t)in.W);
    ok = std::fread(in.tips.data(), sizeof(uint32_t), in.tips.size(), f) == in.tips.size();
  }
  std::fclose(f);
  return ok;
}

void print_list(const char *tag, const std::vector<int32_t> &v)
{
  std::printf("%s", tag);
  for (int32_t x : v) std::printf(" %d", x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char **argv)
{
  if (argc < 3) { std::fprintf(stderr, "usage: place_host check|costs|grow|firstmin FILE | shuffle N STATE\n"); return 2; }
  const std::string cmd = argv[1];
  if (cmd == "shuffle") {
    if (argc < 4) return 2;
    const int n = std::atoi(argv[2]);
    uint64_t state = std::strtoull(argv[3], nullptr, 10);
    if (n < 1 || n > (1 << 24)) return 2;
    std::vector<int32_t> order((size_t)n);
    shuffle_order(n, state, order.data());
    print_list("order", order);
    std::printf("state %llu\n", (unsigned long long)state);
    return 0;
  }
  Input in;
  if (!read_input(argv[2], cmd == "costs", in)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  if (cmd == "firstmin") {
    std::vector<uint32_t> row(in.query.begin(), in.query.end());
    std::printf("firstmin %d\n", row.empty() ? -1 : first_min(row.data(), (int)row.size()));
    return 0;
  }
  if (cmd == "grow") {
    for (size_t i = 0; i + 2 < in.query.size(); i += 3)
      if (!insert_tip(in.n, in.first, in.nbr, in.query[i], in.query[i + 1], in.query[i + 2])) { std::printf("no such branch\n"); return 0; }
    print_list("first", in.first);
    print_list("nbr", in.nbr);
    return 0;
  }
  Walk w;
  std::string err;
  const int verdict = check(in.n, in.n_inner, in.first.data(), in.nbr.data(), in.root, w, err);
  if (verdict) { std::printf("%s: %s\n", verdict == PT_UNSUPPORTED ? "unsupported" : "invalid", err.c_str()); return 0; }
  if (cmd == "check") {
    std::printf("ok\nbranches");
    std::vector<mpf::listtree::Branch> br;
    mpf::listtree::branches(w, br);
    for (const auto &b : br) std::printf(" %d %d", b.node1, b.node2);
    std::printf("\n");
    return 0;
  }
  if (cmd != "costs") return 2;
  for (int32_t q : in.query)
    if (q < 1 || q > in.n || w.tip_nb[(size_t)q]) { std::printf("invalid: query %d\n", q); return 0; }
  std::vector<uint32_t> delta;
  uint32_t len = 0;
  const auto t0 = std::chrono::steady_clock::now();
  host_costs(in.n, in.S, in.W, in.tips.data(), in.n_inner, in.first.data(), in.nbr.data(), w, in.Q, in.query.data(), delta, &len);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const size_t nb = w.order.size() - 1;
  std::printf("length %u\n", len);
  for (int q = 0; q < in.Q; q++) {
    std::printf("row %d", q);
    for (size_t b = 0; b < nb; b++) std::printf(" %u", len + delta[(size_t)q * nb + b]);
    std::printf("\nbest %d %d\n", q, first_min(&delta[(size_t)q * nb], (int)nb));
  }
  std::printf("seconds %.6f\n", sec);
  return 0;
}
