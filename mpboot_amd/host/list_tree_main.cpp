// list_tree_main.cpp -- what follows from a tree's neighbour lists alone (list_tree.hpp: the hand-over check, the walk, the view plan,
// the sides of every branch) as a stand-alone program: no device, no engine.  tests/test_list_tree_host.py builds it with
// -fsanitize=address,undefined, runs it as a child process and compares its output with the Python witnesses.
//
//   list_tree check FILE [absent]   listtree::check (absent: tips may be missing): "ok", "order ..", "parent .." (of nodes 1 .. N),
//                                   "branches a b a b .."; or "invalid: <why>"
//   list_tree place FILE            the same lists through placetree::check: "ok" | "invalid: .." | "unsupported: .."
//   list_tree plan FILE all|up fitch|weighted [absent]
//                                   listtree::plan_views, printed ("n_rows", "levels", "item", "out", "inputs", "up_slot") and, fitch,
//                                   carried out on the host in plain C++ -- level by level, item by item, the k-ary Fitch rule:
//                                   "length L"; with all views "subst s s .." per branch from branch_sides and, on a binary tree,
//                                   "row q c c .." per query
// FILE: the layout place_host_main.cpp reads -- int32 n, S, W, n_inner, root, Q, first[n_inner + 1], nbr[first[n_inner]], query[Q],
// then (plan) uint32 tips[n][S][W], padding bits set in every row.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "place_tree.hpp"

using namespace mpf;
using namespace mpf::listtree;

namespace {

struct Input {
  int32_t n = 0, S = 0, W = 0, n_inner = 0, root = 0, Q = 0;
  std::vector<int32_t> first, nbr, query;
  std::vector<uint32_t> tips;
};

template <class T>
bool read_vec(FILE *f, std::vector<T> &v, size_t k)
{
  v.resize(k);
  return !k || std::fread(v.data(), sizeof(T), k, f) == k;
}

bool read_input(const char *path, bool want_tips, Input &in)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t h[6];
  bool ok = std::fread(h, sizeof(int32_t), 6, f) == 6;
  if (ok) {
    in.n = h[0]; in.S = h[1]; in.W = h[2]; in.n_inner = h[3]; in.root = h[4]; in.Q = h[5];
    ok = in.n >= 0 && in.n < (1 << 20) && in.n_inner >= 0 && in.n_inner < (1 << 20) && in.Q >= 0 && in.Q < (1 << 20) && in.S >= 0 && in.S <= 32 &&
         in.W >= 0 && in.W < (1 << 20);
  }
  ok = ok && read_vec(f, in.first, (size_t)in.n_inner + 1);
  ok = ok && in.first.back() >= 0 && in.first.back() < (1 << 24) && read_vec(f, in.nbr, (size_t)in.first.back());
  ok = ok && read_vec(f, in.query, (size_t)in.Q);
  if (ok && want_tips) ok = read_vec(f, in.tips, (size_t)in.n * (size_t)in.S * (size_t)in.W);
  std::fclose(f);
  return ok;
}

template <class V>
void print_list(const char *tag, const V &v, size_t from = 0)
{
  std::printf("%s", tag);
  for (size_t i = from; i < v.size(); i++) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}

// The plan carried out: store[slot] = S rows of W words, the tips in front.  An output is the rule over the item's inputs other
// than the one in slot excl: their AND, or where that is empty in every row their OR and one step (the step mask)
void run_plan(const Input &in, const ViewPlan &p, std::vector<uint32_t> &store, std::vector<uint32_t> &masks)
{
  const size_t V = (size_t)in.S * (size_t)in.W;
  store.assign(((size_t)in.n + in.nbr.size()) * V, 0u);
  std::copy(in.tips.begin(), in.tips.end(), store.begin());
  masks.assign((size_t)p.n_rows * (size_t)in.W, 0u);
  std::vector<uint32_t> o(V);
  for (int l = 0; l < p.n_lev; l++)
    for (int32_t i = p.lev_off[(size_t)l]; i < p.lev_off[(size_t)l + 1]; i++) {
      const PolyItem it = p.items[(size_t)i];
      for (uint32_t q = 0; q < it.n_out; q++) {
        const PolyOut out = p.outs[it.out_begin + q];
        for (int x = 0; x < in.W; x++) {
          uint32_t any = 0, all[32], some[32];
          for (int s = 0; s < in.S; s++) {
            all[s] = 0xFFFFFFFFu;
            some[s] = 0;
            for (uint32_t k = 0; k < it.n_in; k++) {
              const uint32_t slot = p.inputs[it.in_begin + k];
              if (slot == out.excl) continue;
              const uint32_t w = store[(size_t)slot * V + (size_t)s * (size_t)in.W + (size_t)x];
              all[s] &= w;
              some[s] |= w;
            }
            any |= all[s];
          }
          for (int s = 0; s < in.S; s++) o[(size_t)s * (size_t)in.W + (size_t)x] = all[s] | (~any & some[s]);
          if (out.mask_row != kNoSlot) masks[(size_t)out.mask_row * (size_t)in.W + (size_t)x] = ~any;
        }
        if (out.dst != kNoSlot) std::copy(o.begin(), o.end(), store.begin() + (long)((size_t)out.dst * V));
      }
    }
}

// sites at which the two vectors share no state
uint32_t apart(const Input &in, const uint32_t *a, const uint32_t *b)
{
  uint32_t d = 0;
  for (int x = 0; x < in.W; x++) {
    uint32_t any = 0;
    for (int s = 0; s < in.S; s++) any |= a[(size_t)s * (size_t)in.W + (size_t)x] & b[(size_t)s * (size_t)in.W + (size_t)x];
    d += (uint32_t)__builtin_popcount(~any);
  }
  return d;
}

}  // namespace

int main(int argc, char **argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (argc < 3 || (cmd != "check" && cmd != "place" && cmd != "plan") || (cmd == "plan" && argc < 5)) {
    std::fprintf(stderr, "usage: list_tree check FILE [absent] | place FILE | plan FILE all|up fitch|weighted [absent]\n");
    return 2;
  }
  Input in;
  if (!read_input(argv[2], cmd == "plan", in)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  const bool absent = std::string(argv[argc - 1]) == "absent";
  Shape t;
  std::string why;
  if (cmd == "place") {
    const int verdict = placetree::check(in.n, in.n_inner, in.first.data(), in.nbr.data(), in.root, t, why);
    if (verdict) std::printf("%s: %s\n", verdict == placetree::PT_UNSUPPORTED ? "unsupported" : "invalid", why.c_str());
    else std::printf("ok\n");
    return 0;
  }
  if (!check(in.n, in.n_inner, in.first.data(), in.nbr.data(), in.root, absent, t, &why)) { std::printf("invalid: %s\n", why.c_str()); return 0; }
  std::vector<Branch> br;
  branches(t, br);
  if (cmd == "check") {
    std::printf("ok\n");
    print_list("order", t.order);
    print_list("parent", t.parent, 1);
    std::printf("branches");
    for (const Branch &b : br) std::printf(" %d %d", b.node1, b.node2);
    std::printf("\n");
    return 0;
  }
  const bool all_views = std::string(argv[3]) == "all", fitch = std::string(argv[4]) == "fitch";
  ViewPlan p;
  if (!plan_views(in.n, in.n_inner, in.first.data(), in.nbr.data(), t, all_views, fitch, p)) { std::printf("invalid: no plan\n"); return 0; }
  std::printf("n_rows %d\n", p.n_rows);
  print_list("levels", p.lev_off);
  for (const PolyItem &it : p.items) std::printf("item %u %u %u %u\n", it.in_begin, it.n_in, it.out_begin, it.n_out);
  for (const PolyOut &o : p.outs) std::printf("out %lld %lld %lld\n", o.dst == kNoSlot ? -1ll : (long long)o.dst, o.excl == kNoSlot ? -1ll : (long long)o.excl,
                                              o.mask_row == kNoSlot ? -1ll : (long long)o.mask_row);
  print_list("inputs", p.inputs);
  print_list("up_slot", p.up_slot, 1);
  if (!fitch) return 0;
  std::vector<uint32_t> store, masks;
  run_plan(in, p, store, masks);
  uint32_t len = 0;
  for (uint32_t w : masks) len += (uint32_t)__builtin_popcount(w);
  std::printf("length %u\n", len);
  if (!all_views) return 0;
  std::vector<BranchDesc> sides(br.size());
  if (!branch_sides(in.n, in.n_inner, in.first.data(), in.nbr.data(), t, p, sides.data())) { std::printf("invalid: no sides\n"); return 0; }
  const size_t V = (size_t)in.S * (size_t)in.W;
  std::printf("subst");
  for (const BranchDesc &d : sides) std::printf(" %u", apart(in, &store[(size_t)d.a * V], &store[(size_t)d.b * V]));
  std::printf("\n");
  for (int i = 0; i < in.n_inner; i++)
    if (in.first[(size_t)i + 1] - in.first[(size_t)i] != 3) return 0;
  // a binary backbone: the query's cost on a branch = the length + the sites at which it shares no state with the join of the sides
  for (int q = 0; q < in.Q; q++) {
    if (in.query[(size_t)q] < 1 || in.query[(size_t)q] > in.n || t.tip_nb[(size_t)in.query[(size_t)q]]) { std::printf("invalid: query %d\n", in.query[(size_t)q]); return 0; }
    std::printf("row %d", q);
    std::vector<uint32_t> x(V);
    for (const BranchDesc &d : sides) {
      const uint32_t *a = &store[(size_t)d.a * V], *b = &store[(size_t)d.b * V];
      for (int w = 0; w < in.W; w++) {
        uint32_t any = 0;
        for (int s = 0; s < in.S; s++) any |= a[(size_t)s * (size_t)in.W + (size_t)w] & b[(size_t)s * (size_t)in.W + (size_t)w];
        for (int s = 0; s < in.S; s++) {
          const uint32_t u = a[(size_t)s * (size_t)in.W + (size_t)w], v = b[(size_t)s * (size_t)in.W + (size_t)w];
          x[(size_t)s * (size_t)in.W + (size_t)w] = (u & v) | (~any & (u | v));
        }
      }
      std::printf(" %u", len + apart(in, x.data(), &store[(size_t)(in.query[(size_t)q] - 1) * V]));
    }
    std::printf("\n");
  }
  return 0;
}
