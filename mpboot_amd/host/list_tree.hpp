// list_tree.hpp -- everything that follows from a tree's CSR neighbour lists alone: no device code, no engine, so that it can be
// compiled into a stand-alone program and run under a sanitizer (host/list_tree_main.cpp, tests/test_list_tree_host.py).
//
// The hand-over (include/mpfitch.h): tips are nodes 1 .. n, inner node i (0-based) is node n + 1 + i with the neighbours
// nbr[first[i] .. first[i + 1]) in the host's neighbors[] order.  The polytomy calls, the split and Robinson-Foulds calls on mixed
// sets, the consensus tree and taxon insertion all read such a tree through this header:
//
//   check         THE statement of the hand-over conditions, with the rooted shape (parent, pre-order) as a by-product
//   branches      the branches in the pre-order walk from the root leaf, neighbours in list order (fixNegativeBranch's and
//                 addTaxonMPFast's walk: FOR_NEIGHBOR_IT(node, dad, it))
//   list_root     the inner node next to tip 1
//   plan_views    the items of the one k_poly_views launch that makes the tree's directed views (polytomy.hip)
//   branch_sides  the two view slots of every branch
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace mpf {

// What k_poly_views / k_poly_snk_views read as uploaded (csrc/kernels.hpp describes the launch).  An item is one node's accumulation
// over inputs[in_begin .. in_begin + n_in) followed by its outputs outs[out_begin .. out_begin + n_out)
struct PolyItem { uint32_t in_begin, n_in, out_begin, n_out; };
struct PolyOut { uint32_t dst, excl, mask_row, pad; };
// the two directional vectors of a branch (k_branch_subst, k_snk_branch_eval, k_place_costs)
struct BranchDesc { uint32_t a, b; };

namespace listtree {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

struct Shape {
  int m = 0;                                   // tips that occur
  std::vector<int32_t> tip_nb, parent, order;  // tip_nb[u]: the inner neighbour of tip u (0: absent); parent (-1: an absent tip) and
                                               // pre-order from the root leaf, neighbours in list order
};

// The conditions of the hand-over: 1 <= n_inner <= n - 2, first[0] = 0, every inner degree >= 3, entries in range, no loop on a
// node, every tip at most once -- exactly once unless absent_tips (taxon insertion: a backbone over a subset of the tips) --,
// root_taxon among them, symmetric adjacency without doubles, tips + n_inner - 1 edges, one connected tree.  why (may be null):
// what is wrong; the caller names the tree in front of it
inline bool check(int n, int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, bool absent_tips, Shape &t,
                  std::string *why = nullptr)
{
  auto no = [&](const std::string &w) { if (why) *why = w; return false; };
  if (!first || !nbr) return no("null neighbour lists");
  if (n_inner < 1 || n_inner > n - 2) return no("n_inner must be in 1 .. n_taxa - 2");
  if (root_taxon < 1 || root_taxon > n) return no("root_taxon must be in 1 .. n_taxa");
  if (first[0] != 0) return no("first[0] must be 0");
  const int N = n + n_inner;
  for (int i = 0; i < n_inner; i++)
    if ((int64_t)first[i + 1] - (int64_t)first[i] < 3) return no("inner node " + std::to_string(n + 1 + i) + " has fewer than three neighbours");
  if ((int64_t)first[n_inner] > 3 * (int64_t)(n - 2)) return no("more neighbour entries than a tree of n_taxa leaves can have");
  t.tip_nb.assign((size_t)n + 1, 0);
  std::vector<std::pair<int32_t, int32_t>> arcs;       // inner -> inner, for the symmetry check
  for (int i = 0; i < n_inner; i++)
    for (int k = first[i]; k < first[i + 1]; k++) {
      const int u = nbr[k], v = n + 1 + i;
      if (u < 1 || u > N) return no("neighbour number out of range");
      if (u == v) return no("a node is its own neighbour");
      if (u <= n) {
        if (t.tip_nb[(size_t)u]) return no("tip " + std::to_string(u) + " occurs more than once");
        t.tip_nb[(size_t)u] = v;
      } else arcs.emplace_back(v, u);
    }
  t.m = 0;
  for (int u = 1; u <= n; u++) {
    if (t.tip_nb[(size_t)u]) t.m++;
    else if (!absent_tips) return no("tip " + std::to_string(u) + " does not occur");
  }
  if (!t.tip_nb[(size_t)root_taxon]) return no("root_taxon does not occur");
  std::sort(arcs.begin(), arcs.end());
  for (size_t i = 0; i < arcs.size(); i++) {
    if (i && arcs[i] == arcs[i - 1]) return no("a neighbour is listed twice");
    if (!std::binary_search(arcs.begin(), arcs.end(), std::make_pair(arcs[i].second, arcs[i].first))) return no("adjacency is not symmetric");
  }
  if ((int64_t)t.m + (int64_t)arcs.size() / 2 != (int64_t)t.m + n_inner - 1) return no("not tips + n_inner - 1 edges");
  // pre-order from the root leaf; with that many edges: one tree iff the walk meets no node twice and reaches every node
  t.parent.assign((size_t)N + 1, -1);
  t.order.clear();
  t.order.reserve((size_t)t.m + (size_t)n_inner);
  t.parent[(size_t)root_taxon] = 0;
  t.order.push_back(root_taxon);
  std::vector<int32_t> st{t.tip_nb[(size_t)root_taxon]};
  t.parent[(size_t)st[0]] = root_taxon;
  while (!st.empty()) {
    const int v = st.back();
    st.pop_back();
    t.order.push_back(v);
    if (v <= n) continue;
    const int i = v - n - 1;
    for (int k = first[i + 1] - 1; k >= first[i]; k--) {
      const int u = nbr[k];
      if (u == t.parent[(size_t)v]) continue;
      if (t.parent[(size_t)u] >= 0) return no("the neighbour lists hold a cycle");
      t.parent[(size_t)u] = v;
      st.push_back(u);
    }
  }
  if ((int)t.order.size() != t.m + n_inner) return no("the tree is not connected");
  return true;
}

// the 2 m - 3 (any inner degree: m + n_inner - 1) branches (parent[v], v) for v in walk order behind the root leaf, node1 the root
// side.  B: any {node1, node2} pair of int32_t (Branch, Engine::NniBranch)
struct Branch { int32_t node1, node2; };
template <class B>
inline void branches(const Shape &t, std::vector<B> &br)
{
  br.clear();
  for (size_t q = 1; q < t.order.size(); q++) br.push_back(B{t.parent[(size_t)t.order[q]], t.order[q]});
}

// the inner node next to tip 1 (0: tip 1 is in no list).  For lists that have passed no check: every index is checked
inline int list_root(int n, int n_inner, const int32_t *first, const int32_t *nbr)
{
  const int E = first[n_inner];
  for (int i = 0; i < n_inner; i++) {
    if (first[i] < 0 || first[i + 1] > E) return 0;
    for (int k = first[i]; k < first[i + 1]; k++)
      if (nbr[k] == 1) return n + 1 + i;
  }
  return 0;
}

// The view launch of a checked tree.  Slots: a tip keeps its own (u - 1); the view of inner node i towards its k-th neighbour (list
// position first[i] + k) is n + first[i] + k.  Items by level, lev_off[0 .. n_lev]: [0, maxh) up views by height - 1; maxh: the
// root edge (Fitch); maxh + 1 + depth: down views (all_views)
struct ViewPlan {
  std::vector<PolyItem> items;
  std::vector<PolyOut> outs;
  std::vector<uint32_t> inputs, up_slot;       // up_slot[v]: the view of v towards its parent (a tip: its own vector)
  std::vector<int32_t> lev_off;
  int n_rows = 0;                              // step-mask rows (Fitch): one per up view + the root edge
  int n_lev = 0;
};

// all_views: the down views too (every branch needs both sides); fitch: step masks and the root edge's item (the weighted engine
// evaluates the root edge with a kernel of its own).  false: the shape is not that of these lists
inline bool plan_views(int n, int n_inner, const int32_t *first, const int32_t *nbr, const Shape &t, bool all_views, bool fitch, ViewPlan &p)
{
  const int N = n + n_inner, root_taxon = t.order[0];
  // the parent's position in every inner node's list, and every inner node's position in its parent's list
  std::vector<int32_t> ppos((size_t)N + 1, -1), cpos((size_t)N + 1, -1), height((size_t)N + 1, 0), depth((size_t)N + 1, 0);
  for (int v = n + 1; v <= N; v++) {
    const int i = v - n - 1;
    for (int k = first[i]; k < first[i + 1]; k++) {
      const int u = nbr[k];
      if (u == t.parent[(size_t)v]) ppos[(size_t)v] = k;
      else if (u > n && t.parent[(size_t)u] == v) cpos[(size_t)u] = k;
    }
    if (ppos[(size_t)v] < 0) return false;
  }
  int maxh = 0, maxd = 0;
  for (size_t q = t.order.size(); q-- > 0;) {
    const int v = t.order[q];
    if (v == root_taxon) continue;
    const int par = t.parent[(size_t)v];
    if (par != root_taxon) height[(size_t)par] = std::max(height[(size_t)par], height[(size_t)v] + 1);
    maxh = std::max(maxh, height[(size_t)v]);
  }
  for (int v : t.order) {
    if (v <= n || t.parent[(size_t)v] == root_taxon) continue;
    depth[(size_t)v] = depth[(size_t)t.parent[(size_t)v]] + 1;
    maxd = std::max(maxd, depth[(size_t)v]);
  }
  const int r0 = t.tip_nb[(size_t)root_taxon];
  p.n_lev = all_views ? maxh + 2 + maxd : maxh + 1;
  std::vector<int32_t> lev_cnt((size_t)p.n_lev + 1, 0);
  auto up_level = [&](int v) { return height[(size_t)v] - 1; };
  auto down_level = [&](int v) { return maxh + 1 + depth[(size_t)v]; };
  for (int v = n + 1; v <= N; v++) {
    lev_cnt[(size_t)up_level(v)]++;
    if (all_views) lev_cnt[(size_t)down_level(v)]++;
  }
  if (fitch) lev_cnt[(size_t)maxh]++;
  p.lev_off.assign((size_t)p.n_lev + 1, 0);
  for (int l = 0; l < p.n_lev; l++) p.lev_off[(size_t)l + 1] = p.lev_off[(size_t)l] + lev_cnt[(size_t)l];
  p.items.assign((size_t)p.lev_off[(size_t)p.n_lev], PolyItem{0, 0, 0, 0});
  p.outs.clear();
  p.inputs.clear();
  std::vector<int32_t> fill(p.lev_off.begin(), p.lev_off.end() - 1);
  p.n_rows = 0;
  p.up_slot.assign((size_t)N + 1, kNoSlot);
  for (int v = 1; v <= n; v++) p.up_slot[(size_t)v] = (uint32_t)(v - 1);
  for (int v = n + 1; v <= N; v++) p.up_slot[(size_t)v] = (uint32_t)(n + ppos[(size_t)v]);
  // the view of v's k-th neighbour u TOWARDS v (an input of v): a tip's own vector, the up view of a child, the down view of the
  // parent -- the latter sits at the parent's entry for v
  auto input_of = [&](int v, int k) -> uint32_t {
    const int u = nbr[k];
    if (u <= n) return (uint32_t)(u - 1);
    if (u == t.parent[(size_t)v]) return (uint32_t)(n + cpos[(size_t)v]);
    return p.up_slot[(size_t)u];
  };
  for (int v = n + 1; v <= N; v++) {
    const int i = v - n - 1;
    // up: the rule over the children, one output towards the parent; its step mask is a row of the tree's per-site count
    PolyItem up{(uint32_t)p.inputs.size(), 0, (uint32_t)p.outs.size(), 1};
    for (int k = first[i]; k < first[i + 1]; k++)
      if (k != ppos[(size_t)v]) p.inputs.push_back(input_of(v, k));
    up.n_in = (uint32_t)p.inputs.size() - up.in_begin;
    p.outs.push_back(PolyOut{p.up_slot[(size_t)v], kNoSlot, fitch ? (uint32_t)p.n_rows++ : kNoSlot, 0});
    p.items[(size_t)fill[(size_t)up_level(v)]++] = up;
    if (!all_views) continue;
    // down: accumulators over all d inputs, one output towards every child (the rule over the other d - 1 inputs)
    PolyItem dn{(uint32_t)p.inputs.size(), 0, (uint32_t)p.outs.size(), 0};
    for (int k = first[i]; k < first[i + 1]; k++) p.inputs.push_back(input_of(v, k));
    dn.n_in = (uint32_t)p.inputs.size() - dn.in_begin;
    for (int k = first[i]; k < first[i + 1]; k++)
      if (k != ppos[(size_t)v]) p.outs.push_back(PolyOut{(uint32_t)(n + k), input_of(v, k), kNoSlot, 0});
    dn.n_out = (uint32_t)p.outs.size() - dn.out_begin;
    p.items[(size_t)fill[(size_t)down_level(v)]++] = dn;
  }
  if (fitch) {
    // computeParsimonyBranch(root->neighbors[0], root): the root leaf against the rest of the tree, a two-input node that stores
    // no vector
    PolyItem re{(uint32_t)p.inputs.size(), 2, (uint32_t)p.outs.size(), 1};
    p.inputs.push_back((uint32_t)(root_taxon - 1));
    p.inputs.push_back(p.up_slot[(size_t)r0]);
    p.outs.push_back(PolyOut{kNoSlot, kNoSlot, (uint32_t)p.n_rows++, 0});
    p.items[(size_t)fill[(size_t)maxh]++] = re;
  }
  return true;
}

// sides[b] = {sub, rest} of branch b of branches(): sub the subtree at node2 (its up view; a leaf: its own vector), rest the rest of
// the tree seen from node2 (node1's down view towards it, at node1's list entry for node2; a leaf node1: its own vector).  The plan
// must hold all views.  sides: room for order.size() - 1.  false: the shape is not that of these lists
inline bool branch_sides(int n, int n_inner, const int32_t *first, const int32_t *nbr, const Shape &t, const ViewPlan &p, BranchDesc *sides)
{
  std::vector<uint32_t> down((size_t)n + (size_t)n_inner + 1, kNoSlot);
  for (int i = 0; i < n_inner; i++)
    for (int k = first[i]; k < first[i + 1]; k++)
      if (t.parent[(size_t)nbr[k]] == n + 1 + i) down[(size_t)nbr[k]] = (uint32_t)(n + k);
  for (size_t q = 1; q < t.order.size(); q++) {
    const int v2 = t.order[q], v1 = t.parent[(size_t)v2];
    const uint32_t rest = v1 <= n ? (uint32_t)(v1 - 1) : down[(size_t)v2], sub = p.up_slot[(size_t)v2];
    if (rest == kNoSlot || sub == kNoSlot) return false;
    sides[q - 1] = BranchDesc{sub, rest};
  }
  return true;
}

}  // namespace listtree
}  // namespace mpf
