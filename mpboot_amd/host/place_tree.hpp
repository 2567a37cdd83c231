// place_tree.hpp -- the device-free part of taxon insertion (host/place.cpp; place_host_main.cpp tests it under the sanitizers).
//
// Reference: PhyloTree::addTaxonMPFast (phylotree.cpp:1322-1378) tries a taxon on every branch in a pre-order walk from the root
// leaf -- first (root leaf, its neighbour), then FOR_NEIGHBOR_IT(node, dad, it) in neighbors[] order -- and keeps the FIRST
// strictly smallest score.  PhyloTree::computeParsimonyTree (phylotree.cpp:1243-1320) grows a tree that way in a
// my_random_shuffle order (tools.h:2107-2113), and the way it rewires neighbors[] decides the next step's walk.
//
// A backbone comes as the CSR neighbour lists of the polytomy calls (tips 1 .. n, inner node i = node n + 1 + i with neighbours
// nbr[first[i] .. first[i + 1]) in the host's neighbors[] order) with one relaxation: tips may be absent.  Check and walk are those of
// list_tree.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "list_tree.hpp"

namespace mpf {
namespace placetree {

enum { PT_OK = 0, PT_INVALID = 1, PT_UNSUPPORTED = 2 };

using Walk = listtree::Shape;                   // the rooted shape; its 2 m - 3 branches in walk order: listtree::branches

// The hand-over check (listtree::check, tips may be absent) and the rule of insertion alone.  PT_INVALID: not a tree over a subset
// of the tips with root_taxon among them (three or more occur: every inner node of a tree that passes has three or more
// neighbours); PT_UNSUPPORTED: a tree, but some inner node has a degree other than 3 (the k-ary Fitch rule depends on the root, and
// an insertion cost on such a tree is not what any reference function computes)
inline int check(int n, int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, Walk &w, std::string &err)
{
  std::string why;
  if (!listtree::check(n, n_inner, first, nbr, root_taxon, true, w, &why)) { err = "backbone tree: " + why; return PT_INVALID; }
  for (int i = 0; i < n_inner; i++)
    if (first[i + 1] - first[i] != 3) {
      err = "backbone tree: an inner node of degree " + std::to_string(first[i + 1] - first[i]) + " (insertion costs are defined on binary trees)";
      return PT_UNSUPPORTED;
    }
  return PT_OK;
}

// addTaxonMPFast keeps a later branch only with score < best_score: the first minimum in walk order
inline int first_min(const uint32_t *row, int nb)
{
  int at = 0;
  for (int b = 1; b < nb; b++)
    if (row[b] < row[at]) at = b;
  return at;
}

// The insertion of computeParsimonyTree on the lists: the new inner node (number n + 1 + old n_inner, its list appended) takes
// the place of node1 in node2's list and of node2 in node1's list, in place, and gets neighbors = [tip, node2, node1]
// (target_node = node2, the far end; target_dad = node1).  false: (node1, node2) is no branch of the lists
inline bool insert_tip(int n, std::vector<int32_t> &first, std::vector<int32_t> &nbr, int tip, int node1, int node2)
{
  const int n_inner = (int)first.size() - 1, v = n + 1 + n_inner;
  int hits = 0;
  auto replace = [&](int at, int what) {
    if (at <= n) return;
    const int i = at - n - 1;
    if (i >= n_inner) return;
    for (int k = first[(size_t)i]; k < first[(size_t)i + 1]; k++)
      if (nbr[(size_t)k] == what) { nbr[(size_t)k] = v; hits++; return; }
  };
  replace(node2, node1);
  replace(node1, node2);
  if (hits != (node1 > n) + (node2 > n) || hits == 0) return false;
  nbr.push_back(tip);
  nbr.push_back(node2);
  nbr.push_back(node1);
  first.push_back((int32_t)nbr.size());
  return true;
}

// my_random_shuffle (tools.h:2107-2113) over the identity: for i = n - 1 .. 1 swap(order[i], order[random_int(i + 1)]), random_int(k)
// = floor(random_double() * k) (tools.cpp:3353) on the SPRNG lcg64 stream handed over by state (host/rng.hpp restates it)
inline void shuffle_order(int n, uint64_t &state, int32_t *order)
{
  for (int i = 0; i < n; i++) order[i] = i + 1;
  for (int i = n - 1; i >= 1; i--) {
    state = state * 0x27bb2ee687b0b0fdULL + 3037000493ULL;
    const double r = (double)state * 5.4210108624275222e-20;
    std::swap(order[i], order[(int)(r * (double)(i + 1))]);
  }
}

// the star of the first three: its centre (inner node 0) has neighbors = [order[0], order[1], order[2]]
inline void star(const int32_t *order, std::vector<int32_t> &first, std::vector<int32_t> &nbr)
{
  first.assign({0, 3});
  nbr.assign({order[0], order[1], order[2]});
}

// Plain host costs on one core, for checks and timing: vectors are S rows of W 32-site words (the engine's row-major layout,
// padding bits set in every row), tips[(u - 1) * S * W ..].  delta[q * nb + b] as k_place_costs makes it; *tree_length by Fitch
// from the root leaf.  The lists must have passed check()
inline void host_costs(int n, int S, int W, const uint32_t *tips, int n_inner, const int32_t *first, const int32_t *nbr, const Walk &w,
                       int n_query, const int32_t *queries, std::vector<uint32_t> &delta, uint32_t *tree_length)
{
  const size_t V = (size_t)S * (size_t)W, N = (size_t)n + (size_t)n_inner;
  // up[v]: the view of v towards its parent; down[v]: the rest of the tree seen from v (towards v)
  std::vector<uint32_t> up((N + 1) * V), down((N + 1) * V);
  uint32_t len = 0;
  auto join = [&](const uint32_t *a, const uint32_t *b, uint32_t *o, bool count) {
    for (int x = 0; x < W; x++) {
      uint32_t any = 0;
      for (int s = 0; s < S; s++) any |= a[(size_t)s * W + x] & b[(size_t)s * W + x];
      for (int s = 0; s < S; s++) {
        const uint32_t p = a[(size_t)s * W + x], q = b[(size_t)s * W + x];
        o[(size_t)s * W + x] = (p & q) | (~any & (p | q));
      }
      if (count) len += (uint32_t)__builtin_popcount(~any);
    }
  };
  const int root = w.order[0];
  auto kids = [&](int v, int out[2]) {
    int c = 0;
    for (int k = first[v - n - 1]; k < first[v - n]; k++)
      if (nbr[k] != w.parent[(size_t)v]) out[c++] = nbr[k];
  };
  for (size_t i = w.order.size(); i-- > 1;) {
    const int v = w.order[i];
    if (v <= n) { std::copy(tips + (size_t)(v - 1) * V, tips + (size_t)v * V, &up[(size_t)v * V]); continue; }
    int c[2];
    kids(v, c);
    join(&up[(size_t)c[0] * V], &up[(size_t)c[1] * V], &up[(size_t)v * V], true);
  }
  {
    std::vector<uint32_t> tmp(V);
    join(tips + (size_t)(root - 1) * V, &up[(size_t)w.order[1] * V], tmp.data(), true);
  }
  std::copy(tips + (size_t)(root - 1) * V, tips + (size_t)root * V, &down[(size_t)w.order[1] * V]);
  for (size_t i = 1; i < w.order.size(); i++) {
    const int v = w.order[i];
    if (v <= n) continue;
    int c[2];
    kids(v, c);
    join(&down[(size_t)v * V], &up[(size_t)c[1] * V], &down[(size_t)c[0] * V], false);
    join(&down[(size_t)v * V], &up[(size_t)c[0] * V], &down[(size_t)c[1] * V], false);
  }
  if (tree_length) *tree_length = len;
  const size_t nb = w.order.size() - 1;
  delta.assign((size_t)n_query * nb, 0u);
  std::vector<uint32_t> x(V);
  for (size_t b = 0; b < nb; b++) {
    const int v = w.order[b + 1];                // branch b ends at the b-th node behind the root leaf
    join(&down[(size_t)v * V], &up[(size_t)v * V], x.data(), false);
    for (int q = 0; q < n_query; q++) {
      const uint32_t *t = tips + (size_t)(queries[q] - 1) * V;
      uint32_t d = 0;
      for (int k = 0; k < W; k++) {
        uint32_t any = 0;
        for (int s = 0; s < S; s++) any |= x[(size_t)s * W + k] & t[(size_t)s * W + k];
        d += (uint32_t)__builtin_popcount(~any);
      }
      delta[(size_t)q * nb + b] = d;
    }
  }
}

}  // namespace placetree
}  // namespace mpf
