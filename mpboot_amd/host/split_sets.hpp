// split_sets.hpp -- the host-only part of the bootstrap summary (host/splits.cpp): no device code, no engine, so that it can be
// compiled into a stand-alone program and run under a sanitizer (host/splits_host_main.cpp, tests/test_splits_host.py).
//
// A split is the set of tips on the side of an inner branch that does NOT hold tip 1 (the normal form of trees.splits), kept as
// words = ceil(n / 32) 32-bit words: bit (t - 1) % 32 of word (t - 1) / 32 means tip t is in the set.  Sets are always compared
// as whole sets; the hash of SetIndex only picks a bucket.
//
//   walk_clusters     the walk of k_split_keys restated: DFS from tip 1, every inner branch an interval [lo, hi) of DFS positions
//   lists_ok          the hand-over conditions on a tree given as CSR neighbour lists (listtree::check of list_tree.hpp: root leaf 1, every tip)
//   walk_clusters_lists  the walk of k_split_keys_lists restated: the same intervals for a tree of any inner degree >= 3
//   TreeSet, TreeRef  a set that mixes record-format and list-form trees (the records first, then the lists), and one tree of it
//   SetIndex          exact set -> index map (the overflow list of k_split_count is resolved through it; so is count_splits)
//   count_splits      the whole summary on the host (the CPU yardstick of tools/splits_timing.py)
//   order_splits      the contract order: count descending, then the words ascending as unsigned, word 0 first
//   greedy_compatible SplitGraph::findMaxCompatibleSplits (reference splitgraph.cpp:615-648): walk the splits in that order and
//                     keep each one that is compatible with all kept so far; at most n - 3 non-trivial ones fit a tree
//   build_lists       the kept (pairwise compatible) sets as the CSR neighbour lists mpf_polytomy_* takes
//
// ... and of the Robinson-Foulds distances (Engine::rf_distances; host/rf_host_main.cpp, tests/test_rf_host.py):
//   overflow_columns  the clusters of the overflow list grouped as sets: a group of two or more gets a column of its own
//   rf_chunk_plan     the column chunks the incidence matrix is built and multiplied in
//   host_rf           MTreeSet::computeRFDist (reference mtreeset.cpp:484-660) on the host: one sorted list of split ids per tree,
//                     a merge per pair (the CPU yardstick of tools/rf_timing.py and a second witness)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "list_tree.hpp"

namespace mpf {
namespace splitsets {

inline int words_of(int n) { return (n + 31) / 32; }

// the engine's record convention: rec = 3 * node + slot, the ring of an inner node
inline int nxt(int r) { const int v = r / 3, s = r % 3; return 3 * v + (s + 1) % 3; }

// mpf_set_tree's check of a complete tree on n taxa: every record of tips 1 .. n and inner nodes n + 1 .. 2n - 2 linked both ways
inline bool links_ok(const int32_t *back, int n)
{
  const int len = 3 * (2 * n - 1);
  for (int v = 1; v <= 2 * n - 2; v++)
    for (int s = 0; s < (v <= n ? 1 : 3); s++) {
      const int r = 3 * v + s, b = back[r];
      if (b < 3 || b >= len || back[b] != r) return false;
    }
  return true;
}

struct TreeClusters {
  std::vector<int32_t> pos;     // [n]      DFS position of tip t at pos[t - 1]; tip 1 gets n - 1, outside every interval
  std::vector<int32_t> order;   // [n - 1]  the tip at each DFS position
  std::vector<int32_t> lo, hi;  // [n - 3]  cluster ci = the tips with lo <= pos < hi, ci in pre-order of the inner nodes
  std::vector<int32_t> node;    // [n - 3]  the inner node below the branch (the end away from tip 1)
  // (a list tree with m inner nodes: m - 1 clusters)
  int size() const { return (int)lo.size(); }
};

// The walk of k_split_keys, step for step: an explicit stack of records, a negative entry closes cluster -(x + 1).  The inner
// node next to tip 1 holds every other tip and is no split; it is entered first and gets no cluster.  false: the records do not
// form ONE tree over all n tips (the counts run over or fall short)
inline bool walk_clusters(const int32_t *back, int n, TreeClusters &c)
{
  const int C = n - 3;
  c.pos.assign((size_t)n, 0);
  c.order.assign((size_t)std::max(n - 1, 0), 0);
  c.lo.assign((size_t)std::max(C, 0), 0);
  c.hi.assign((size_t)std::max(C, 0), 0);
  c.node.assign((size_t)std::max(C, 0), 0);
  std::vector<int32_t> st;
  st.reserve((size_t)2 * n + 4);
  st.push_back(back[3]);
  int cnt = 0, inner = 0;
  while (!st.empty()) {
    const int x = st.back();
    st.pop_back();
    if (x < 0) { c.hi[(size_t)(-x - 1)] = cnt; continue; }
    const int v = x / 3;
    if (v <= n) {
      if (v == 1 || cnt >= n - 1) return false;
      c.pos[(size_t)v - 1] = cnt;
      c.order[(size_t)cnt++] = v;
      continue;
    }
    if (inner >= n - 2) return false;
    const int ci = inner++ - 1;
    if (ci >= 0) {
      c.lo[(size_t)ci] = cnt;
      c.node[(size_t)ci] = v;
      st.push_back(-(ci + 1));
    }
    st.push_back(back[nxt(nxt(x))]);
    st.push_back(back[nxt(x)]);
  }
  c.pos[0] = n - 1;
  return cnt == n - 1 && inner == n - 2;
}

// ---- trees as CSR neighbour lists (the hand-over of mpf_polytomy_*): tips 1 .. n, inner node i = node n + 1 + i with the
// neighbours nbr[first[i] .. first[i + 1])

// the largest stack walk_clusters_lists / k_split_keys_lists can need: every node waits there at most once, and every inner node
// but the first leaves one closing entry
inline size_t list_walk_stack(int n, int n_inner) { return (size_t)n + 2 * (size_t)n_inner + 2; }

// The conditions of the hand-over (listtree::check states them) for a tree of a set: every tip occurs, the root leaf is tip 1.
// why (may be null): what is wrong
inline bool lists_ok(int n, int n_inner, const int32_t *first, const int32_t *nbr, std::string *why = nullptr)
{
  listtree::Shape shape;
  return listtree::check(n, n_inner, first, nbr, 1, false, shape, why);
}

using listtree::list_root;

// The walk of k_split_keys_lists, step for step: an explicit stack of (node, dad) entries, children in list order, a negative
// entry closes cluster -(x + 1).  The inner node next to tip 1 is entered first and gets no cluster, so a tree with m inner nodes
// has m - 1 clusters; c.node[ci] is the inner node below cluster ci's branch.  Tips and inner nodes are met in the order of the
// branch walk of mpf_polytomy_branch_substitutions from root_taxon = 1.  Every index is checked and the walk is bounded by the
// node counts, as on the device.  false: the lists do not form ONE tree over all n tips
inline bool walk_clusters_lists(int n, int n_inner, const int32_t *first, const int32_t *nbr, TreeClusters &c)
{
  const int K = std::max(n_inner - 1, 0);
  c.pos.assign((size_t)n, 0);
  c.order.assign((size_t)std::max(n - 1, 0), 0);
  c.lo.assign((size_t)K, 0);
  c.hi.assign((size_t)K, 0);
  c.node.assign((size_t)K, 0);
  if (n < 3 || n_inner < 1 || n_inner > n - 2) return false;
  const int N = n + n_inner, E = first[n_inner];
  const size_t cap = list_walk_stack(n, n_inner);
  const int root = list_root(n, n_inner, first, nbr);
  if (!root) return false;
  struct F { int32_t node, dad; };
  std::vector<F> st;
  st.reserve(cap);
  st.push_back(F{root, 1});
  int cnt = 0, inner = 0;
  while (!st.empty()) {
    const F x = st.back();
    st.pop_back();
    if (x.node < 0) { c.hi[(size_t)(-x.node - 1)] = cnt; continue; }
    const int v = x.node;
    if (v < 1 || v > N) return false;
    if (v <= n) {
      if (v == 1 || cnt >= n - 1) return false;
      c.pos[(size_t)v - 1] = cnt;
      c.order[(size_t)cnt++] = v;
      continue;
    }
    if (inner >= n_inner) return false;
    const int f0 = first[v - n - 1], f1 = first[v - n];
    if (f0 < 0 || f1 < f0 || f1 > E || st.size() + (size_t)(f1 - f0) + 1 > cap) return false;
    const int ci = inner++ - 1;
    if (ci >= 0) {
      c.lo[(size_t)ci] = cnt;
      c.node[(size_t)ci] = v;
      st.push_back(F{-(ci + 1), 0});
    }
    for (int k = f1 - 1; k >= f0; k--)
      if (nbr[k] != x.dad) st.push_back(F{nbr[k], v});
  }
  c.pos[0] = n - 1;
  return cnt == n - 1 && inner == n_inner;
}

// A set that mixes the two forms, as the C-ABI hands it over (mpf_tree_set): the records first, then the lists.  The lists'
// first[] lie one behind the other (n_inner[t] + 1 entries each, each starting at 0), and so do their nbr[] (first[n_inner[t]] each)
struct TreeSet {
  int n_records = 0; const int32_t *backs = nullptr;
  int n_lists = 0;   const int32_t *n_inner = nullptr, *first = nullptr, *nbr = nullptr;
  int size() const { return std::max(n_records, 0) + std::max(n_lists, 0); }
  bool pointers_ok() const { return (n_records <= 0 || backs) && (n_lists <= 0 || (n_inner && first && nbr)); }
};
// one tree of a set: records (back != null) or lists
struct TreeRef {
  const int32_t *back = nullptr;
  int n_inner = 0; const int32_t *first = nullptr, *nbr = nullptr;
  bool is_list() const { return back == nullptr; }
  int clusters(int n) const { return is_list() ? std::max(n_inner - 1, 0) : std::max(n - 3, 0); }
};

// The trees of a set, appended to refs.  A list tree's place follows from the sizes of those before it, so the walk ends at the
// first list whose n_inner or first[n_inner] cannot be one of a tree on n taxa: its index within the lists comes back (-1: all found)
inline int set_refs(int n, const TreeSet &s, std::vector<TreeRef> &refs)
{
  const size_t len = 3 * (size_t)(2 * n - 1);
  for (int t = 0; t < s.n_records; t++) { TreeRef r; r.back = s.backs + (size_t)t * len; refs.push_back(r); }
  size_t fo = 0, no = 0;
  for (int t = 0; t < s.n_lists; t++) {
    const int m = s.n_inner[t];
    if (m < 1 || m > n - 2) return t;
    TreeRef r;
    r.n_inner = m;
    r.first = s.first + fo;
    r.nbr = s.nbr + no;
    const int64_t E = r.first[m];
    if (r.first[0] != 0 || E < 0 || E > 3 * (int64_t)(n - 2)) return t;
    refs.push_back(r);
    fo += (size_t)m + 1;
    no += (size_t)E;
  }
  return -1;
}

// checks and walk of one tree of either form.  false: not a complete tree on n taxa
inline bool tree_clusters(const TreeRef &r, int n, TreeClusters &c)
{
  if (r.is_list()) return lists_ok(n, r.n_inner, r.first, r.nbr) && walk_clusters_lists(n, r.n_inner, r.first, r.nbr, c);
  return links_ok(r.back, n) && walk_clusters(r.back, n, c);
}

inline void cluster_bits(const TreeClusters &c, int ci, int words, uint32_t *out)
{
  std::fill(out, out + words, 0u);
  for (int p = c.lo[(size_t)ci]; p < c.hi[(size_t)ci]; p++) {
    const int t = c.order[(size_t)p] - 1;
    out[t >> 5] |= 1u << (t & 31);
  }
}

// exact map from a set to its index in a table of sets kept by the caller; the hash routes, equality is word by word
class SetIndex {
 public:
  explicit SetIndex(int words) : words_(words) {}
  static uint64_t hash(const uint32_t *w, int words)
  {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < words; i++) { h ^= w[i]; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
    return h;
  }
  // index of `w` in table (rows of `words` words), or -1
  int64_t find(const std::vector<uint32_t> &table, const uint32_t *w) const
  {
    auto rg = map_.equal_range(hash(w, words_));
    for (auto it = rg.first; it != rg.second; ++it)
      if (!std::memcmp(table.data() + (size_t)it->second * (size_t)words_, w, (size_t)words_ * sizeof(uint32_t))) return it->second;
    return -1;
  }
  void insert(const uint32_t *w, int64_t index) { map_.emplace(hash(w, words_), index); }
  void reserve(size_t k) { map_.reserve(k); }

 private:
  int words_;
  std::unordered_multimap<uint64_t, int64_t> map_;
};

struct SplitTable {
  int n = 0, words = 0;
  int64_t total = 0;
  std::vector<uint32_t> bits;    // [count.size()][words]
  std::vector<int64_t> count;
  size_t size() const { return count.size(); }
  const uint32_t *row(size_t i) const { return bits.data() + i * (size_t)words; }
};

// MTreeSet::convertSplits (reference mtreeset.cpp:288-470) without the strings: every tree's splits into one table, weighted.
// weights (indexed as the set: records, then lists) may be null (all 1); a tree of weight 0 contributes nothing.  false: a tree is
// not a complete tree on n taxa (*bad_tree: which, in set order)
inline bool count_splits(int n, const TreeSet &set, const int32_t *weights, SplitTable &out, int *bad_tree = nullptr)
{
  out.n = n;
  out.words = words_of(n);
  out.total = 0;
  out.bits.clear();
  out.count.clear();
  std::vector<TreeRef> refs;
  const int stop = set_refs(n, set, refs);
  if (stop >= 0) { if (bad_tree) *bad_tree = set.n_records + stop; return false; }
  SetIndex idx(out.words);
  TreeClusters c;
  std::vector<uint32_t> w((size_t)out.words);
  for (size_t t = 0; t < refs.size(); t++) {
    const int64_t wt = weights ? weights[t] : 1;
    if (!tree_clusters(refs[t], n, c)) { if (bad_tree) *bad_tree = (int)t; return false; }
    if (wt == 0) continue;
    out.total += wt;
    for (int ci = 0; ci < c.size(); ci++) {
      cluster_bits(c, ci, out.words, w.data());
      int64_t k = idx.find(out.bits, w.data());
      if (k < 0) {
        k = (int64_t)out.count.size();
        out.bits.insert(out.bits.end(), w.begin(), w.end());
        out.count.push_back(0);
        idx.insert(w.data(), k);
      }
      out.count[(size_t)k] += wt;
    }
  }
  return true;
}
inline bool count_splits(int n, int n_trees, const int32_t *backs, const int32_t *weights, SplitTable &out)
{
  TreeSet s;
  s.n_records = n_trees;
  s.backs = backs;
  return count_splits(n, s, weights, out);
}

// the contract order: count descending, then the set's words ascending as unsigned, word 0 first
inline std::vector<int64_t> order_splits(const SplitTable &t)
{
  std::vector<int64_t> p(t.size());
  std::iota(p.begin(), p.end(), (int64_t)0);
  std::sort(p.begin(), p.end(), [&](int64_t a, int64_t b) {
    if (t.count[(size_t)a] != t.count[(size_t)b]) return t.count[(size_t)a] > t.count[(size_t)b];
    const uint32_t *x = t.row((size_t)a), *y = t.row((size_t)b);
    for (int i = 0; i < t.words; i++)
      if (x[i] != y[i]) return x[i] < y[i];
    return false;
  });
  return p;
}

inline void apply_order(SplitTable &t, const std::vector<int64_t> &p)
{
  std::vector<uint32_t> b(t.bits.size());
  std::vector<int64_t> c(t.count.size());
  for (size_t i = 0; i < p.size(); i++) {
    std::copy(t.row((size_t)p[i]), t.row((size_t)p[i]) + t.words, b.begin() + (long)(i * (size_t)t.words));
    c[i] = t.count[(size_t)p[i]];
  }
  t.bits.swap(b);
  t.count.swap(c);
}

// both sets leave tip 1 out, so their complements always meet: two splits fit one tree iff the sets are disjoint or nested
// (Split::compatible, reference split.cpp:170-193, with the fourth intersection never empty)
inline bool compatible(const uint32_t *a, const uint32_t *b, int words)
{
  uint32_t both = 0, a_only = 0, b_only = 0;
  for (int i = 0; i < words; i++) {
    both |= a[i] & b[i];
    a_only |= a[i] & ~b[i];
    b_only |= b[i] & ~a[i];
  }
  return !both || !a_only || !b_only;
}

// the reference's consensus rule on a table in the contract order: drop count <= threshold * total (mtreeset.cpp:301-312), then
// findMaxCompatibleSplits.  Returns the kept rows, in table order
inline std::vector<int64_t> greedy_compatible(const SplitTable &t, double threshold)
{
  std::vector<int64_t> kept;
  const double cut = threshold * (double)t.total;
  const size_t max_splits = t.n >= 3 ? (size_t)(t.n - 3) : 0;
  for (size_t i = 0; i < t.size() && kept.size() < max_splits; i++) {
    if ((double)t.count[i] <= cut) continue;
    bool ok = true;
    for (size_t k = 0; k < kept.size() && ok; k++) ok = compatible(t.row(i), t.row((size_t)kept[k]), t.words);
    if (ok) kept.push_back((int64_t)i);
  }
  return kept;
}

struct ListTree {
  std::vector<int32_t> first, nbr;
  std::vector<int64_t> support;      // the count of the split above each inner node, -1 for the first (it hangs on tip 1)
  int n_inner() const { return (int)first.size() - 1; }
};

// Tips 1 .. n; inner nodes n + 1 .. in pre-order from tip 1; each inner node lists its parent first, then its children by their
// smallest tip.  The kept sets are pairwise disjoint or nested, so taken by size descending each set's parent is the set that
// owns its tips at that moment (the smallest superset met so far; none: the node next to tip 1)
inline void build_lists(const SplitTable &t, const std::vector<int64_t> &kept, ListTree &out)
{
  const int n = t.n, K = (int)kept.size();
  std::vector<int> size((size_t)K, 0), by_size((size_t)K), min_tip((size_t)K + 1, n + 1);
  for (int k = 0; k < K; k++) {
    const uint32_t *w = t.row((size_t)kept[(size_t)k]);
    for (int i = 0; i < t.words; i++) size[(size_t)k] += __builtin_popcount(w[i]);
    by_size[(size_t)k] = k;
  }
  std::stable_sort(by_size.begin(), by_size.end(), [&](int a, int b) { return size[(size_t)a] > size[(size_t)b]; });
  // set K stands for the node next to tip 1
  std::vector<int> owner((size_t)n + 1, K), parent((size_t)K, K);
  for (int k : by_size) {
    const uint32_t *w = t.row((size_t)kept[(size_t)k]);
    bool seen = false;
    for (int tip = 2; tip <= n; tip++)
      if (w[(tip - 1) >> 5] >> ((tip - 1) & 31) & 1u) {
        if (!seen) { parent[(size_t)k] = owner[(size_t)tip]; min_tip[(size_t)k] = tip; seen = true; }
        owner[(size_t)tip] = k;
      }
  }
  min_tip[(size_t)K] = 2;
  // children of every set: (smallest tip, child), a child set as K + 1 + index so that tips and sets sort together by tip
  std::vector<std::vector<std::pair<int, int>>> kids((size_t)K + 1);
  for (int tip = 2; tip <= n; tip++) kids[(size_t)owner[(size_t)tip]].emplace_back(tip, -tip);
  for (int k = 0; k < K; k++) kids[(size_t)parent[(size_t)k]].emplace_back(min_tip[(size_t)k], k);
  for (auto &v : kids) std::sort(v.begin(), v.end());
  // pre-order numbering from tip 1
  std::vector<int> number((size_t)K + 1, 0), pre;
  std::vector<int> st{K};
  while (!st.empty()) {
    const int s = st.back();
    st.pop_back();
    number[(size_t)s] = n + 1 + (int)pre.size();
    pre.push_back(s);
    for (size_t i = kids[(size_t)s].size(); i-- > 0;)
      if (kids[(size_t)s][i].second >= 0) st.push_back(kids[(size_t)s][i].second);
  }
  out.first.assign(1, 0);
  out.nbr.clear();
  out.support.clear();
  for (int s : pre) {
    out.nbr.push_back(s == K ? 1 : number[(size_t)parent[(size_t)s]]);
    for (const auto &kd : kids[(size_t)s]) out.nbr.push_back(kd.second < 0 ? -kd.second : number[(size_t)kd.second]);
    out.first.push_back((int32_t)out.nbr.size());
    out.support.push_back(s == K ? -1 : t.count[(size_t)kept[(size_t)s]]);
  }
}

// ---- Robinson-Foulds distances

enum { RF_ALL_PAIRS = 0, RF_ADJACENT = 1, RF_TWO_SETS = 2 };

// sets[m][words]: the sets of the clusters on the overflow list (true key collisions: none of them is the set its table slot
// stands for, so none of them equals a split that has a device-numbered column).  Equal sets form a group; a group of two or more
// gets the next column from first_col on, in the order its first member appears; a set that stands alone gets none (-1): no pair
// of trees shares it.  Two clusters of one tree are different sets, so a group never holds one tree twice.  Returns the number of
// columns handed out
inline int64_t overflow_columns(const std::vector<uint32_t> &sets, size_t m, int words, int64_t first_col, std::vector<int64_t> &col)
{
  std::vector<int64_t> group(m, -1), size, first;
  std::vector<uint32_t> reps;
  SetIndex idx(words);
  idx.reserve(m);
  for (size_t i = 0; i < m; i++) {
    const uint32_t *w = sets.data() + i * (size_t)words;
    int64_t g = idx.find(reps, w);
    if (g < 0) {
      g = (int64_t)size.size();
      reps.insert(reps.end(), w, w + words);
      size.push_back(0);
      idx.insert(w, g);
    }
    size[(size_t)g]++;
    group[i] = g;
  }
  std::vector<int64_t> col_of_group(size.size(), -1);
  int64_t next = first_col;
  col.assign(m, -1);
  for (size_t i = 0; i < m; i++) {
    const size_t g = (size_t)group[i];
    if (size[g] < 2) continue;
    if (col_of_group[g] < 0) col_of_group[g] = next++;
    col[i] = col_of_group[g];
  }
  return next - first_col;
}

struct RfChunk { int64_t c0, c1; };
inline int64_t rf_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// The chunks [c0, c1) that cover columns 0 .. columns once, in order.  forced > 0: chunks of `forced` columns rounded up to a
// multiple of 32 (a test option).  Else the widest chunk whose matrix -- rows x words, the words of a row padded to k_step --
// stays within budget_bytes, at least k_step words.  Every chunk but the last is a multiple of 32 columns.  No columns: no chunk
inline std::vector<RfChunk> rf_chunk_plan(int64_t columns, int64_t rows, int64_t forced, int64_t budget_bytes, int64_t k_step)
{
  std::vector<RfChunk> plan;
  if (columns <= 0) return plan;
  int64_t per;
  if (forced > 0) per = rf_round_up(forced, 32);
  else {
    const int64_t words = std::max<int64_t>(k_step, budget_bytes / (4 * std::max<int64_t>(rows, 1)) / k_step * k_step);
    per = 32 * words;
  }
  for (int64_t c = 0; c < columns; c += per) plan.push_back(RfChunk{c, std::min(columns, c + per)});
  return plan;
}

// one tree's splits as a sorted list of ids into one exact table, appended to ids.  false: the tree is not a complete tree on n taxa
inline bool rf_id_list(int n, const TreeRef &r, SetIndex &idx, std::vector<uint32_t> &table, std::vector<int64_t> &ids)
{
  const int words = words_of(n);
  TreeClusters c;
  std::vector<uint32_t> w((size_t)words);
  if (!tree_clusters(r, n, c)) return false;
  const size_t at = ids.size();
  for (int ci = 0; ci < c.size(); ci++) {
    cluster_bits(c, ci, words, w.data());
    int64_t k = idx.find(table, w.data());
    if (k < 0) {
      k = (int64_t)(table.size() / (size_t)words);
      table.insert(table.end(), w.begin(), w.end());
      idx.insert(w.data(), k);
    }
    ids.push_back(k);
  }
  std::sort(ids.begin() + (long)at, ids.end());
  return true;
}

// MTreeSet::computeRFDist without the strings and without weights: the number of splits in one tree and not in the other,
// size(A) + size(B) - 2 common, for trees of either form (a fully resolved tree has n - 3 splits, a list tree with m inner nodes
// m - 1).  out: the layout of the mode (all pairs [T][T]; adjacent [T - 1]; two sets [T][T2]).  false: a tree is broken
// (*bad_tree: which, counted through both sets, each in set order) or the mode is unknown
inline bool host_rf(int n, int mode, const TreeSet &s1, const TreeSet &s2, std::vector<int32_t> &out, int *bad_tree = nullptr)
{
  const int words = words_of(n);
  SetIndex idx(words);
  std::vector<uint32_t> table;
  std::vector<int64_t> ids;
  std::vector<size_t> at{0};                         // tree t's ids: ids[at[t] .. at[t + 1])
  if (mode != RF_ALL_PAIRS && mode != RF_ADJACENT && mode != RF_TWO_SETS) return false;
  std::vector<TreeRef> refs;
  int stop = set_refs(n, s1, refs);
  if (stop >= 0) { if (bad_tree) *bad_tree = s1.n_records + stop; return false; }
  const int n_trees = (int)refs.size();
  if (mode == RF_TWO_SETS) {
    stop = set_refs(n, s2, refs);
    if (stop >= 0) { if (bad_tree) *bad_tree = n_trees + s2.n_records + stop; return false; }
  }
  const int n_trees2 = (int)refs.size() - n_trees;
  for (size_t t = 0; t < refs.size(); t++) {
    if (!rf_id_list(n, refs[t], idx, table, ids)) { if (bad_tree) *bad_tree = (int)t; return false; }
    at.push_back(ids.size());
  }
  auto dist = [&](int i, int j) {
    const int64_t *a = ids.data() + at[(size_t)i], *b = ids.data() + at[(size_t)j];
    const int na = (int)(at[(size_t)i + 1] - at[(size_t)i]), nb = (int)(at[(size_t)j + 1] - at[(size_t)j]);
    int shared = 0;
    for (int p = 0, q = 0; p < na && q < nb;) {
      if (a[p] == b[q]) { shared++; p++; q++; }
      else if (a[p] < b[q]) p++;
      else q++;
    }
    return (int32_t)(na + nb - 2 * shared);
  };
  out.clear();
  if (mode == RF_ALL_PAIRS) {
    out.assign((size_t)n_trees * (size_t)n_trees, 0);
    for (int i = 0; i < n_trees; i++)
      for (int j = i + 1; j < n_trees; j++) out[(size_t)i * (size_t)n_trees + (size_t)j] = out[(size_t)j * (size_t)n_trees + (size_t)i] = dist(i, j);
  } else if (mode == RF_ADJACENT) {
    for (int i = 0; i + 1 < n_trees; i++) out.push_back(dist(i, i + 1));
  } else {
    out.reserve((size_t)n_trees * (size_t)n_trees2);
    for (int i = 0; i < n_trees; i++)
      for (int j = 0; j < n_trees2; j++) out.push_back(dist(i, n_trees + j));
  }
  return true;
}
inline bool host_rf(int n, int mode, int n_trees, const int32_t *backs, int n_trees2, const int32_t *backs2, std::vector<int32_t> &out,
                    int *bad_tree = nullptr)
{
  TreeSet a, b;
  a.n_records = n_trees;
  a.backs = backs;
  b.n_records = n_trees2;
  b.backs = backs2;
  return host_rf(n, mode, a, b, out, bad_tree);
}

}  // namespace splitsets
}  // namespace mpf
