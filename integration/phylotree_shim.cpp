// phylotree_shim.cpp -- the IQ-TREE-level drop-in: PhyloTree::computeParsimony() (reference phylotree.cpp:1049-1061,
// virtual, phylotree.h:432) and its ParsTree override (parstree.cpp:101-116, parstree.h:50) on libmpfitch.so.
//
// Both classes stay opaque: the two members are DEFINED here under their Itanium-mangled names
//     _ZN9PhyloTree16computeParsimonyEv        int PhyloTree::computeParsimony()
//     _ZN8ParsTree16computeParsimonyEv         int ParsTree::computeParsimony()
// (an extern "C" function whose symbol IS the member's; `this` arrives as the first argument), so a mpboot build that
// drops the two bodies from phylotree.cpp / parstree.cpp and links this file + -lmpfitch gets every call site
// (iqtree.cpp:1772, :2143, :2558-2958; phyloanalysis.cpp:1309, :1737, :1865, :2790, :2811; phylotree.cpp:1704, :3258)
// and every virtual dispatch served by the engine.  Members are reached through integration/phylotree_hooks.h.
//
// Contract kept: returns the int score; side effect: _pattern_pars[0 .. nptn) = per-pattern
// lengths of the tree (phylotree.cpp:986-987), the VCSIZE_USHORT = 16 entries behind them zero (:956-957).  Patterns
// are NOT filtered: the IQ-TREE kernel scores every pattern x frequency, uninformative ones included (the engine is
// created with keep_all_sites = 1).  ParsTree with a cost matrix runs the weighted engine (mpf_engine_create_sankoff).
//
// Built and exercised without the reference: oracle/Makefile `shims` links it with oracle/phylotree_shim_driver.cpp (a
// stand-in class hierarchy that only DECLARES the two members) -> oracle/_build/phylotree_shim_driver, run on the GPU
// by tests/test_gpu_dropin.py.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include "phylotree_hooks.h"

namespace {

constexpr int kVcsizeUshort = 16;          // VCSIZE_USHORT (phyloanalysis.h / vectorclass: 16 unsigned shorts per AVX vector)

mpf_phylotree_hooks g_h;
bool g_installed = false;

struct Cached {
  mpf_engine *eng = nullptr;
  const void *aln = nullptr;
  unsigned long long stamp = 0;            // alignment_stamp at the last content check (when the hook exists)
  unsigned long long hash = 0;             // of the pattern states the engine was built from
  int n = 0, P = 0, protein = 0;
  std::vector<int32_t> freq;               // pattern frequencies in force in the engine
  std::vector<uint32_t> cost;              // empty = Fitch
};
Cached g_fitch, g_cost;                    // PhyloTree / unit-cost ParsTree, and ParsTree with a matrix

[[noreturn]] void die(const char *what)
{
  std::fprintf(stderr, "mpfitch phylotree shim: %s: %s\n", what, mpf_last_error());
  std::exit(EXIT_FAILURE);                 // the reference's outError() (tools.cpp) also exits
}

void drop(Cached &c)
{
  if (c.eng) mpf_engine_destroy(c.eng);
  c = Cached();
}

mpf_engine *engine_for(PhyloTree *t, const unsigned int *cost)
{
  if (!g_installed) { std::fprintf(stderr, "mpfitch phylotree shim: mpfitch_phylotree_install() was not called\n"); std::exit(EXIT_FAILURE); }
  const int n = g_h.n_taxa(t), P = g_h.n_patterns(t), protein = g_h.is_protein(t) ? 1 : 0;
  const int S = protein ? 20 : 4;
  Cached &c = cost ? g_cost : g_fitch;
  const bool same_cost = !cost || (c.cost.size() == (size_t)S * (size_t)S && std::memcmp(c.cost.data(), cost, c.cost.size() * sizeof(uint32_t)) == 0);
  const bool same_shape = c.eng && c.n == n && c.P == P && c.protein == protein && same_cost;
  // the host vouches for the content: same object, same stamp
  if (same_shape && g_h.alignment_stamp && c.aln == g_h.alignment_id(t) && c.stamp == g_h.alignment_stamp(t)) return c.eng;
  // otherwise the content decides (a pointer is no identity: `delete aln; new Alignment` returns the same address):
  // the alignment as the IQ-TREE side holds it (patterns of convertState codes), frequencies, and a hash of the states
  std::vector<signed char> col((size_t)n);
  std::vector<int8_t> states((size_t)n * (size_t)P);
  std::vector<int32_t> freq((size_t)P);
  unsigned long long hash = 1469598103934665603ull;       // FNV-1a over the patterns, taxon-minor
  for (int p = 0; p < P; p++) {
    int f = 0;
    g_h.pattern(t, p, col.data(), &f);
    freq[(size_t)p] = f;
    for (int i = 0; i < n; i++) {
      states[(size_t)i * (size_t)P + (size_t)p] = (int8_t)col[(size_t)i];
      hash = (hash ^ (unsigned char)col[(size_t)i]) * 1099511628211ull;
    }
  }
  if (same_shape && hash == c.hash) {
    // the same characters: at most the frequencies differ (a re-weighted copy of the alignment)
    if (freq != c.freq) {
      if (mpf_set_weights(c.eng, freq.data())) die("mpf_set_weights");
      c.freq = freq;
    }
    c.aln = g_h.alignment_id(t);
    c.stamp = g_h.alignment_stamp ? g_h.alignment_stamp(t) : 0;
    return c.eng;
  }
  drop(c);
  std::vector<uint8_t> codes(states.size());
  if (mpf_encode_iqtree_states(protein ? MPF_AA : MPF_DNA, states.data(), (int64_t)states.size(), codes.data())) die("mpf_encode_iqtree_states");
  mpf_config cfg;
  std::memset(&cfg, 0, sizeof cfg);
  cfg.n_taxa = n;
  cfg.n_patterns = P;
  cfg.datatype = protein ? MPF_AA : MPF_DNA;
  cfg.keep_all_sites = 1;                  // every pattern counts (phylotree.cpp:758, :985)
  if (cost) {
    c.cost.assign(cost, cost + (size_t)S * (size_t)S);
    if (mpf_engine_create_sankoff(&c.eng, &cfg, codes.data(), freq.data(), c.cost.data())) die("mpf_engine_create_sankoff");
  } else if (mpf_engine_create(&c.eng, &cfg, codes.data(), freq.data())) die("mpf_engine_create");
  c.aln = g_h.alignment_id(t);
  c.stamp = g_h.alignment_stamp ? g_h.alignment_stamp(t) : 0;
  c.hash = hash;
  c.freq = freq;
  c.n = n;
  c.P = P;
  c.protein = protein;
  return c.eng;
}

// IQ-TREE nodes (ids: leaves = taxon ids 0..n-1, inner n..2n-3) -> the engine's record links: node number = id + 1,
// slot = position in neighbors[]
void marshal_tree(PhyloTree *t, int n, std::vector<int32_t> &back)
{
  back.assign(3 * (size_t)(2 * n - 1), -1);
  std::vector<int> nei((size_t)(2 * n - 2) * 3, -1);
  for (int id = 0; id < 2 * n - 2; id++) g_h.neighbors(t, id, &nei[(size_t)id * 3]);
  auto slot_of = [&](int id, int other) {
    const int k = id < n ? 1 : 3;
    for (int s = 0; s < k; s++)
      if (nei[(size_t)id * 3 + (size_t)s] == other) return s;
    std::fprintf(stderr, "mpfitch phylotree shim: nodes %d and %d are not mutual neighbours\n", id, other);
    std::exit(EXIT_FAILURE);
  };
  for (int id = 0; id < 2 * n - 2; id++) {
    const int k = id < n ? 1 : 3;
    for (int s = 0; s < k; s++) {
      const int o = nei[(size_t)id * 3 + (size_t)s];
      if (o < 0 || o >= 2 * n - 2) { std::fprintf(stderr, "mpfitch phylotree shim: node %d has no neighbour %d (multifurcating or rooted tree?)\n", id, s); std::exit(EXIT_FAILURE); }
      back[(size_t)(3 * (id + 1) + s)] = 3 * (o + 1) + slot_of(o, id);
    }
  }
}

mpf_phylotree_poly_hooks g_poly;
bool g_poly_installed = false;

// A tree with polytomies as the neighbour lists the engine's polytomy calls take (include/mpfitch.h): walked from leaf 0 through the
// optional hook table; inner node numbers n + 1 + i follow the order of the host's inner ids, ids[i] = the host id of inner node i.
// false: no table installed, or the tree is fully resolved (n - 2 inner nodes of degree 3) -- the caller takes marshal_tree
bool marshal_lists(PhyloTree *t, int n, std::vector<int32_t> &first, std::vector<int32_t> &nbr, std::vector<int> &ids)
{
  if (!g_poly_installed) return false;
  auto fail = [](const char *what, int id) { std::fprintf(stderr, "mpfitch phylotree shim: multifurcating tree: %s (node %d)\n", what, id); std::exit(EXIT_FAILURE); };
  if (g_poly.degree(t, 0) != 1) fail("leaf 0 has not one neighbour", 0);
  int r0 = -1;
  g_poly.neighbors_n(t, 0, &r0, 1);
  if (r0 < n) fail("leaf 0 hangs on no inner node", r0);
  ids.assign(1, r0);
  std::vector<int> stack(1, r0), buf;
  bool resolved = true;
  while (!stack.empty()) {                  // every inner node is reached from the first one through inner neighbours
    const int v = stack.back();
    stack.pop_back();
    const int d = g_poly.degree(t, v);
    if (d < 3) fail("an inner node of degree below 3", v);
    if (d != 3) resolved = false;
    buf.assign((size_t)d, -1);
    g_poly.neighbors_n(t, v, buf.data(), d);
    for (int u : buf)
      if (u >= n && std::find(ids.begin(), ids.end(), u) == ids.end()) {
        if ((int)ids.size() >= n - 2) fail("more than n - 2 inner nodes (a cycle?)", u);
        ids.push_back(u);
        stack.push_back(u);
      }
  }
  if (resolved && (int)ids.size() == n - 2) return false;
  std::sort(ids.begin(), ids.end());
  first.assign(1, 0);
  nbr.clear();
  for (int v : ids) {
    const int d = g_poly.degree(t, v);
    buf.assign((size_t)d, -1);
    g_poly.neighbors_n(t, v, buf.data(), d);
    for (int u : buf) {
      if (u < 0) fail("a neighbour without an id", v);
      nbr.push_back(u < n ? u + 1 : n + 1 + (int32_t)(std::lower_bound(ids.begin(), ids.end(), u) - ids.begin()));
    }
    first.push_back((int32_t)nbr.size());
  }
  return true;                              // (what else can be wrong with the lists the engine's own checks refuse, with a message)
}
// node number of the lists -> host id
inline int host_id(int node, int n, const std::vector<int> &ids) { return node <= n ? node - 1 : ids[(size_t)(node - n - 1)]; }

int compute(PhyloTree *t, const unsigned int *cost)
{
  mpf_engine *e = engine_for(t, cost);
  const int n = g_h.n_taxa(t), P = g_h.n_patterns(t);
  std::vector<int32_t> back, first, nbr;
  std::vector<int> ids;
  if (marshal_lists(t, n, first, nbr, ids)) {
    // the k-ary rules at the root leaf: the Fitch length of a tree with polytomies depends on it as well (phylotree.cpp:869-931)
    unsigned short *pp = g_h.pattern_pars(t, P + kVcsizeUshort);
    std::memset(pp, 0, sizeof(unsigned short) * (size_t)(P + kVcsizeUshort));
    const int root = g_h.root_id ? g_h.root_id(t) : 0;
    if (root < 0 || root >= n) { std::fprintf(stderr, "mpfitch phylotree shim: root %d is not a leaf id\n", root); std::exit(EXIT_FAILURE); }
    uint32_t score = 0;
    if (mpf_polytomy_parsimony(e, (int32_t)ids.size(), first.data(), nbr.data(), root + 1, &score, pp)) die("mpf_polytomy_parsimony");
    return (int)score;
  }
  marshal_tree(t, n, back);
  unsigned short *pp = g_h.pattern_pars(t, P + kVcsizeUshort);           // phylotree.cpp:1056-1057
  std::memset(pp, 0, sizeof(unsigned short) * (size_t)(P + kVcsizeUshort));   // :957
  uint32_t score = 0;
  // ParsTree::computeParsimony() = computeParsimonyBranch(root->neighbors[0], root) (parstree.cpp:101-116): evaluated at the
  // root leaf's edge, the rest of the tree as the parent side -- the engine's evaluation at that leaf (node number = id + 1)
  const int root = (cost && g_h.root_id) ? g_h.root_id(t) : 0;
  if (root < 0 || root >= n) { std::fprintf(stderr, "mpfitch phylotree shim: root %d is not a leaf id\n", root); std::exit(EXIT_FAILURE); }
  if (mpf_compute_parsimony_at(e, back.data(), root + 1, &score, pp)) die("mpf_compute_parsimony_at");
  return (int)score;
}

mpf_phylotree_nni_hooks g_nni;
bool g_nni_installed = false;

}  // namespace

void mpfitch_phylotree_install_poly(const mpf_phylotree_poly_hooks *hooks)
{
  g_poly_installed = hooks && hooks->degree && hooks->neighbors_n;
  if (g_poly_installed) g_poly = *hooks;
}

void mpfitch_phylotree_install_nni(const mpf_phylotree_nni_hooks *hooks)
{
  g_nni = *hooks;
  g_nni_installed = hooks->swap != nullptr;
}

// IQTree::optimizeNNI (iqtree.cpp:2173-2302), MP mode, MAXSTEPS 50: the climb runs on the engine, its swaps are replayed here
// (a ParsTree: the return value is ParsTree::computeParsimony() of the final tree, the length at the root leaf)
int mpfitch_optimize_nni(PhyloTree *t, int *nni_count, int *nni_steps)
{
  if (!g_nni_installed) { std::fprintf(stderr, "mpfitch phylotree shim: mpfitch_phylotree_install_nni() was not called\n"); std::exit(EXIT_FAILURE); }
  // A ParsTree (-cost: phyloanalysis.cpp:2200-2203) climbs on the weighted engine under "nni_weighted": NNIs scored by
  // ParsTree::computeParsimonyBranch, and no rollback (iqtree.cpp:2258).  That rule hangs on -cost being given, not on the matrix,
  // so unit costs ("-cost e", which computeParsimony below runs on the Fitch engine) take the weighted engine here as well.
  const unsigned int *cost = g_h.cost_matrix ? g_h.cost_matrix(t) : nullptr;
  mpf_engine *e = engine_for(t, cost);
  if (cost && mpf_set_option(e, "nni_weighted", 1)) die("mpf_set_option nni_weighted");
  const int n = g_h.n_taxa(t);
  std::vector<int32_t> back;
  marshal_tree(t, n, back);
  if (mpf_set_tree(e, back.data())) die("mpf_set_tree");
  const int root = g_h.root_id ? g_h.root_id(t) : 0;
  if (root < 0 || root >= n) { std::fprintf(stderr, "mpfitch phylotree shim: root %d is not a leaf id\n", root); std::exit(EXIT_FAILURE); }
  const int speednni = g_nni.speednni ? g_nni.speednni(t) : 1;
  uint32_t score = 0;
  int32_t count = 0, steps = 0, k = 0;
  if (mpf_optimize_nni(e, root + 1, speednni, 50, &score, &count, &steps)) die("mpf_optimize_nni");
  if (mpf_get_nni_moves(e, 0, nullptr, nullptr, nullptr, nullptr, &k)) die("mpf_get_nni_moves");
  std::vector<int32_t> n1((size_t)k), s1((size_t)k), n2((size_t)k), s2((size_t)k);
  if (k && mpf_get_nni_moves(e, k, n1.data(), s1.data(), n2.data(), s2.data(), &k)) die("mpf_get_nni_moves");
  for (int i = 0; i < k; i++) g_nni.swap(t, n1[(size_t)i] - 1, s1[(size_t)i], n2[(size_t)i] - 1, s2[(size_t)i]);   // node number = id + 1
  if (nni_count) *nni_count = count;
  if (nni_steps) *nni_steps = steps;
  return (int)score;
}

static mpf_phylotree_brlen_hooks g_brlen;
static bool g_brlen_installed = false;

void mpfitch_phylotree_install_brlen(const mpf_phylotree_brlen_hooks *hooks)
{
  g_brlen = *hooks;
  g_brlen_installed = hooks->n_sites && hooks->get_length && hooks->set_length;
}

// int PhyloTree::fixNegativeBranch(bool force, Node *node = NULL, Node *dad = NULL) (phylotree.cpp:3597-3633) called from the root
// -- _ZN9PhyloTree17fixNegativeBranchEbP4NodeS1_ in a mpboot build; served: phyloanalysis.cpp:1153, :1180, :1336, :1501, and the
// consensus tree (:2280), which may be multifurcating, once mpfitch_phylotree_install_poly has been called (else marshal_tree
// refuses such a tree).
int mpfitch_fix_negative_branch(PhyloTree *t, int force)
{
  if (!g_brlen_installed) { std::fprintf(stderr, "mpfitch phylotree shim: mpfitch_phylotree_install_brlen() was not called\n"); std::exit(EXIT_FAILURE); }
  const unsigned int *cost = g_h.cost_matrix ? g_h.cost_matrix(t) : nullptr;
  // ParsTree's rule (branch_subst = the tree's length) hangs on the class, not on the matrix; unit costs score on the Fitch engine
  const int parstree = g_brlen.is_parstree ? (g_brlen.is_parstree(t) ? 1 : 0) : (cost ? 1 : 0);
  if (cost) {
    const int S = g_h.is_protein(t) ? 20 : 4;
    bool unit = true;
    for (int i = 0; i < S && unit; i++)
      for (int j = 0; j < S; j++)
        if (cost[i * S + j] != (i == j ? 0u : 1u)) { unit = false; break; }
    if (unit) cost = nullptr;
  }
  mpf_engine *e = engine_for(t, cost);
  const int n = g_h.n_taxa(t);
  std::vector<int32_t> back, first, nbr;
  std::vector<int> ids;
  const bool poly = marshal_lists(t, n, first, nbr, ids);
  if (!poly) {
    marshal_tree(t, n, back);
    if (mpf_set_tree(e, back.data())) die("mpf_set_tree");
    ids.resize((size_t)(n - 2));
    for (int i = 0; i < n - 2; i++) ids[(size_t)i] = n + i;          // node number = id + 1
  }
  const int root = g_h.root_id ? g_h.root_id(t) : 0;
  if (root < 0 || root >= n) { std::fprintf(stderr, "mpfitch phylotree shim: root %d is not a leaf id\n", root); std::exit(EXIT_FAILURE); }
  int32_t m = n + (int32_t)ids.size() - 1, k = 0;
  std::vector<int32_t> n1((size_t)m), n2((size_t)m);
  std::vector<double> len((size_t)m);
  if (poly) {
    if (mpf_polytomy_branch_lengths(e, (int32_t)ids.size(), first.data(), nbr.data(), root + 1, g_brlen.n_sites(t), parstree, m, n1.data(), n2.data(),
                                    len.data(), &k) || k != m) die("mpf_polytomy_branch_lengths");
  } else if (mpf_branch_lengths(e, root + 1, g_brlen.n_sites(t), parstree, m, n1.data(), n2.data(), len.data(), &k) || k != m) die("mpf_branch_lengths");
  int fixed = 0;
  for (int i = 0; i < m; i++) {
    const int a = host_id(n1[(size_t)i], n, ids), b = host_id(n2[(size_t)i], n, ids);
    double cur = g_brlen.get_length(t, a, b);
    if (cur < 0.0 || force) {
      cur = len[(size_t)i];
      g_brlen.set_length(t, a, b, cur);
      fixed++;
    }
    if (cur <= 0.0) g_brlen.set_length(t, a, b, 1e-6);              // MIN_BRANCH_LEN (:3626-3629)
  }
  return fixed;
}

static mpf_phylotree_support_hooks g_support;
static bool g_support_installed = false;

void mpfitch_phylotree_install_support(const mpf_phylotree_support_hooks *hooks)
{
  g_support_installed = hooks && hooks->set_support;
  if (g_support_installed) g_support = *hooks;
}

// the supports summarizeBootstrap's split counts put on the best tree (iqtree.cpp:4020-4165): one mpf_split_support call, the
// branches in the walk order of mpf_branch_substitutions from leaf 0 (node number = id + 1)
int mpfitch_assign_split_support(PhyloTree *t, int n_trees, const int *backs, const int *weights)
{
  if (!g_support_installed) { std::fprintf(stderr, "mpfitch phylotree shim: mpfitch_phylotree_install_support() was not called\n"); std::exit(EXIT_FAILURE); }
  const unsigned int *cost = g_h.cost_matrix ? g_h.cost_matrix(t) : nullptr;
  mpf_engine *e = engine_for(t, cost);
  const int n = g_h.n_taxa(t);
  std::vector<int32_t> back;
  marshal_tree(t, n, back);
  int32_t m = 2 * n - 3, k = 0;
  int64_t total = 0;
  std::vector<int32_t> n1((size_t)m), n2((size_t)m);
  std::vector<int64_t> sup((size_t)m);
  if (mpf_split_support(e, n_trees, backs, weights, back.data(), m, n1.data(), n2.data(), sup.data(), &k, &total) || k != m) die("mpf_split_support");
  int inner = 0;
  for (int i = 0; i < m; i++)
    if (sup[(size_t)i] >= 0) {
      g_support.set_support(t, n1[(size_t)i] - 1, n2[(size_t)i] - 1, (long long)sup[(size_t)i], (long long)total);
      inner++;
    }
  return inner;
}

void mpfitch_phylotree_install(const mpf_phylotree_hooks *hooks)
{
  g_h = *hooks;
  g_installed = hooks->n_taxa && hooks->n_patterns && hooks->is_protein && hooks->pattern && hooks->neighbors && hooks->pattern_pars &&
                hooks->alignment_id;
}

void mpfitch_phylotree_release(void)
{
  drop(g_fitch);
  drop(g_cost);
}

extern "C" {

// int PhyloTree::computeParsimony()        (phylotree.cpp:1049-1061)
int _ZN9PhyloTree16computeParsimonyEv(PhyloTree *self) { return compute(self, nullptr); }

// int ParsTree::computeParsimony()         (parstree.cpp:101-116): the Sankoff twin; "-cost fitch" / "-cost e" load unit
// costs (parstree.cpp:42-49), for which the weighted length IS the Fitch length -- those run on the Fitch engine
int _ZN8ParsTree16computeParsimonyEv(PhyloTree *self)
{
  const unsigned int *cost = g_h.cost_matrix ? g_h.cost_matrix(self) : nullptr;
  if (cost) {
    const int S = g_h.is_protein(self) ? 20 : 4;
    bool unit = true;
    for (int i = 0; i < S && unit; i++)
      for (int j = 0; j < S; j++)
        if (cost[i * S + j] != (i == j ? 0u : 1u)) { unit = false; break; }
    if (unit) cost = nullptr;
    // (an asymmetric matrix makes the length depend on the rooting: compute() evaluates where ParsTree does, hook root_id)
  }
  return compute(self, cost);
}

}  // extern "C"
