/*
 * polytomy_shim_driver.cpp -- TEST INFRASTRUCTURE ONLY (compiled by tests/test_gpu_polytomy_dropin.py).
 * A stand-in tree driver for a MULTIFURCATING tree at integration/phylotree_shim.cpp: the tree is held as a neighbour vector per
 * node with a length per neighbour, the way mpboot's Node::neighbors does.  It installs the hook tables -- the optional one for
 * trees with polytomies only when asked --, calls computeParsimony() (ParsTree's with a cost matrix) and
 * mpfitch_fix_negative_branch(), and prints what they left:
 *     score S
 *     ptn p0 p1 ...                    (_pattern_pars)
 *     fixed F
 *     one row "k len0 .. len(k-1)" per node   (%.17g)
 * input (text, stdin): n P protein(0|1) ; P frequencies ; n rows of P state codes ; nodes ; per node "id k id0 .. id(k-1)" ;
 *                      root n_sites force parstree(-1 | 0 | 1) has_cost(0|1) poly_hooks(0|1) ; [S * S cost entries] ;
 *                      per node "len0 .. len(k-1)"
 * Node ids need not be contiguous: the rows carry them.
 */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../integration/phylotree_hooks.h"

class PhyloTree {
 public:
  int n = 0, P = 0, protein = 0, root = 0, nsites = 0, parstree = -1;
  std::vector<int> freq;
  std::vector<signed char> states;            // [n][P]
  std::vector<int> order;                     // node ids in input order
  std::map<int, std::vector<int>> nei;
  std::map<int, std::vector<double>> len;
  std::vector<unsigned int> cost;
  std::vector<unsigned short> pattern_pars;
};

extern "C" int _ZN9PhyloTree16computeParsimonyEv(PhyloTree *self);
extern "C" int _ZN8ParsTree16computeParsimonyEv(PhyloTree *self);

static int hk_ntaxa(const PhyloTree *t) { return t->n; }
static int hk_nptn(const PhyloTree *t) { return t->P; }
static int hk_prot(const PhyloTree *t) { return t->protein; }
static void hk_pattern(const PhyloTree *t, int p, signed char *st, int *f)
{
  for (int i = 0; i < t->n; i++) st[i] = t->states[(size_t)i * (size_t)t->P + (size_t)p];
  *f = t->freq[(size_t)p];
}
// the three-neighbour hook of the first table: what a host that knows nothing of polytomies hands out
static void hk_nei(const PhyloTree *t, int id, int out[3])
{
  auto it = t->nei.find(id);
  for (int k = 0; k < 3; k++) out[k] = (it != t->nei.end() && k < (int)it->second.size()) ? it->second[(size_t)k] : -1;
}
static unsigned short *hk_ptnpars(PhyloTree *t, int len) { t->pattern_pars.assign((size_t)len, 0); return t->pattern_pars.data(); }
static const void *hk_alnid(const PhyloTree *t) { return t->states.data(); }
static int hk_root(const PhyloTree *t) { return t->root; }
static const unsigned int *hk_cost(const PhyloTree *t) { return t->cost.empty() ? nullptr : t->cost.data(); }
static int hk_degree(const PhyloTree *t, int id) { auto it = t->nei.find(id); return it == t->nei.end() ? 0 : (int)it->second.size(); }
static int hk_nei_n(const PhyloTree *t, int id, int *out, int cap)
{
  auto it = t->nei.find(id);
  if (it == t->nei.end()) return 0;
  for (int k = 0; k < (int)it->second.size() && k < cap; k++) out[k] = it->second[(size_t)k];
  return (int)it->second.size();
}

static size_t slot_of(const PhyloTree *t, int id1, int id2)
{
  const std::vector<int> &v = t->nei.at(id1);
  for (size_t k = 0; k < v.size(); k++)
    if (v[k] == id2) return k;
  std::fprintf(stderr, "polytomy_shim_driver: %d is no neighbour of %d\n", id2, id1);
  std::exit(3);
}
static int hk_nsites(const PhyloTree *t) { return t->nsites; }
static double hk_getlen(const PhyloTree *t, int id1, int id2) { return t->len.at(id1)[slot_of(t, id1, id2)]; }
static void hk_setlen(PhyloTree *t, int id1, int id2, double v) { t->len[id1][slot_of(t, id1, id2)] = v; t->len[id2][slot_of(t, id2, id1)] = v; }
static int hk_parstree(const PhyloTree *t) { return t->parstree; }

int main()
{
  PhyloTree t;
  if (std::scanf("%d %d %d", &t.n, &t.P, &t.protein) != 3) return 2;
  t.freq.resize((size_t)t.P);
  for (int &f : t.freq) if (std::scanf("%d", &f) != 1) return 2;
  t.states.resize((size_t)t.n * (size_t)t.P);
  for (auto &s : t.states) { int v; if (std::scanf("%d", &v) != 1) return 2; s = (signed char)v; }
  int nodes = 0;
  if (std::scanf("%d", &nodes) != 1) return 2;
  for (int i = 0; i < nodes; i++) {
    int id = 0, k = 0;
    if (std::scanf("%d %d", &id, &k) != 2) return 2;
    t.order.push_back(id);
    t.nei[id].resize((size_t)k);
    for (int &u : t.nei[id]) if (std::scanf("%d", &u) != 1) return 2;
  }
  int force = 0, has_cost = 0, poly_hooks = 0;
  if (std::scanf("%d %d %d %d %d %d", &t.root, &t.nsites, &force, &t.parstree, &has_cost, &poly_hooks) != 6) return 2;
  if (has_cost) {
    const int S = t.protein ? 20 : 4;
    t.cost.resize((size_t)S * (size_t)S);
    for (auto &c : t.cost) if (std::scanf("%u", &c) != 1) return 2;
  }
  for (int id : t.order) {
    t.len[id].resize(t.nei[id].size());
    for (double &v : t.len[id]) if (std::scanf("%lf", &v) != 1) return 2;
  }

  mpf_phylotree_hooks h{};
  h.n_taxa = hk_ntaxa; h.n_patterns = hk_nptn; h.is_protein = hk_prot; h.pattern = hk_pattern; h.neighbors = hk_nei;
  h.pattern_pars = hk_ptnpars; h.alignment_id = hk_alnid; h.root_id = hk_root; h.cost_matrix = hk_cost;
  mpfitch_phylotree_install(&h);
  mpf_phylotree_brlen_hooks bh{};
  bh.n_sites = hk_nsites; bh.get_length = hk_getlen; bh.set_length = hk_setlen;
  if (t.parstree >= 0) bh.is_parstree = hk_parstree;
  mpfitch_phylotree_install_brlen(&bh);
  mpf_phylotree_poly_hooks ph{};
  ph.degree = hk_degree; ph.neighbors_n = hk_nei_n;
  if (poly_hooks) mpfitch_phylotree_install_poly(&ph);

  const int score = has_cost ? _ZN8ParsTree16computeParsimonyEv(&t) : _ZN9PhyloTree16computeParsimonyEv(&t);
  std::printf("score %d\nptn", score);
  for (int p = 0; p < t.P; p++) std::printf(" %d", (int)t.pattern_pars[(size_t)p]);
  const int fixed = mpfitch_fix_negative_branch(&t, force);
  std::printf("\nfixed %d\n", fixed);
  for (int id : t.order) {
    std::printf("%d", (int)t.len[id].size());
    for (double v : t.len[id]) std::printf(" %.17g", v);
    std::printf("\n");
  }
  mpfitch_phylotree_release();
  return 0;
}
