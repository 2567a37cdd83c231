/*
 * brlen_shim_driver.cpp -- TEST INFRASTRUCTURE ONLY (compiled by tests/test_gpu_brlen_dropin.py).
 * A stand-in tree driver for the branch-length entry point of integration/phylotree_shim.cpp: it holds a tree as neighbour lists
 * with a length per (node, slot) the way mpboot's Node::neighbors does, installs the hook tables, calls
 * mpfitch_fix_negative_branch() and prints what it left:
 *     fixed F
 *     2n-2 rows "k len0 [len1 len2]"   (the length on every neighbour, %.17g)
 * input (text, stdin): n P protein(0|1) ; P frequencies ; n rows of P state codes ; 2n-2 rows "k id0 [id1 id2]" ; root leaf id ;
 *                      n_sites force parstree(-1 = no is_parstree hook | 0 | 1) has_cost(0|1) ; [S * S cost entries] ;
 *                      2n-2 rows "len0 [len1 len2]"
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../integration/phylotree_hooks.h"

class PhyloTree {
 public:
  int n = 0, P = 0, protein = 0, root = 0, nsites = 0, parstree = -1;
  std::vector<int> freq;
  std::vector<signed char> states;            // [n][P]
  std::vector<int> nei;                       // [2n-2][3]
  std::vector<double> len;                    // [2n-2][3]
  std::vector<unsigned int> cost;             // empty: no matrix
  std::vector<unsigned short> pattern_pars;
};

static int hk_ntaxa(const PhyloTree *t) { return t->n; }
static int hk_nptn(const PhyloTree *t) { return t->P; }
static int hk_prot(const PhyloTree *t) { return t->protein; }
static void hk_pattern(const PhyloTree *t, int p, signed char *st, int *f)
{
  for (int i = 0; i < t->n; i++) st[i] = t->states[(size_t)i * (size_t)t->P + (size_t)p];
  *f = t->freq[(size_t)p];
}
static void hk_nei(const PhyloTree *t, int id, int out[3]) { for (int k = 0; k < 3; k++) out[k] = t->nei[(size_t)id * 3 + (size_t)k]; }
static unsigned short *hk_ptnpars(PhyloTree *t, int len) { t->pattern_pars.assign((size_t)len, 0); return t->pattern_pars.data(); }
static const void *hk_alnid(const PhyloTree *t) { return t->states.data(); }
static int hk_root(const PhyloTree *t) { return t->root; }
static const unsigned int *hk_cost(const PhyloTree *t) { return t->cost.empty() ? nullptr : t->cost.data(); }

static size_t slot_of(const PhyloTree *t, int id1, int id2)
{
  for (int k = 0; k < 3; k++)
    if (t->nei[(size_t)id1 * 3 + (size_t)k] == id2) return (size_t)id1 * 3 + (size_t)k;
  std::fprintf(stderr, "brlen_shim_driver: %d is no neighbour of %d\n", id2, id1);
  std::exit(3);
}
static int hk_nsites(const PhyloTree *t) { return t->nsites; }
static double hk_getlen(const PhyloTree *t, int id1, int id2) { return t->len[slot_of(t, id1, id2)]; }
static void hk_setlen(PhyloTree *t, int id1, int id2, double v) { t->len[slot_of(t, id1, id2)] = v; t->len[slot_of(t, id2, id1)] = v; }
static int hk_parstree(const PhyloTree *t) { return t->parstree; }

int main()
{
  PhyloTree t;
  if (std::scanf("%d %d %d", &t.n, &t.P, &t.protein) != 3) return 2;
  t.freq.resize((size_t)t.P);
  for (int &f : t.freq) if (std::scanf("%d", &f) != 1) return 2;
  t.states.resize((size_t)t.n * (size_t)t.P);
  for (auto &s : t.states) { int v; if (std::scanf("%d", &v) != 1) return 2; s = (signed char)v; }
  t.nei.assign((size_t)(2 * t.n - 2) * 3, -1);
  for (int id = 0; id < 2 * t.n - 2; id++) {
    int k = 0;
    if (std::scanf("%d", &k) != 1) return 2;
    for (int j = 0; j < k; j++) if (std::scanf("%d", &t.nei[(size_t)id * 3 + (size_t)j]) != 1) return 2;
  }
  int force = 0, has_cost = 0;
  if (std::scanf("%d %d %d %d %d", &t.root, &t.nsites, &force, &t.parstree, &has_cost) != 5) return 2;
  if (has_cost) {
    const int S = t.protein ? 20 : 4;
    t.cost.resize((size_t)S * (size_t)S);
    for (auto &c : t.cost) if (std::scanf("%u", &c) != 1) return 2;
  }
  t.len.assign((size_t)(2 * t.n - 2) * 3, 0.0);
  for (int id = 0; id < 2 * t.n - 2; id++)
    for (int j = 0; j < (id < t.n ? 1 : 3); j++) if (std::scanf("%lf", &t.len[(size_t)id * 3 + (size_t)j]) != 1) return 2;

  mpf_phylotree_hooks h{};
  h.n_taxa = hk_ntaxa; h.n_patterns = hk_nptn; h.is_protein = hk_prot; h.pattern = hk_pattern; h.neighbors = hk_nei;
  h.pattern_pars = hk_ptnpars; h.alignment_id = hk_alnid; h.root_id = hk_root; h.cost_matrix = hk_cost;
  mpfitch_phylotree_install(&h);
  mpf_phylotree_brlen_hooks bh{};
  bh.n_sites = hk_nsites; bh.get_length = hk_getlen; bh.set_length = hk_setlen;
  if (t.parstree >= 0) bh.is_parstree = hk_parstree;
  mpfitch_phylotree_install_brlen(&bh);

  const int fixed = mpfitch_fix_negative_branch(&t, force);
  std::printf("fixed %d\n", fixed);
  for (int id = 0; id < 2 * t.n - 2; id++) {
    const int k = id < t.n ? 1 : 3;
    std::printf("%d", k);
    for (int j = 0; j < k; j++) std::printf(" %.17g", t.len[(size_t)id * 3 + (size_t)j]);
    std::printf("\n");
  }
  mpfitch_phylotree_release();
  return 0;
}
