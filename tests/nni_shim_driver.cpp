/*
 * nni_shim_driver.cpp -- TEST INFRASTRUCTURE ONLY (compiled by tests/test_gpu_nni_dropin.py).
 * A stand-in tree driver for the NNI entry point of integration/phylotree_shim.cpp: it holds a tree as neighbour lists the way
 * mpboot's Node::neighbors does, installs the two hook tables, calls mpfitch_optimize_nni() and prints what the climb left:
 *     score S count C steps T
 *     2n-2 rows "k id0 [id1 id2]"   (the host's tree after the replayed swaps)
 * input (text, stdin): n P protein(0|1) ; P frequencies ; n rows of P state codes ; 2n-2 rows "k id0 [id1 id2]" ; root leaf id ;
 *                      speednni (0|1)
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../integration/phylotree_hooks.h"

class PhyloTree {
 public:
  int n = 0, P = 0, protein = 0, root = 0, speednni = 1;
  std::vector<int> freq;
  std::vector<signed char> states;            // [n][P]
  std::vector<int> nei;                       // [2n-2][3]
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
static int hk_speednni(const PhyloTree *t) { return t->speednni; }

// PhyloTree::doNNI on neighbour lists: the two slots trade their neighbours, each subtree root's link follows
static void relink(PhyloTree *t, int node, int from, int to)
{
  for (int k = 0; k < 3; k++)
    if (t->nei[(size_t)node * 3 + (size_t)k] == from) { t->nei[(size_t)node * 3 + (size_t)k] = to; return; }
  std::fprintf(stderr, "nni_shim_driver: %d is no neighbour of %d\n", from, node);
  std::exit(3);
}
static void hk_swap(PhyloTree *t, int id1, int slot1, int id2, int slot2)
{
  int &x = t->nei[(size_t)id1 * 3 + (size_t)slot1], &y = t->nei[(size_t)id2 * 3 + (size_t)slot2];
  const int a = x, c = y;
  x = c;
  y = a;
  relink(t, c, id2, id1);
  relink(t, a, id1, id2);
}

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
  if (std::scanf("%d %d", &t.root, &t.speednni) != 2) return 2;

  mpf_phylotree_hooks h{};
  h.n_taxa = hk_ntaxa; h.n_patterns = hk_nptn; h.is_protein = hk_prot; h.pattern = hk_pattern; h.neighbors = hk_nei;
  h.pattern_pars = hk_ptnpars; h.alignment_id = hk_alnid; h.root_id = hk_root;
  mpfitch_phylotree_install(&h);
  mpf_phylotree_nni_hooks nh{};
  nh.swap = hk_swap;
  nh.speednni = hk_speednni;
  mpfitch_phylotree_install_nni(&nh);

  int count = -1, steps = -1;
  const int score = mpfitch_optimize_nni(&t, &count, &steps);      // curScore = -score in doNNISearch
  std::printf("score %d count %d steps %d\n", score, count, steps);
  for (int id = 0; id < 2 * t.n - 2; id++) {
    const int k = id < t.n ? 1 : 3;
    std::printf("%d", k);
    for (int j = 0; j < k; j++) std::printf(" %d", t.nei[(size_t)id * 3 + (size_t)j]);
    std::printf("\n");
  }
  mpfitch_phylotree_release();
  return 0;
}
