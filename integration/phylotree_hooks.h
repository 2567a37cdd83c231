// phylotree_hooks.h -- what integration/phylotree_shim.cpp needs from mpboot's PhyloTree / ParsTree objects.
//
// The shim defines PhyloTree::computeParsimony() and ParsTree::computeParsimony() (phylotree.h:432, parstree.h:50) on
// libmpfitch.so without seeing the class definitions (phylotree.h drags in tools.h -> <iqtree_config.h>, a
// CMake-generated header), so every member it needs is reached through this table.  A maintainer fills it once, e.g. in
// phylotree.cpp:
//
//     static int  hk_ntaxa(const PhyloTree *t)  { return t->aln->getNSeq(); }
//     static int  hk_nptn(const PhyloTree *t)   { return t->aln->size(); }
//     static int  hk_prot(const PhyloTree *t)   { return t->aln->seq_type == SEQ_PROTEIN; }
//     static void hk_pattern(const PhyloTree *t, int p, signed char *st, int *f)
//         { const Pattern &pt = t->aln->at(p); for (size_t i = 0; i < pt.size(); i++) st[i] = pt[i]; *f = pt.frequency; }
//     static int  hk_root(const PhyloTree *t)   { return t->root->id; }
//     static void hk_nei(const PhyloTree *t, int id, int out[3])    // ids of the neighbours of node `id` (leaf: one)
//         { ... NodeVector from getAllNodes / a cached id -> Node* table; out[k] = node->neighbors[k]->node->id ... }
//     static unsigned short *hk_ptnpars(PhyloTree *t, int len)
//         { if (!t->_pattern_pars) t->_pattern_pars = aligned_alloc<BootValTypePars>(len); return t->_pattern_pars; }
//     static const unsigned int *hk_cost(const PhyloTree *t)        // ParsTree only: its cost_matrix, NULL for Fitch
//         { const ParsTree *p = dynamic_cast<const ParsTree *>(t); return p ? p->cost_matrix : NULL; }
//     static const void *hk_alnid(const PhyloTree *t) { return t->aln; }
//     ... mpfitch_phylotree_install(&hooks);
#pragma once
#include "../include/mpfitch.h"

class PhyloTree;

struct mpf_phylotree_hooks {
  int (*n_taxa)(const PhyloTree *);                       // aln->getNSeq()
  int (*n_patterns)(const PhyloTree *);                   // aln->size()
  int (*is_protein)(const PhyloTree *);                   // aln->seq_type == SEQ_PROTEIN (20 states), else DNA
  // aln->at(ptn): Alignment::convertState codes of every taxon (alignment.cpp:839-916) and the pattern's frequency
  void (*pattern)(const PhyloTree *, int ptn, signed char *states /* [n_taxa] */, int *frequency);
  // topology by node id: leaves carry the taxon id 0..n-1, inner nodes n..2n-3 (Node::id, node.h); out = ids of the
  // neighbours in neighbors[] order (a leaf fills out[0] only)
  void (*neighbors)(const PhyloTree *, int node_id, int out[3]);
  // _pattern_pars (phylotree.h:1368), allocated with room for `len` = nptn + VCSIZE_USHORT entries if still NULL
  // (phylotree.cpp:956, :1057)
  unsigned short *(*pattern_pars)(PhyloTree *, int len);
  // ParsTree: cost_matrix[i * nstates + j] (parstree.h; loaded and triangle-repaired by loadCostMatrixFile,
  // parstree.cpp:31-95); NULL = unit costs (PhyloTree, and ParsTree with "-cost fitch|e")
  const unsigned int *(*cost_matrix)(const PhyloTree *);
  // optional (may be NULL = taxon 0): t->root->id, the leaf ParsTree::computeParsimony() roots the tree at (parstree.cpp:101-116).
  // Only an ASYMMETRIC cost matrix makes the length depend on it.
  int (*root_id)(const PhyloTree *);
  // identity of the alignment the tree currently holds (t->aln).  NOT sufficient as a cache key: optimizeBootTrees does
  // `bootstrap_aln = new Alignment; ...; delete aln;` once per sample (iqtree.cpp:2519/2863, :2940/2977) and the allocator
  // hands the same address back, often with the same pattern count -- so the shim compares CONTENT: every call re-reads the
  // patterns, hashes the states and compares the frequencies (states changed -> engine rebuilt; only frequencies changed ->
  // mpf_set_weights).  That is P hook calls and n x P bytes per computeParsimony().
  const void *(*alignment_id)(const PhyloTree *);
  // optional (may be NULL): a number the host changes whenever the alignment's CONTENT changes (e.g. a counter bumped in
  // Alignment's constructors / setAlignment()).  When present and unchanged, with the same alignment_id, the shim skips
  // the re-read above.
  unsigned long long (*alignment_stamp)(const PhyloTree *);
};

void mpfitch_phylotree_install(const mpf_phylotree_hooks *hooks);
void mpfitch_phylotree_release(void);                     // frees the engines (end of the run / new alignment set)

// ---- the NNI hill climb (IQTree::optimizeNNI in MP mode; INTEGRATION.md "NNI climb").  A table of its own, so that the one above
// and its users stay as they are.
//     static void hk_swap(PhyloTree *t, int id1, int slot1, int id2, int slot2)     // PhyloTree::doNNI on the host's tree
//         { Node *n1 = node_of(t, id1), *n2 = node_of(t, id2); NeighborVec::iterator i1 = n1->neighbors.begin() + slot1,
//           i2 = n2->neighbors.begin() + slot2; NNIMove m; m.node1 = (PhyloNode *)n1; m.node2 = (PhyloNode *)n2;
//           m.node1Nei_it = i1; m.node2Nei_it = i2; t->doNNI(m); }
//     static int  hk_speednni(const PhyloTree *t) { return ((IQTree *)t)->searchinfo.speednni; }
//     ... mpfitch_phylotree_install_nni(&nni_hooks);
struct mpf_phylotree_nni_hooks {
  // the neighbours in neighbors[slot1] of node id1 and neighbors[slot2] of node id2 trade places, the back links of the two
  // subtree roots follow (PhyloTree::doNNI, phylotree.cpp:3715-3742)
  void (*swap)(PhyloTree *, int id1, int slot1, int id2, int slot2);
  // optional (may be NULL = on): searchinfo.speednni (tools.cpp:765)
  int (*speednni)(const PhyloTree *);
};
void mpfitch_phylotree_install_nni(const mpf_phylotree_nni_hooks *hooks);
// IQTree::optimizeNNI(nni_count, nni_steps) (iqtree.cpp:2173-2302) on the engine: the tree is marshalled as computeParsimony()
// marshals it, climbed by mpf_optimize_nni from the root leaf (hook root_id, else taxon 0) and the engine's swaps are replayed on
// the host's tree through the swap hook.  Returns the final length (curScore = -length).
int mpfitch_optimize_nni(PhyloTree *t, int *nni_count, int *nni_steps);

// ---- parsimony branch lengths (PhyloTree::fixNegativeBranch, phylotree.cpp:3597-3633; INTEGRATION.md "Branch lengths").  A third
// table of its own, so that the two above and their users stay as they are.
//     static int    hk_nsites(const PhyloTree *t) { return ((PhyloTree *)t)->getAlnNSite(); }
//     static double hk_getlen(const PhyloTree *t, int id1, int id2) { return node_of(t, id1)->findNeighbor(node_of(t, id2))->length; }
//     static void   hk_setlen(PhyloTree *t, int id1, int id2, double len)
//         { Node *a = node_of(t, id1), *b = node_of(t, id2); a->findNeighbor(b)->length = len; b->findNeighbor(a)->length = len; }
//     static int    hk_parstree(const PhyloTree *t) { return dynamic_cast<const ParsTree *>(t) != NULL; }
//     ... mpfitch_phylotree_install_brlen(&brlen_hooks);
struct mpf_phylotree_brlen_hooks {
  int (*n_sites)(const PhyloTree *);                               // getAlnNSite()
  double (*get_length)(const PhyloTree *, int id1, int id2);       // the length on the neighbour of id1 that points to id2
  void (*set_length)(PhyloTree *, int id1, int id2, double len);   // BOTH directions of the branch (phylotree.cpp:3619, :3623)
  // optional (may be NULL = "a tree with a cost matrix"): the tree is a ParsTree, whose computeParsimonyBranch hands back the
  // tree's length as branch_subst (parstree.cpp:534-535) -- under -cost fitch | e too, where the scoring runs on the Fitch engine
  int (*is_parstree)(const PhyloTree *);
};
void mpfitch_phylotree_install_brlen(const mpf_phylotree_brlen_hooks *hooks);
// PhyloTree::fixNegativeBranch(force) from the root on the engine: the tree is marshalled as computeParsimony() marshals it (the
// cached engine is reused), every branch's length comes from ONE mpf_branch_lengths call (walk from the root leaf: hook root_id,
// else taxon 0) and is written through set_length.  force == 0: only branches whose current length is negative are rewritten;
// then any length <= 0 becomes 1e-6 (:3626-3629).  Returns the number of rewritten branches.  A multifurcating tree is served once
// the table below is installed.
int mpfitch_fix_negative_branch(PhyloTree *t, int force);

// ---- multifurcating trees (the bootstrap consensus of phyloanalysis.cpp:2263-2307, user trees with polytomies; INTEGRATION.md
// "Branch lengths").  A further, optional table: `neighbors` above hands out three ids and cannot show a node of higher degree.
//     static int hk_degree(const PhyloTree *t, int id) { return (int)node_of(t, id)->neighbors.size(); }
//     static int hk_nei_n(const PhyloTree *t, int id, int *out, int cap)
//         { Node *v = node_of(t, id); int d = (int)v->neighbors.size(); for (int k = 0; k < d && k < cap; k++) out[k] = v->neighbors[k]->node->id; return d; }
//     ... mpfitch_phylotree_install_poly(&poly_hooks);
// With it installed, computeParsimony() (both classes) and mpfitch_fix_negative_branch walk the tree from leaf 0 through
// neighbors_n; a tree with a node of degree above 3 (or fewer than n - 2 inner nodes) goes to the engine as neighbour lists
// (mpf_polytomy_parsimony / mpf_polytomy_branch_lengths: the reference's k-ary rules, evaluated at hook root_id -- the Fitch length
// of such a tree depends on it), a fully resolved one takes the path it took before.  Inner ids need not be contiguous.  Without
// the table a multifurcating tree is refused as before.
struct mpf_phylotree_poly_hooks {
  int (*degree)(const PhyloTree *, int node_id);                                   // neighbors.size()
  int (*neighbors_n)(const PhyloTree *, int node_id, int *out, int cap);           // ids in neighbors[] order, at most cap; returns the degree
};
void mpfitch_phylotree_install_poly(const mpf_phylotree_poly_hooks *hooks);       // NULL (or a table with a NULL entry) uninstalls

// ---- split supports on the host's tree (the summary of a -bb run: IQTree::summarizeBootstrap, iqtree.cpp:4020-4165, and the
// assignment of the supports to the best tree behind it; INTEGRATION.md "Bootstrap summary").  A further, optional table; nothing
// above is rerouted.
//     static void hk_setsup(PhyloTree *t, int id1, int id2, long long support, long long total)
//         { Node *a = node_of(t, id1), *b = node_of(t, id2); Node *inner = ...the end away from the root...;
//           inner->name = convertIntToString((int)(100.0 * support / total + 0.5)); }
//     ... mpfitch_phylotree_install_support(&support_hooks);
struct mpf_phylotree_support_hooks {
  // inner branch id1 -- id2 (id1 the end nearer leaf 0) is held by trees of summed weight `support` out of `total_weight`
  void (*set_support)(PhyloTree *, int id1, int id2, long long support, long long total_weight);
};
void mpfitch_phylotree_install_support(const mpf_phylotree_support_hooks *hooks);   // NULL (or a NULL entry) uninstalls
// The host's (fully resolved) tree is marshalled as computeParsimony() marshals it and handed to mpf_split_support as the target;
// the weighted tree set comes in the engine's record format (e.g. from mpf_ufboot_summary_trees of the engine that ran the search;
// weights NULL = all 1).  Every inner branch is reported once through set_support.  Returns the number of inner branches.
int mpfitch_assign_split_support(PhyloTree *t, int n_trees, const int *backs, const int *weights);
