/*
 * mpfitch.h -- C-ABI of libmpfitch.so, the MI355X-native Fitch parsimony engine
 * that sits behind the parsimony entry points of diepthihoang/mpboot.
 *
 * Plain pointers and sizes only; no C++/torch types cross this boundary.  All
 * state lives in an opaque engine handle that owns its HBM buffers.  Every
 * call returns MPF_OK (0) or a negative MPF_E_* code; mpf_last_error() gives the
 * text.  The library needs a HIP device: mpf_engine_create fails with
 * MPF_E_NO_DEVICE when none is present -- there is no CPU fallback.
 *
 * Conventions shared with the reference (all file:line under the reference tree)
 * ---------------------------------------------------------------------------
 * tip codes   : PLL yVector bytes (pllrepo/src/utils.c:98-137): DNA = 4-bit state
 *               masks 1..15 (15 = gap/N), protein = 0..22 (20 = B, 21 = Z, 22 = gap/X).
 * weights     : tr->aliaswgt, one int per pattern (sprparsimony.cpp:2922-2943).
 * topology    : `back` = int32[3*(2n-1)], record rec = 3*number + slot; number 1..n are
 *               tips (slot 0), n+1..2n-2 inner nodes whose three slots form PLL's
 *               `next` ring (slot -> (slot+1)%3); back[rec] is PLL's `->back`
 *               (pllrepo/src/pll.h:622-701), -1 where unused.
 * tie rule    : MPF_TIE_RANDOM = mpboot (sprparsimony.cpp:2168-2176, :3001-3008,
 *               :3306-3311) drawing random_double(); MPF_TIE_FIRST = strict '<' as in
 *               pllrepo/src/fastDNAparsimony.c:1224, :1803, :1925, on exactly scored candidates -- i.e. the PLL
 *               original's rule with mpboot's evaluate before each scan (sprparsimony.cpp:2285); the original, lacking
 *               that evaluate, can score insertions on not-yet-refreshed vectors and then take another path.
 *
 * Each entry point names the reference interface it replaces.
 */
#ifndef MPFITCH_H
#define MPFITCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPF_ABI_VERSION 8   /* 2: mpf_stats grew (plan_kernel_ms_total, plan_launches), mpf_get_option; 3: mpf_stats grew (climb_*);
                               4: mpf_set_tie_state / mpf_get_tie_state; 5: mpf_ufboot_refine_sweep; 6: mpf_compute_parsimony_at;
                               8: mpf_iq_* (the search loop's own steps between two climbs), mpf_ufboot_adopt, mpf_optimize_spr_many */

enum {
  MPF_OK = 0,
  MPF_E_NO_DEVICE = -1,   /* no HIP device / HIP runtime failure at start-up            */
  MPF_E_INVALID = -2,     /* bad argument (reference: assert / exit(EXIT_FAILURE))      */
  MPF_E_HIP = -3,         /* a HIP call failed                                          */
  MPF_E_NOMEM = -4,
  MPF_E_STATE = -5,       /* call out of order (e.g. no tree set)                       */
  MPF_E_UNSUPPORTED = -6  /* e.g. states outside {4,20}; reference sprparsimony.cpp:575 */
};

/* data types (PLL: pll.h:238-244; partition types "DNA", protein models, "BIN", "MOR" -- iqtree.cpp:515-530):
     MPF_DNA      4 states, tip codes = 4-bit sets 1..15 (15 = undetermined)
     MPF_AA      20 states, codes 0..19, B = 20, Z = 21, 22 = undetermined
     MPF_BIN      2 states (PLL_BINARY_DATA), codes 1, 2, 3 = undetermined            (reference Fitch case 2, sprparsimony.cpp:679-721)
     MPF_GENERIC 32 states (PLL_GENERIC_32), codes 0..31, 32 = undetermined           (reference `default` case, :824-869)
   The binary alphabet runs on the 4-state kernels and multistate data with at most 20 symbols in use on the 20-state kernels
   with the unused state rows empty -- Fitch sets never acquire a state no tip has, so lengths, vectors and trajectories are the
   reference's.  A multistate alignment that uses more than 20 symbols, or any multistate alignment under a cost matrix, runs on
   the 32-state kernels with the reference's own numbering (read-only option "kernel_states" tells which). */
enum { MPF_DNA = 0, MPF_AA = 1, MPF_BIN = 2, MPF_GENERIC = 3 };
enum { MPF_TIE_FIRST = 0, MPF_TIE_RANDOM = 1 };

typedef struct mpf_engine mpf_engine;

typedef struct mpf_config {
  int32_t device;          /* HIP device ordinal                                         */
  int32_t n_taxa;          /* tr->mxtips                                                 */
  int32_t n_patterns;      /* tr->originalCrunchedLength                                 */
  int32_t datatype;        /* MPF_DNA | MPF_AA                                           */
  int32_t keep_all_sites;  /* 1 = !globalParam->sort_alignment (sprparsimony.cpp:2462)   */
  int32_t reserved[3];
} mpf_config;

typedef struct mpf_stats {
  uint64_t insertion_tests;   /* candidates scored (testInsertParsimony equivalents)     */
  uint64_t newview_ops;       /* directional vectors recomputed                          */
  uint64_t scan_launches;
  uint64_t view_launches;
  uint64_t moves_applied;
  uint64_t algorithmic_bytes; /* 6*S*W*4 per insertion test + 3*S*W*4 per newview        */
  double   last_scan_kernel_ms; /* HIP-event time of the most recent scan launch         */
  double   scan_kernel_ms_total;
  double   view_kernel_ms_total;
  double   host_plan_ms_total;   /* wall time spent building scan programs                  */
  double   host_views_ms_total;  /* wall time of update_views() incl. launches and sync     */
  double   host_scan_ms_total;   /* wall time of run_scans() incl. copies and sync         */
  double   host_sweep_ms_total;  /* wall time inside mpf_spr_sweep_scan                      */
  double   plan_kernel_ms_total; /* HIP-event time of the scan-program planner (k_walk_plan)  */
  uint64_t plan_launches;        /* scan launches that ran as planned programs (k_scan_prog)  */
  uint64_t climb_launches;       /* k_climb launches (device-resident sweep segments)         */
  uint64_t climb_steps;          /* steps (speculative batches of prune nodes) inside them    */
  uint64_t climb_nodes;          /* prune nodes they visited                                  */
  uint64_t climb_moves;          /* moves they accepted                                       */
  double   climb_ms_total;       /* wall time of those launches incl. hand-over               */
} mpf_stats;   /* (its size is part of ABI 8: callers hold one on their stack; later counters are read-only options, mpf_get_option) */

const char *mpf_last_error(void);
int mpf_abi_version(void);

/* _allocateParsimonyDataStructures + compressDNA (sprparsimony.cpp:3032-3060, :2828-2973):
   upload codes/weights, drop uninformative sites, bit-pack the tips in HBM. */
int mpf_engine_create(mpf_engine **out, const mpf_config *cfg, const uint8_t *codes /* [n][P] */,
                      const int32_t *weights /* [P] */);
/* Weighted (Sankoff) parsimony, the reference's `-cost <file|e>` mode: same entry points, scores are sums of
   cost-matrix entries.  cost[i*S+j] = cost of i -> j (pllCostMatrix, sprparsimony.cpp:190; loaded and closed under
   the triangle inequality as ParsTree::loadCostMatrixFile does, parstree.cpp:31-95; initializeCostMatrix
   sprparsimony.cpp:159-188).  Kernels: newviewSankoffParsimonyIterativeFastSIMD / evaluateSankoff... (:477-551,
   :880-961), tips as compressSankoffDNA (:2636-2825).  Arithmetic is exact 32-bit (the reference's -short_off
   mode).  A matrix that is not symmetric (the loader accepts any, parstree.cpp:31-95) makes the length of a tree depend
   on where it is rooted: every evaluation is then rooted as the reference roots it -- mpf_score_tree at the start tip's
   edge with the tip as the child, an SPR insertion test at the new node's edge towards the near side of the tested branch
   (testInsertParsimony evaluates p->next->next, :2158), a stepwise-addition test at the new tip's edge (:2993-2997) --, so
   the numbers are the reference's own; mpf_ufboot_attach refuses such an engine.  Serves ParsTree::computeParsimony
   (parstree.cpp:101-116) through mpf_compute_parsimony (symmetric matrices only: IQ-TREE's own Sankoff kernel roots elsewhere). */
int mpf_engine_create_sankoff(mpf_engine **out, const mpf_config *cfg, const uint8_t *codes, const int32_t *weights,
                              const uint32_t *cost /* [S*S] */);
/* _pllFreeParsimonyDataStructures (sprparsimony.cpp:3062-3104) */
void mpf_engine_destroy(mpf_engine *e);

/* _updateInternalPllOnRatchet + re-allocate (sprparsimony.cpp:3022-3029, :3249-3252):
   new pattern weights (ratchet / bootstrap replicate), tips re-packed on the device. */
int mpf_set_weights(mpf_engine *e, const int32_t *weights);

/* packing geometry and test hooks (tips as the reference lays them out, rows of W words) */
int mpf_get_geometry(const mpf_engine *e, int32_t *states, int32_t *words_per_row /* W, multiple of 8 as the
                     reference's parsimonyLength */, int32_t *n_informative, int32_t *words_padded);
int mpf_get_informative(const mpf_engine *e, int32_t *flags /* [P] */);
int mpf_get_tip_vector(mpf_engine *e, int32_t tip /* 1..n */, uint32_t *out /* [S][W] */);

/* pllTreeInitTopologyNewick's result, handed over as record links instead of a Newick string
   (iqtree.cpp:2127-2129). */
int mpf_set_tree(mpf_engine *e, const int32_t *back);
int mpf_get_tree(const mpf_engine *e, int32_t *back);
/* tr->nodep[] as left by earlier calls matters to the reference's visiting order
   (sprparsimony.cpp:2046-2101); this resets it to the state of a fresh PLL instance. */
int mpf_reset_node_order(mpf_engine *e);

/* evaluateParsimony(tr, pr, tr->start, PLL_TRUE) (sprparsimony.cpp:1889-1917, :3277):
   Fitch length of the current tree. */
int mpf_score_tree(mpf_engine *e, uint32_t *score);
/* the same for many topologies in one call (replicates / candidate trees) */
int mpf_score_trees(mpf_engine *e, int32_t n_trees, const int32_t *backs, uint32_t *scores);

/* pllComputePatternParsimony (sprparsimony.cpp:3363-3392): per-pattern Fitch lengths of the
   current tree, ptn_pars[P] (0 for dropped patterns); *total = sum(ptn * weight). */
int mpf_pattern_scores(mpf_engine *e, uint16_t *ptn_pars, int32_t *total);
/* pllComputeSiteParsimony (sprparsimony.cpp:3403-3450): the same lengths per EXPANDED site, i.e. in the packed order
   of the kept patterns with a pattern of weight w repeated w times (the reference's perSitePartialPars row of
   tr->start); entries from the number of expanded sites up to n_sites are 0; *total = their sum. */
int mpf_site_scores(mpf_engine *e, int32_t *site_pars, int32_t n_sites, int32_t *total);

/* int PhyloTree::computeParsimony() (phylotree.cpp:1049-1061; callers precede it with
   initializeAllPartialPars(); clearAllPartialLH(), e.g. iqtree.cpp:2141-2143): Fitch length of the given
   tree from scratch plus the per-pattern lengths the reference leaves in _pattern_pars
   (phylotree.cpp:956-957, :986-987).  `back` may be NULL to use the current tree. */
int mpf_compute_parsimony(mpf_engine *e, const int32_t *back, uint32_t *score, uint16_t *pattern_pars /* [P] or NULL */);
/* The same, evaluated at the edge of leaf `root_taxon` (1-based; 0 = the engine's own start leaf, taxon 1).  Only matters for
   the weighted engine with an ASYMMETRIC cost matrix, where the length of a tree depends on the edge it is rooted at:
   ParsTree::computeParsimony() (parstree.cpp:101-116) roots at IQ-TREE's `root` leaf -- computeParsimonyBranch(root->neighbors[0],
   root), :439-541: min_i( rest[i] + min_j( leaf[j] + cost[i][j] ) ), the rest of the tree as the parent side (rows of the matrix)
   -- which is the orientation of this evaluation (and of evaluateSankoffParsimonyIterativeFastSIMD, sprparsimony.cpp:880-961).
   (ABI 6) */
int mpf_compute_parsimony_at(mpf_engine *e, const int32_t *back, int32_t root_taxon, uint32_t *score, uint16_t *pattern_pars);

/* The IQ-TREE side of the reference stores Alignment::convertState codes (alignment.cpp:839-916):
   DNA 0..3, ambiguity = 4-bit mask + 3, STATE_UNKNOWN 18; protein 0..19, B 20, Z 21, STATE_UNKNOWN 22.
   This maps them to the PLL tip codes the engine takes (the reference does it through a PHYLIP text
   round trip, iqtree.cpp:557-564).  No device needed. */
int mpf_encode_iqtree_states(int32_t datatype, const int8_t *states, int64_t count, uint8_t *codes);

/* random_double() source for MPF_TIE_RANDOM.  Default: our restatement of the SPRNG lcg64
   stream the reference creates in init_random(seed) (tools.cpp:3320-3331).  A host that
   wants to share ITS stream passes a callback (drop-in inside mpboot: random_double). */
int mpf_seed_ties(mpf_engine *e, int32_t tie_mode, int32_t seed);
int mpf_set_rand_callback(mpf_engine *e, double (*fn)(void *), void *arg);
/* Hand-over of the tie stream itself (ABI 4).  random_double() is SPRNG's 64-bit LCG with prime addend
   (sprng/lcg64.c:220, :268: state = state * multiplier + prime, value = state * 2^-64); mpboot creates stream 0 of 1 with
   the default parameter (tools.cpp:3326), i.e. MPF_LCG64_MULTIPLIER / MPF_LCG64_ADDEND (lcg64.c:63, :197;
   primes-lcg64.c:64-68).  A host whose stream has exactly these two constants passes the generator's 64-bit state in
   before a call and takes it back afterwards: the engine then consumes the host's stream draw for draw (ties of
   testInsertParsimony sprparsimony.cpp:2171-2172, of the sweep :3309-3310, of saveCurrentTree iqtree.cpp:3594) WITHOUT a
   call-back per draw -- which is what lets the whole sweep loop run on the device (a call-back keeps it on the host).
   mpf_set_tie_state also removes an installed call-back. */
#define MPF_LCG64_MULTIPLIER 0x27bb2ee687b0b0fdULL
#define MPF_LCG64_ADDEND 3037000493ULL
int mpf_set_tie_state(mpf_engine *e, uint64_t state);
int mpf_get_tie_state(const mpf_engine *e, uint64_t *state);
/* the state of that stream n_draws random_double() calls on, in O(log n_draws) (no engine, no device: pure arithmetic) -- what the
   batched refinement uses to pass over prune-node visits in which nothing but the visit's own accept draw happens */
uint64_t mpf_tie_state_after(uint64_t state, uint64_t n_draws);

/* rearrangeParsimony(tr, pr, p, mintrav, maxtrav) candidates (sprparsimony.cpp:2259-2376):
   every insertion test of prune record `rec`, in the reference's DFS order (p side, then q
   side); q_recs[i] = record q of testInsertParsimony(p, q), mp[i] = tree length after the move.
   *n_p = number of p-side candidates.  Does not change the tree. */
int mpf_spr_scan(mpf_engine *e, int32_t rec, int32_t mintrav, int32_t maxtrav, int32_t cap,
                 int32_t *q_recs, uint32_t *mp, int32_t *n_p, int32_t *n_total);

/* one full sweep of scans over every prune node of the current tree WITHOUT applying moves:
   the throughput primitive bench.py times.  Returns the number of insertion tests and the
   minimum mp seen. */
int mpf_spr_sweep_scan(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint64_t *n_tests, uint32_t *min_mp);
/* the same sweep, handing back every insertion test's tree length: prune nodes in the order pllOptimizeSprParsimony
   visits them (nodep[1 .. 2n-2] after nodeRectifierPars, sprparsimony.cpp:3298), each node's candidates in the
   reference's order (as mpf_spr_scan).  offsets[i] .. offsets[i+1] = candidates of the i-th prune node (offsets has
   2n-1 entries; may be NULL).  *n_tests is always set; mp is filled only if cap >= *n_tests. */
int mpf_spr_sweep_costs(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint64_t cap, uint32_t *mp, uint64_t *offsets,
                        uint64_t *n_tests);
/* tr->nodep[1 .. 2n-2] as nodeRectifierPars leaves it (sprparsimony.cpp:2046-2101): the prune records of a sweep, in order */
int mpf_get_node_order(mpf_engine *e, int32_t *recs /* [2n-2] */);

/* int pllOptimizeSprParsimony(tr, pr, mintrav, maxtrav, iqtree) (sprparsimony.cpp:3244-3319):
   SPR hill climb on the current tree until no sweep improves; the tree is modified in place
   (read it back with mpf_get_tree).  *score = final length (tr->bestParsimony); the function's
   own return value in the reference (startMP) equals it. */
int mpf_optimize_spr(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint32_t *score);
/* pllOptimizeSprParsimony on n INDEPENDENT engines at once (the 100 start trees of a run, phyloanalysis.cpp:1270-1317; the bootstrap
   samples' refinement climbs, iqtree.cpp:2797-2862): each engine with its tree set, its weights, its tie rule and stream, as for
   mpf_optimize_spr -- and each climb makes exactly the moves its own mpf_optimize_spr call would make.  Every climb is one resident
   workgroup of ONE launch (k_climb_many: all its sweeps inside, nodeRectifierPars on the device), fed by the calling thread; a climb
   with more moves than the launch's list holds goes on in a second launch.  Engines the batch cannot take (another
   alignment shape, a tracker attached, the weighted engine, a host random_double() call-back) run their climb alone inside the call.
   final_scores[n_engines]. */
int mpf_optimize_spr_many(mpf_engine **engines, int32_t n_engines, int32_t mintrav, int32_t maxtrav, uint32_t *final_scores);
/* ... one LAUNCH of it (every active climb to its optimum, or to a full move list), for callers with more climbs than engines:
   state[k] in: 0 = engine k takes no part, 1 = a climb STARTS on it now, 2 = its climb goes on; out: 2 = goes on, 0 = done
   (final_scores[k] valid).  A finished engine gets its next tree (and weights, stream) and state 1 before the next round.
   The shape of a round's launch (mpboot_amd/host/many_shape.hpp): one launch has one tile width, number of states, word-major flag
   and device, and a climb keeps the shape it STARTED on until it is done -- its tiles and per-tile scores are laid out for it, and
   the width follows from the row pitch, i.e. from the weights.  The climbs that go on give the shape; a starting climb whose own
   shape is another one (re-weighted across a pitch boundary, option "climb_tile", another alphabet or device) runs alone inside the
   call, as every engine the batch cannot take; where no climb goes on, the first starting engine that fits the batch gives the shape.
   MPF_E_STATE, before anything is touched: two climbs that go on in different shapes; a climb that goes on while its engine was
   packed again (mpf_set_weights between two rounds) or no longer fits the shape it started on (an option changed); state 2 on an
   engine that never started.  MPF_E_INVALID: an engine listed twice (as mpf_optimize_spr_many). */
int mpf_optimize_spr_many_round(mpf_engine **engines, int32_t n_engines, int32_t mintrav, int32_t maxtrav, uint8_t *state, uint32_t *final_scores);

/* _pllComputeRandomizedStepwiseAdditionParsimonyTree(tr, pr, sprDist, iqtree)
   (sprparsimony.cpp:3224-3235, :3107-3209): random addition order from PLL randum(seed),
   stepwise addition, then SPR sweeps with radius spr_dist. */
int mpf_make_parsimony_tree(mpf_engine *e, int64_t seed, int32_t spr_dist, uint32_t *score);
/* stepwise addition only, with the per-taxon checkpoints (best length, insertion record) */
int mpf_stepwise_addition(mpf_engine *e, int64_t seed, uint32_t *best_per_step /* [n+1] */,
                          int32_t *insert_per_step /* [n+1] */, uint32_t *score);

/* double IQTree::optimizeNNI(int &nni_count, int &nni_steps) (reference iqtree.cpp:2173-2302) in MP mode: the NNI hill climb of
   -nni_pars (tools.cpp:2378-2382) and of the ratchet's first climb under -hclimb1_nni (iqtree.cpp:2106-2108), with the defaults
   there (Fitch, nni5 off, leastSquareNNI off).  Every NNI is scored as computeParsimonyBranch scores it (phylotree.cpp:3177-3182,
   getBestNNIForBran :3807-3980); a step scores the whole tree (evalNNIs, :3144-3159: pre-order from taxon root_taxon, 1-based --
   IQ-TREE's root, id root_taxon - 1) or, with speednni (tools.cpp:765), the branches around the last step's moves (:2304-2311);
   positive moves are ordered by std::sort on the length, non-conflicting ones applied together and rolled back when the tree got
   longer than the best of them.  The tree is modified in place; node number = IQ-TREE id + 1, slot = position in neighbors[].
   *score = final length (-curScore), *nni_count / *nni_steps as the reference leaves them (nni_steps = max_steps + 1 when the
   cap is hit; the reference's MAXSTEPS is 50).  MPF_E_UNSUPPORTED on the weighted engine (unless the option "nni_weighted" is
   set, see below) and with a UFBoot tracker attached (the climb under -bb is mpf_ufboot_optimize_nni), MPF_E_STATE without a
   tree, MPF_E_INVALID for a root_taxon outside 1 .. n.
   Options "nni_launches", "nni_rollbacks" and "nni_branches_scored" count scoring launches, rolled-back steps and scored
   branches (mpf_get_option).

   The weighted engine (mpf_engine_create_sankoff; the reference's -cost m -nni_pars).  Option "nni_weighted" (mpf_set_option,
   default 0; accepted and without effect on a Fitch engine): with 0 every NNI entry refuses a weighted engine as above, with 1
   mpf_optimize_nni, mpf_nni_scores and mpf_get_nni_moves are served on it.  Under -cost the search tree is a ParsTree
   (phyloanalysis.cpp:2200-2203), so what optimizeNNI calls are ParsTree's overrides:
     - an NNI is scored by ParsTree::computeParsimonyBranch(node1->findNeighbor(node2), node1) (parstree.cpp:439-541): Sankoff,
       the tree ROOTED AT THE SCORED BRANCH with node2's side as the parent side (the rows of the matrix) and node1's side the
       transformed one -- length = sum_ptn w * min_i( Y[i] + min_j( X[j] + cost[i][j] ) ), X / Y the views of node1 / node2 after
       the swap.  With a matrix that is not symmetric this is NOT the length the tree has at the root leaf;
     - curScore is ParsTree::computeParsimony() (parstree.cpp:101-116), the length at the edge of the leaf root_taxon (what
       mpf_compute_parsimony_at(e, NULL, root_taxon, ..) returns): *score is that length of the final tree;
     - no rollback (iqtree.cpp:2258, `if(globalParam->sankoff_cost_file) continue;`): when the tree after a step's NNIs is longer
       than the best of them promised, the moves STAY, curScore stays the longer length, nni_count does not grow, and the next
       step goes on from there (with speednni: on the branches around these moves).  The climb may therefore end longer than it
       started, and with a non-symmetric matrix it often runs into the step cap.  "nni_rollbacks" does not move on this path;
       read-only option "nni_kept_worse" counts these steps.
   Still MPF_E_UNSUPPORTED on a weighted engine under this option alone: mpf_ufboot_optimize_nni (served under the further option
   "nni_weighted_tracked", see there), mpf_optimize_nni with a tracker attached, mpf_nni_pattern_terms.
   With the option "timing" set, read-only option "nni_kernel_ns" accumulates the HIP-event time of the scoring kernels. */
int mpf_optimize_nni(mpf_engine *e, int32_t root_taxon, int32_t speednni, int32_t max_steps, uint32_t *score, int32_t *nni_count,
                     int32_t *nni_steps);
/* one full evaluation of the current tree (evalNNIs(), iqtree.cpp:3144-3159, with getBestNNIForBran, phylotree.cpp:3807-3980):
   branch i in the reference's order joins node1[i] and node2[i] (node numbers); len[2i + k] = tree length after its move k (k = 0:
   node1's first neighbour other than node2 swapped with node2's first other neighbour, k = 1: with its second).  *n = number of
   inner branches, always set; the arrays are filled when cap >= *n.  On a weighted engine under "nni_weighted": the two FULL weighted
   lengths, each rooted at its branch (node2[i]'s side the parent), as described at mpf_optimize_nni. */
int mpf_nni_scores(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len /* [2 * cap] */,
                   int32_t *n);
/* DIAGNOSTIC, for tests of the kernel alone -- no part of mpboot's flow, and nothing a host should build on: mpf_nni_scores by
   the mask-writing kernel of the tracked climb (k_nni_eval_masks), with what it writes for the tracker read back per pattern: terms[(3 i + r) * n_patterns + p] = number (0..3) of the three joins at branch i without a common state at
   pattern p -- r = 0: in the current tree, r = 1 / 2: after move 0 / 1.  Per pattern, length(tree after move k) = length(current
   tree) - terms[3 i] + terms[3 i + 1 + k].  0 for patterns the engine drops.  Filled when cap >= *n. */
int mpf_nni_pattern_terms(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len /* [2 * cap] */,
                          uint8_t *terms /* [3 * cap][n_patterns] */, int32_t *n);
/* DIAGNOSTIC, the weighted counterpart of mpf_nni_pattern_terms (same sizing protocol, same standing): mpf_nni_scores by the
   row-writing kernel of the tracked weighted climb (k_snk_nni_eval_vals), with what it writes for the tracker read back per
   ORIGINAL pattern as 16-bit values, rows[r * n_patterns + p]: r = 0 the current tree at the edge of the leaf root_taxon (the row
   ParsTree::computeParsimony() writes, parstree.cpp:101-116), r = 1 + 2 i + k the tree after move k of branch i rooted at that
   branch with node2[i]'s side the parent (the minima ParsTree::computeParsimonyBranch writes to _pattern_pars, parstree.cpp:460-461,
   :482-529).  sum_p weight[p] * rows[r][p] is the row's length (len[2 i + k] for a candidate).  0 for patterns the engine drops.
   rows is filled when cap >= *n ([1 + 2 * cap][n_patterns]).  Weighted engines under "nni_weighted" and "nni_weighted_tracked"
   only; MPF_E_UNSUPPORTED on a Fitch engine. */
int mpf_nni_pattern_lengths(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len /* [2 * cap] */,
                            uint16_t *rows /* [1 + 2 * cap][n_patterns] */, int32_t *n);
/* every swap (PhyloTree::doNNI, phylotree.cpp:3715-3742) the last mpf_optimize_nni made, in order, the reverting swaps of a
   rollback (iqtree.cpp:2271-2272) included: the neighbours in slot1[i] of node1[i] and slot2[i] of node2[i] traded places.
   Replaying them on the start tree gives the final tree.  *n is always set; the arrays are filled up to cap entries. */
int mpf_get_nni_moves(const mpf_engine *e, int32_t cap, int32_t *node1, int32_t *slot1, int32_t *node2, int32_t *slot2, int32_t *n);

/* ---- parsimony branch lengths: PhyloTree::fixNegativeBranch (phylotree.cpp:3597-3633), which an MP run calls on the first start
   tree (phyloanalysis.cpp:1180; :1153 for the IQ-TREE start tree), on each further initial candidate (:1336), on the consensus tree
   (:2280) and under -parsbran (:1501).  It calls computeParsimonyBranch(.., &branch_subst) once per branch; here every branch of
   the current (complete, bifurcating) tree is scored by ONE launch on the directional vectors the engine keeps (k_branch_subst /
   k_snk_branch_eval), after a refresh of whatever is stale.

   Branch order: fixNegativeBranch(force, node = root, dad = NULL) is a pre-order walk from the root leaf root_taxon that takes
   the neighbours other than dad in neighbors[] slot order; each branch is met once, from its root side.  That is the order of
   mpf_nni_scores with the pendant branches included: 2 n_taxa - 3 entries, node1[i] the end nearer the root leaf, node2[i] the
   other end (node numbers).

   subst[i] is what the reference's computeParsimonyBranch stores in *branch_subst at that call:
     - Fitch engine (PhyloTree::computeParsimonyBranch, phylotree.cpp:938-1047): the sum over patterns of frequency x [the state
       sets of the two sides have no state in common], taken before the two subtree scores are added (:1041-1044); the leaf swap
       (:945-953) does not change it.  The sum runs over the patterns the engine KEEPS under the weights in force (after
       mpf_set_weights: the new ones).  An engine made with keep_all_sites = 1 counts uninformative patterns too, as IQ-TREE
       does; an engine that drops uninformative patterns counts the kept ones only -- a dropped pattern with k > 1 singleton
       states puts its changes on pendant branches in IQ-TREE's count and on none here;
     - weighted engine (ParsTree::computeParsimonyBranch, parstree.cpp:439-541): *branch_subst = tree_pars (:534-535), the FULL
       weighted length of the tree rooted at that branch, not a per-branch count:
         sum_ptn w * min_i( min_j( node_branch[j] + cost[i][j] ) + dad_branch[i] )
       For an inner node2[i], dad_branch is the subtree at node2 (enters as it is) and node_branch the rest of the tree (the
       transformed side); for a leaf node2[i] the swap at :449-457 makes the leaf the transformed side.  With a symmetric matrix
       every branch gives the one tree length; with a non-symmetric one the branches differ.
   *n = 2 n_taxa - 3, always set; the arrays are filled when cap >= *n (the sizing protocol of mpf_nni_scores).
   MPF_E_STATE without a tree or on a partial tree (a stepwise addition under way); an attached UFBoot tracker does not matter --
   nothing is booked, no topology changes.  Options: "brlen_tile" (-1 | 0 | 1 | 2 | 4, the kernel shape, as "nni_tile"), read-only
   "brlen_launches", and under "timing" read-only "brlen_kernel_ns" (HIP-event time of the kernel). */
int mpf_branch_substitutions(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *subst,
                             int32_t *n);
/* the lengths fixNegativeBranch(force = true) gives those branches (phylotree.cpp:3608-3614), in double precision on the host, with
   N = n_sites (the caller's getAlnNSite()) and S the alignment's number of states:
     bl = subst > 0 ? subst / N : 1 / N;  z = S / (S - 1);  x = 1 - z bl;  if (x > 0) bl = -log(x) / z;  if (bl < 1e-6) bl = 1e-6
   (MIN_BRANCH_LEN, phylotree.h:35).  unit_cost_parstree != 0 on a Fitch engine: the tree is a ParsTree under -cost fitch | e, which
   scores on the Fitch engine but takes ParsTree's rule -- every branch's subst is the tree's Fitch length.  Ignored on a weighted
   engine.  Same order, sizing protocol and errors as mpf_branch_substitutions. */
int mpf_branch_lengths(mpf_engine *e, int32_t root_taxon, int32_t n_sites, int32_t unit_cost_parstree, int32_t cap, int32_t *node1,
                       int32_t *node2, double *length /* [cap] */, int32_t *n);
/* Multifurcating trees.  Every -bb run of the reference ends on one: computeConsensusTree writes the bootstrap consensus, the host
   reads it back, calls fixNegativeBranch(true) and optimizeAllBranches() -- in MP mode computeParsimony() -- and prints "Parsimony
   score of consensus tree" (phyloanalysis.cpp:2263-2307); user trees with polytomies reach -comppars, -wspars-user-tree and
   -parsbran alike.  back[] (three records per inner node) cannot hold such a tree, so it is handed over as CSR neighbour lists:
   tips are nodes 1 .. n_taxa, inner node i (0-based) is node n_taxa + 1 + i, its neighbours are nbr[first[i] .. first[i + 1]) in
   the host's neighbors[] order, entries are node numbers; 1 <= n_inner <= n_taxa - 2.  MPF_E_INVALID with a message unless every
   inner degree is at least 3, adjacency is symmetric, every tip occurs exactly once, there are n_taxa + n_inner - 1 edges and the
   tree is connected.

   The rules at a node of degree > 3 are the reference's generic ones, not the bifurcating rule on some binary resolution:
     - Fitch engine (PhyloTree::computePartialParsimony, phylotree.cpp:869-931; the DNA and protein fast paths take degree 3 only,
       :708, :781): a node's set is the AND of all its children's sets; where that is empty it is the OR of all of them and ONE
       step is counted, whatever the degree.  This is not the length of a hard polytomy (it undercounts), and it depends on the
       root leaf; it is what the reference prints.  The reference's is_const skip (:845, :900) is not applied: see INTEGRATION;
     - weighted engine (ParsTree::computePartialParsimony, parstree.cpp:191-214): a node's cost row is the sum over all children
       of the child's min-plus transform.
   A tree whose inner nodes all have degree 3 gives, bit for bit, what mpf_compute_parsimony_at / mpf_branch_substitutions /
   mpf_branch_lengths give for the same tree.  The calls are stateless towards the engine's own tree: mpf_get_tree, mpf_score_tree
   and mpf_branch_substitutions give afterwards what they gave before (the engine's vectors are made again on the next call that
   needs them), and an attached UFBoot tracker books nothing.  No current tree is needed.

   mpf_polytomy_parsimony: computeParsimony() at the root leaf, computeParsimonyBranch(root->neighbors[0], root)
   (phylotree.cpp:1049-1061, :938-1047; parstree.cpp:439-541): the length, and _pattern_pars with 0 for dropped patterns as
   mpf_compute_parsimony_at returns them.  On a weighted engine with a non-symmetric matrix the orientation is the one
   mpf_compute_parsimony_at documents (the rest of the tree as the parent side). */
int mpf_polytomy_parsimony(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, uint32_t *score,
                           uint16_t *pattern_pars /* [P] or NULL */);
/* fixNegativeBranch (phylotree.cpp:3597-3633) on such a tree: the contract of mpf_branch_substitutions and mpf_branch_lengths -- the
   walk (pre-order from the root leaf, neighbours in list order, node1 the root side), the meaning of subst on each engine, the leaf
   swap, the sizing protocol, the length formula and unit_cost_parstree -- with *n = n_taxa + n_inner - 1 and the two sides of a
   branch made by the k-ary rule above (all directed views of the tree: ONE launch of k_poly_views / k_poly_snk_views, then the one
   branch launch).  Options: "poly_tile" (0 | 4 | 8 | 16 | 32, words of a row per workgroup), read-only "poly_launches" and
   "poly_views", and under "timing" read-only "poly_view_ns" / "poly_branch_ns"; read-only "sankoff_packed" (weighted engine: 1 while
   the store holds two 16-bit costs per word, i.e. "sankoff_short" is on and 3 n_taxa (max cost + 1) < 2^16). */
int mpf_polytomy_branch_substitutions(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t cap,
                                      int32_t *node1, int32_t *node2, uint32_t *subst, int32_t *n);
int mpf_polytomy_branch_lengths(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t n_sites,
                                int32_t unit_cost_parstree, int32_t cap, int32_t *node1, int32_t *node2, double *length /* [cap] */, int32_t *n);
/* Taxon insertion: what it costs to attach taxon t to branch b of a tree that does not hold t yet.  The reference asks this in
   PhyloTree::addTaxonMPFast (phylotree.cpp:1322-1378), which tries the taxon on every branch in a pre-order walk from the root
   leaf -- first (root leaf, its neighbour), then FOR_NEIGHBOR_IT(node, dad, it) in neighbors[] order, the walk of
   fixNegativeBranch -- calls computeParsimonyBranch at each and keeps the FIRST strictly smallest score (no random draw).  On top
   of it sit PhyloTree::computeParsimonyTree (phylotree.cpp:1243-1320: the start tree of -starttree PARS, tools.cpp:1476-1489, and
   the fall-back when PLL cannot take the data, phyloanalysis.cpp:1671-1681) and IQTree::reinsertLeavesByParsimony
   (iqtree.cpp:981-1016).

   The backbone is handed over as the lists of mpf_polytomy_* with ONE relaxation: tips may be absent.  MPF_E_INVALID unless every
   tip occurs at most once, at least three occur, adjacency is symmetric, there are tips + n_inner - 1 edges, the tree is connected
   and root_taxon is one of the tips present.  Every inner node must have degree exactly 3, else MPF_E_UNSUPPORTED (the k-ary Fitch
   rule depends on the root; an insertion cost on such a tree is not what any reference function computes).  Query taxa are rows of
   the engine's alignment, absent from the backbone and pairwise distinct (else MPF_E_INVALID); n_query = 0 is legal.

   The weighted engine (mpf_engine_create_sankoff; -cost m with -starttree PARS or a leaf re-insertion).  Option "place_weighted"
   (mpf_set_option, default 0): with 0 the three calls answer MPF_E_UNSUPPORTED with a message, as they always did; with 1 they are
   served (a Fitch engine accepts and ignores the option).  The rule: addTaxonMPFast lends added_node the two directed views of the
   branch and calls computeParsimonyBranch(added_node->neighbors[0], added_node), neighbors[0] being the new taxon; on a ParsTree
   the leaf swap (parstree.cpp:449-457) makes the taxon the transformed side and the rest of the tree the parent side (the rows of
   the matrix).  With A, B the two directed views of branch b, T the query tip's cost row (0 for a state in its set, highest_cost
   otherwise) and m(v)[z] = min_x(v[x] + cost[z][x]) the stored min-plus transform,
       cost(q, b) = sum over patterns of w * min_i( m(T_q)[i] + m(A_b)[i] + m(B_b)[i] ).
   This is the FULL length of the completed tree, rooted at the NEW TAXON'S edge: it equals mpf_compute_parsimony_at(completed tree,
   root_taxon = the query).  There is no additive backbone length; with a matrix that is not symmetric the evaluation edge matters,
   and the backbone's root_taxon only fixes the walk order and *tree_length (the backbone's own weighted length at root_taxon, as
   mpf_polytomy_parsimony gives it).  mpf_iq_parsimony_tree: length_per_step[0] = the star's length at the leaf order[0];
   length_per_step[k - 2] = the score addTaxonMPFast returned for order[k], i.e. the length of the tree of the first k + 1 taxa
   evaluated at order[k]'s edge (not a sum of a length and a difference); *score = the last.  All views come from one k_poly_snk_views
   launch, the Q x B x patterns min-plus product from k_place_costs over its min-plus algebra (place.hip), which adds m(A) and m(B) on its way into LDS
   and transforms nothing.  The 16-bit store ("sankoff_packed") needs no further condition: the sum of three transforms over
   disjoint sides is what its guard 3 n_taxa (max cost + 1) < 2^16 covers.

   Fitch length does not depend on the root, so with A, B the two directed views of a branch and T the query tip the length is
   len(backbone) + #sites where X and T share no state, X = A & B where that is non-empty, else A | B: all views come from one
   k_poly_views launch, the Q x B x sites popcount product from k_place_costs (place.hip), which joins A and B on its way into LDS.
   Patterns follow the contract of mpf_branch_substitutions: an engine made with keep_all_sites = 1 counts what IQ-TREE counts, one
   that drops uninformative patterns counts the kept ones (on data without ambiguity-only variation the difference is a constant
   per query and the chosen branch is the same).  Stateless towards the engine's own tree exactly as the polytomy calls are.
   Options: "place_tile" (0 = from the number of outputs | 1 = narrow, 4 queries x 16 branches per workgroup | 2 = wide, 64 x 64 for 4
   state rows, 32 x 32 for 20 and 32; on the weighted engine 64 x 64 for 4 and 20 state rows, 32 x 32 for 32), "place_weighted" (above),
   read-only "place_shape" (the shape the last product launch ran: 1 narrow | 2 wide; 0 before the first), read-only "place_launches" and, under "timing", "place_kernel_ns".

   mpf_insertion_costs: every insertion test of addTaxonMPFast for each query taxon: cost[q * cap + i] = length of the backbone with
   query_taxa[q] attached to branch i; branches in the order of mpf_polytomy_branch_substitutions for the same lists (*n = 2 m - 3
   for m tips); sizing protocol of mpf_nni_scores (arrays filled when cap >= *n); *tree_length = length of the backbone. */
int mpf_insertion_costs(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon,
                        int32_t n_query, const int32_t *query_taxa, int32_t cap, int32_t *node1, int32_t *node2,
                        uint32_t *cost, int32_t *n, uint32_t *tree_length);
/* addTaxonMPFast's answer per query: the first minimum in walk order (best_branch = its index in that order, best_node1 / 2 its
   ends, best_length the length of the tree with the taxon there); the minimum is taken on the device (k_place_best: the lowest
   branch index among the minima), the Q x B matrix is not copied back.  Outputs may be NULL. */
int mpf_place_taxa(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon,
                   int32_t n_query, const int32_t *query_taxa, int32_t *best_branch, int32_t *best_node1,
                   int32_t *best_node2, uint32_t *best_length, uint32_t *tree_length);
/* PhyloTree::computeParsimonyTree.  tie_state != NULL: order[] is filled by my_random_shuffle (tools.h:2107-2113: identity, then for
   i = n - 1 .. 1 swap(order[i], order[random_int(i + 1)])) from that stream (n - 1 draws, state advanced, as mpf_iq_random_nnis
   hands a stream over); NULL: order[] (1-based, a permutation) is taken as given.  The start is the star of order[0 .. 2] rooted at
   the leaf order[0]; every later taxon is tried on every branch (all views made again, one Q = 1 placement) and put at the first
   minimum: the new inner node takes target_dad's place in target_node's list and the other way round, in place, and lists
   [new taxon, target_node, target_dad].  Out: the tree as lists in the reference's neighbors[] order (first[n - 1], nbr[3 (n - 2)];
   inner node 0 = the centre of the first three, inner node k = the node made for order[k + 2]), length_per_step[j] = length of
   the tree of the first j + 3 taxa (j = 0 .. n - 3), *score = the last.  The engine's own tree is not replaced: convert the lists
   (record slot = list position) and call mpf_set_tree to climb from it. */
int mpf_iq_parsimony_tree(mpf_engine *e, uint64_t *tie_state, int32_t *order, int32_t *first, int32_t *nbr,
                          uint32_t *length_per_step, uint32_t *score);
/* Tree bisection and reconnection (TBR) on the engine's tree.  THERE IS NO REFERENCE FUNCTION: MPBoot 1.1.1 has SPR and NNI only.
   A visit is a record rec, its edge (rec, q = back[rec]) and a radius maxtrav in 1 .. 255.  Cut the edge.  g_recs lists the
   branches of rec's part and f_recs those of q's part, each as rearrangeParsimony's one side enumerates them with mintrav = 1
   (addTraverseParsimony's order, sprparsimony.cpp:2208-2218; for q's part that is one level nearer than the 2 the SPR scan starts
   from).  cost is the (1 + n_f) x (1 + n_g) matrix, row-major, of the length of the tree that joins the middle of f_recs[i - 1] to
   the middle of g_recs[j - 1]; index 0 of either side means the part's own root.  So row 0 is testInsertParsimony
   (sprparsimony.cpp:2106-2188) of rec on every g_recs[j - 1], the p side of mpf_spr_scan; column 0 is the q side where the lists
   coincide (depth >= 2; rearrangeParsimony, sprparsimony.cpp:2259-2376); cost[0][0] is the current length.  The tree of an entry is
   apply_spr(apply_spr(back, rec, g), q, f), a step whose record is "none" skipped.  All directional views are resident, so an
   entry costs one popcount over two root sets: k_tbr_roots writes the root sets R(.) of both parts into a scratch store,
   k_tbr_costs forms the matrix, cost = sc[rec] + sc[q] + #sites where R_q(f) and R_rec(g) share no state (tbr.hip).
   The weighted engine (mpf_engine_create_sankoff; -cost m).  Option "tbr_weighted" (mpf_set_option; default 0, no effect on a
   Fitch engine): with 0 a weighted engine answers MPF_E_UNSUPPORTED as before.  With 1 it serves all five entries below over the
   min-plus algebra, m(v)[z] = min_x(v[x] + cost[z][x]) the stored transform with the viewer as the parent: k_tbr_snk_roots forms
   MU[0] = m(vec[own]), U = MU[d - 1] + m(vec[sib]), MU[d] = m(U) and the root set R = MU[d] + m(vec[own]) -- a root set of rec's part
   is stored as m(R) --, k_tbr_costs forms cost[i][j] = sum over the patterns of weight x min_x(R_q(f)[x] + m(R_rec(g))[x]): the FULL
   weighted length of the joined tree, nothing added; cost[0][0] is the current length, row 0 and column 0 are the weighted
   mpf_spr_scan's tests.  Both stores ("sankoff_short").  Symmetric cost matrices only: with a matrix that is not symmetric the
   length depends on the edge it is evaluated at and TBR has no reference function that would fix one -- MPF_E_UNSUPPORTED, the
   message says "not symmetric".
   An engine with a UFBoot tracker attached answers MPF_E_UNSUPPORTED to these five entries on either engine (nothing would be
   booked): under -bb the sweep and the climb are mpf_ufboot_tbr_sweep and mpf_ufboot_optimize_tbr, below.
   maxtrav outside 1 .. 255: MPF_E_INVALID.  Options: "tbr_tile" (0 = per visit from the padded outputs | 1 =
   narrow, 4 x 16 per workgroup | 2 = wide, 64 x 64 for 4 state rows, 32 x 32 for 20 and 32; on the weighted engine 64 x 64 for 4 and
   20 state rows, 32 x 32 for 32), "tbr_weighted" (above), "tbr_chunk_vectors" (the most
   root-set vectors a chunk of a sweep may hold, 0 = 256 MiB worth; a visit that needs more is a chunk of its own; results do not
   depend on it), read-only "tbr_chunks" (chunks of the last sweep), "tbr_launches" and, under "timing", "tbr_kernel_ns".

   mpf_tbr_scan: one visit's lists and matrix.  *n_f and *n_g are always set; the lists are filled if cap_f >= *n_f and
   cap_g >= *n_g, and cost (may be NULL: the lists alone) only then, as mpf_spr_sweep_costs fills mp.  The tree does not change. */
int mpf_tbr_scan(mpf_engine *e, int32_t rec, int32_t maxtrav, int32_t cap_f, int32_t cap_g, int32_t *f_recs, int32_t *g_recs,
                 uint32_t *cost, int32_t *n_f, int32_t *n_g);
/* No reference function (above).  The best of every visit of a sweep over the records of mpf_get_node_order, in that order (the SPR
   sweep's order, sprparsimony.cpp:3298): the minimum over all entries of the visit's matrix except [0][0], ties to the lowest
   row-major index (k_tbr_best); best_f / best_g = its records, -1 for "none" (row 0 / column 0: an SPR move of
   sprparsimony.cpp:2106-2188, :2208-2218, :2259-2376).  A visit with a 1 x 1 matrix has best_cost 0xFFFFFFFF and records -1.  All
   three arrays have 2 n - 2 entries; only these three words per visit leave the device.  *n_pairs (may be NULL) = matrix entries
   scored.  The sweep runs in chunks of consecutive visits ("tbr_chunk_vectors").  The tree does not change. */
int mpf_tbr_sweep_best(mpf_engine *e, int32_t maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs);
/* No reference function (above; with f_rec = -1 or g_rec = -1 it is one removeNodeParsimony + insertParsimony, the move of
   sprparsimony.cpp:2106-2188, :2208-2218, :2259-2376).  Edits the engine's tree to apply_spr(apply_spr(back, rec, g_rec), back[rec],
   f_rec) and returns its length: equal in every observable to mpf_set_tree of the edited back[] followed by mpf_score_tree.  A pair
   that is not in the visit's lists at radius 255: MPF_E_INVALID, tree unchanged. */
int mpf_apply_tbr(mpf_engine *e, int32_t rec, int32_t f_rec, int32_t g_rec, uint32_t *score);
/* No reference function (above; a climb that only ever finds its best in row 0 or column 0 makes the moves of
   sprparsimony.cpp:2106-2188, :2208-2218, :2259-2376).  Steepest descent: take mpf_tbr_sweep_best's lowest cost (the lowest visit
   index among equals) and apply it if it is strictly below the current length, otherwise stop.  max_moves <= 0: no limit.
   Deterministic: draws nothing from the tie stream and leaves it untouched.  *score = final length, *n_moves = moves made; they are
   read back with mpf_get_tbr_moves. */
int mpf_optimize_tbr(mpf_engine *e, int32_t maxtrav, int32_t max_moves, uint32_t *score, int32_t *n_moves);
/* moves of the last mpf_optimize_tbr: (rec, f_rec, g_rec, length after the move); protocol of mpf_get_moves */
int mpf_get_tbr_moves(const mpf_engine *e, int32_t cap, int32_t *rec, int32_t *f_rec, int32_t *g_rec, uint32_t *score,
                      int32_t *n_moves);
/* TBR under -bb (a UFBoot tracker attached; host/tbr.cpp, k_tbr_masks in tbr.hip).  No reference function, so this is the
   definition.  A tracked sweep hands EVERY entry of every visit's matrix to IQTree::saveCurrentTree's rule (iqtree.cpp:3271-3731):
   the visits in the order of mpf_get_node_order, a visit's entries in row-major order from [0][0].  [0][0] is the current tree under
   its own length (as rearrangeParsimony opens every prune node with a booking of the current tree, sprparsimony.cpp:2285-2289),
   every other entry the joined tree under cost[i][j]; a visit with a 1 x 1 matrix books the current tree only.  A booking is the
   cut-off filter, a new entry of treels_logl, then the per-sample update rule, whose tie draws come from the engine's one stream in
   that order.  Duplicated topologies are booked as often as they occur (row 0 and column 0 repeat SPR tests).
   Per site, pattern_pars(T_ij) = pattern_pars(T) - M[0][0] + M[i][j] with M[i][j] the 1-bit-per-site word "R_q(F_i) and R_rec(G_j)
   share no state" whose popcount k_tbr_costs takes: k_tbr_masks writes that word for every entry that passes the cut-off and for each
   visit's [0][0], and the tracker's product, extraction and replay run on those rows as they do on the SPR scan's and the NNI step's.
   The entries are booked in batches of at most "tbr_book_rows" consecutive entries (option; 0 = the mask rows and the product of a
   batch each stay within 256 MiB); books and draws do not depend on it, nor on "tbr_chunk_vectors".  Read-only options "tbr_booked"
   (trees handed over since the attach), "tbr_book_batches" and, under "timing", "tbr_masks_ns", "tbr_product_ns", "tbr_extract_ns".
   Served: the default update rule, -mulhits, a logl_cutoff, -cutoff_from_btrees.  On a suspended tracker (mpf_set_weights left an
   attach-time pattern without a site, or re-weighted patterns with ratchet booking off) both run as their plain counterparts and
   book nothing.  MPF_E_STATE without a tracker or a tree.  MPF_E_UNSUPPORTED, the message naming the case: the weighted engine
   (unless its options "tbr_weighted" and "tbr_weighted_tracked" are both 1: see mpf_tbr_pattern_lengths below), -storetrees, -mulhits -topboot, -distinct_iter_top_boot, a sample-sharded tracker, re-weighted (ratchet) patterns with ratchet
   booking on.
   mpf_ufboot_tbr_sweep: mpf_tbr_sweep_best (same outputs) with every entry booked.  The tree does not change. */
int mpf_ufboot_tbr_sweep(mpf_engine *e, int32_t maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs);
/* mpf_optimize_tbr's steepest descent with every sweep booked as above, the last sweep, which finds nothing, included (a climb that
   stops at max_moves runs no sweep behind its last move).  The climb itself draws nothing.  Moves: mpf_get_tbr_moves. */
int mpf_ufboot_optimize_tbr(mpf_engine *e, int32_t maxtrav, int32_t max_moves, uint32_t *score, int32_t *n_moves);
/* DIAGNOSTIC, with the standing of mpf_nni_pattern_terms: the rows k_tbr_masks writes for ONE visit (every entry, [0][0] included),
   read back per original pattern: terms[(i * (1 + *n_g) + j) * n_patterns + p] = the bit of M[i][j] at pattern p's first site, 0 for
   a pattern the engine drops, so that pattern_pars(T_ij) = pattern_pars(T) - terms[0][0] + terms[i][j].  *n_f and *n_g (the lists'
   sizes, as mpf_tbr_scan gives them) are always set; terms is filled if cap_entries >= (1 + *n_f) * (1 + *n_g).  Works with or
   without a tracker and books nothing; Fitch engines only. */
int mpf_tbr_pattern_terms(mpf_engine *e, int32_t rec, int32_t maxtrav, int64_t cap_entries, uint8_t *terms, int32_t *n_f, int32_t *n_g);
/* TBR under -bb on the weighted engine (-cost m -bb; host/tbr.cpp, k_tbr_snk_vals in tbr.hip).  Option "tbr_weighted_tracked"
   (mpf_set_option; default 0, no effect on a Fitch engine): with 0, or with "tbr_weighted" 0, a weighted engine answers
   MPF_E_UNSUPPORTED to mpf_ufboot_tbr_sweep and mpf_ufboot_optimize_tbr with the message it had.  With both options 1 the two
   entries are served under the definition above, unchanged: every entry of every visit's matrix, visits in sweep order, entries
   row-major from [0][0], [0][0] the current tree under its own length, duplicates booked as often as they occur.  On this engine
   an entry's length is cost[i][j], the full weighted length mpf_tbr_scan returns; its _pattern_pars row is, per pattern,
   min_x(R_q(F_i)[x] + m(R_rec(G_j))[x]), the terms whose weighted sum cost[i][j] is (k_tbr_snk_vals writes them as 16-bit values for
   the entries that pass the cut-off and one home row per visit; k_vals_planes and K runs of k_bitgemm form the product, as for the
   weighted tracked NNI climb); a tree's score under sample b is its OWN product row.  Symmetric cost matrices only ("tbr_weighted"'s
   condition): the current tree's row is then the same at every cut edge.  Served and refused as above -- default rule, -mulhits, a
   cut-off, -cutoff_from_btrees; a suspended tracker runs the plain weighted sweep or climb and books nothing; MPF_E_UNSUPPORTED by
   name for a matrix that is not symmetric, -storetrees, -mulhits -topboot, -distinct_iter_top_boot, a sample-sharded tracker, a
   ratchet state -- and, in the 32-bit store ("sankoff_short" 0 or costs too large for the 16-bit store), for an engine with
   n_taxa x (largest cost + 1) >= 65536, whose per-pattern lengths might not fit their 16-bit rows (nothing is ever truncated).
   "tbr_book_rows" 0 on this engine: the 16-bit rows, the bit planes and the product of a batch each stay within 256 MiB.
   mpf_tbr_pattern_lengths: DIAGNOSTIC, the counterpart of mpf_nni_pattern_lengths with the calling shape and standing of
   mpf_tbr_pattern_terms: the rows k_tbr_snk_vals writes for ONE visit (every entry, [0][0] included), read back per original
   pattern: rows[(i * (1 + *n_g) + j) * n_patterns + p] = the per-pattern length of the tree of entry [i][j] at pattern p, 0 for a
   pattern the engine drops; the weighted sum of a row is cost[i][j].  Works with or without a tracker and books nothing; weighted
   engines with both options only (a Fitch engine: MPF_E_UNSUPPORTED, it has mpf_tbr_pattern_terms, which stays Fitch only). */
int mpf_tbr_pattern_lengths(mpf_engine *e, int32_t rec, int32_t maxtrav, int64_t cap_entries, uint16_t *rows, int32_t *n_f, int32_t *n_g);
/* The summary of a -bb run: split supports and the bootstrap consensus tree.  The reference weights the booked trees by the samples
   that point to them (IQTree::summarizeBootstrap, iqtree.cpp:4020-4165), turns every tree into Split objects through its Newick
   string and counts them in a hash map (MTreeSet::convertSplits, mtreeset.cpp:288-470), and builds the consensus from the counted
   splits (computeConsensusTree, phyloanalysis.cpp:2488-2600, called at :2263-2267).  Here the trees are taken as the engine holds
   them -- backs[n_trees][3 (2 n_taxa - 1)], each checked as mpf_set_tree checks it and for being ONE tree over all tips
   (MPF_E_INVALID) -- and counted on the device (k_split_keys, k_split_insert, k_split_count, k_split_bits).  The results are exact:
   a 64-bit key only routes a cluster to a table slot, equality is decided on the whole sets, and a true key collision goes through
   an overflow list that the host resolves by whole-set comparison.

   A split is the set of tips on the side of an inner branch that does not hold tip 1, as ceil(n_taxa / 32) words: bit (t - 1) % 32
   of word (t - 1) / 32 means tip t.  weights[n_trees]: int32 >= 0 (a negative one: MPF_E_INVALID), NULL = all 1; a tree of weight 0
   contributes nothing.  Counts and supports are 64-bit; *total_weight = the sum of the weights.  MPF_E_UNSUPPORTED above 2047 taxa
   (a tree's records, 12 (2 n - 1) bytes, and its walk's stack, 8 n + 16 bytes, are kept in 64 KiB of LDS) and above 2^27
   clusters, n_trees (n_taxa - 3), in one call.  No current tree is needed, none is changed, an attached tracker books nothing.
   Test option "split_key_bits" (default 64; 1 .. 63 masks the keys so that they collide), read-only options "split_overflow" (length
   of the last call's overflow list), "split_launches" and, under "timing", "split_keys_ns" / "split_count_ns" / "split_bits_ns".
   Trees that are not fully resolved (the consensus tree itself, user trees with polytomies) go through the mpf_*_set calls below.

   mpf_split_counts (MTreeSet::convertSplits with SW_COUNT): the distinct splits ordered by count descending, then by their words
   ascending as unsigned, word 0 first -- that order is the contract.  *n_distinct is always the full number; the first
   min(*n_distinct, cap) rows of bits / count are written (cap = 0: the numbers only, bits and count may be NULL). */
int mpf_split_counts(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, int32_t cap,
                     uint32_t *bits /* [cap][ceil(n_taxa / 32)] */, int64_t *count /* [cap] */, int32_t *n_distinct, int64_t *total_weight);
/* The supports the reference writes onto the best tree's branches (the assignment behind summarizeBootstrap: PhyloTree's
   createBootstrapSupport / assignBranchSupport family): for every branch of target_back, in the walk order of
   mpf_branch_substitutions from root_taxon = 1 (so that the two calls' arrays line up; *n = 2 n_taxa - 3, sizing protocol as there),
   the summed weight of the trees that hold the branch's split; -1 on a leaf branch.  target_back need not be one of the trees. */
int mpf_split_support(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, const int32_t *target_back, int32_t cap,
                      int32_t *node1, int32_t *node2, int64_t *support, int32_t *n, int64_t *total_weight);
/* computeConsensusTree: the splits with count <= threshold * total_weight are dropped (mtreeset.cpp:301-312), then
   SplitGraph::findMaxCompatibleSplits (splitgraph.cpp:615-648): the splits are taken by decreasing count and each one compatible with
   all kept so far is kept.  threshold = 0 is the greedy consensus the reference writes to .contree; threshold >= 0.5 is the majority
   rule, which is unique.  Among equal counts the reference takes the order its sort leaves; here it is the contract order of
   mpf_split_counts.  0 <= threshold <= 1.
   The tree comes back as the neighbour lists mpf_polytomy_parsimony and mpf_polytomy_branch_lengths take: *n_inner inner nodes
   (1 .. n_taxa - 2), first[*n_inner + 1] (room for n_taxa - 1), nbr[first[*n_inner]] (room for 3 n_taxa - 6).  Tips are 1 .. n_taxa,
   inner nodes are numbered n_taxa + 1 .. in pre-order from tip 1, each lists its parent first, then its children by their smallest
   tip.  support_of_inner[i] (room for n_taxa - 2, may be NULL): the count of the split above inner node i, -1 for the first. */
int mpf_consensus_tree(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, double threshold, int32_t *n_inner,
                       int32_t *first, int32_t *nbr, int64_t *support_of_inner, int64_t *total_weight);
/* The same three results for the attached UFBoot tracker, trees and weights taken as IQTree::summarizeBootstrap takes them.  rule:
     MPF_SUMMARY_DEFAULT  tree_weights[boot_trees[b]]++                                          (iqtree.cpp:4036-4038)
     MPF_SUMMARY_MULHITS  -mulhits: += B / |boot_trees_parsimony[b]| for each tree of sample b   (summarizeBootstrapParsimonyWeight, :4097-4115)
     MPF_SUMMARY_TOPBOOT  -mulhits -topboot: +1 per tree on a sample's list                      (summarizeBootstrapParsimonyTop, :4117-4130)
     MPF_SUMMARY_AUTO     the one the tracker's own options select, as the reference does        (:4021-4027)
   Every field of *s that is a buffer may be NULL with its cap 0: that result is then not made (sizes as in the three calls above).
   MPF_E_STATE without a tracker, before any sample points to a tree, or for a rule whose lists the tracker does not keep. */
enum { MPF_SUMMARY_AUTO = -1, MPF_SUMMARY_DEFAULT = 0, MPF_SUMMARY_MULHITS = 1, MPF_SUMMARY_TOPBOOT = 2 };
typedef struct mpf_bb_summary {
  /* in */
  int32_t split_cap;            uint32_t *bits; int64_t *count;                      /* as mpf_split_counts */
  const int32_t *target_back;   int32_t branch_cap; int32_t *node1, *node2; int64_t *support;   /* as mpf_split_support; NULL target: skipped */
  double threshold;             int32_t *first, *nbr; int64_t *support_of_inner;     /* as mpf_consensus_tree; NULL first or nbr: skipped */
  /* out */
  int32_t n_trees;              /* trees of the tracker with a weight > 0 */
  int32_t n_distinct, n_branches, n_inner;
  int64_t total_weight;
} mpf_bb_summary;
int mpf_ufboot_summarize(mpf_engine *e, int32_t rule, mpf_bb_summary *s);
/* ... and the weighted tree set itself: tree_index[cap], weights[cap], backs[cap][3 (2 n_taxa - 1)] (each may be NULL), *n always the
   full number of trees */
int mpf_ufboot_summary_trees(mpf_engine *e, int32_t rule, int32_t cap, int64_t *tree_index, int32_t *weights, int32_t *backs, int32_t *n);
/* Robinson-Foulds distances between trees: -rf_all, -rf <treefile2> and -rf_adj of the reference (MTreeSet::computeRFDist,
   mtreeset.cpp:484-546 for one set, :549-660 for two sets; printed by pda.cpp:1399-1539; the reference's own check of
   -distinct_iter_top_boot calls it too, iqtree.cpp:2781-2793).  The distance of two trees is the number of non-trivial splits that are
   in one of them and not in the other: for two complete bifurcating trees on the engine's taxa 2 (n_taxa - 3) - 2 shared.  No split
   weights and no weight threshold (the reference's default of -1000 lets every split through).

   Trees as in mpf_split_counts: backs[n_trees][3 (2 n_taxa - 1)], each checked as mpf_set_tree checks it and for being ONE tree over
   all tips (MPF_E_INVALID, the message names the tree; in the second set "second set, tree k").  mode and the layout of rf, which
   is the reference's:
     MPF_RF_ALL_PAIRS  rf[i * n_trees + j], symmetric, diagonal 0                                   (mtreeset.cpp:537, pda.cpp:1506-1507)
     MPF_RF_ADJACENT   rf[i] = d(tree i, tree i + 1), n_trees - 1 entries                           (:535)
     MPF_RF_TWO_SETS   rf[i * n_trees2 + j] = d(tree i of backs, tree j of backs2)                  (:629-630)
   n_trees2 / backs2 are 0 / NULL in the other two modes.  cap: the room in rf, in entries.  MPF_E_INVALID: n_trees < 1, an unknown
   mode, MPF_RF_TWO_SETS with n_trees2 < 1 or NULL backs2, backs2 given in another mode, cap smaller than the number of entries
   the mode writes.  All pairs of one tree: the single 0; adjacent pairs of one tree: nothing.  With n_taxa = 3 every distance is 0.
   MPF_E_UNSUPPORTED above 2047 taxa and above 2^27 clusters, (n_trees + n_trees2) (n_taxa - 3), as in the split summary, and when
   the result would have more than 2^31 - 1 entries.  Either engine (Fitch or weighted).  No current tree is needed, none is changed,
   an attached tracker books nothing, the tie stream does not move.

   One split pass runs over all trees of the call (k_split_keys, k_split_insert, k_split_count; the second set behind the first),
   every tree with weight 1.  The table slots that at least two trees hold become the columns of a trees x columns bit matrix
   (k_rf_columns, k_rf_rows), shared(i, j) is the popcount of row i AND row j (k_rf_shared, a tiled integer matrix product on
   v_and_b32 / v_bcnt_u32_b32; k_rf_pairs for the adjacent pairs) and k_rf_finish makes the distances.  Exact: a true key collision
   goes through the overflow list, whose clusters the host groups by whole-set comparison and gives columns of their own.  Memory is
   bounded: the matrix is built and multiplied in chunks of columns, padded rows x words per chunk within 256 MiB, so the call never
   refuses for too many distinct splits.  Multifurcating trees (a consensus as neighbour lists, user trees with polytomies) go
   through mpf_rf_distances_set below.
   Options: read-only, each about the last call, "rf_columns" (columns of the matrix: the splits that at least two trees hold),
   "rf_chunks", "rf_launches" (kernel launches, the split pass included) and, under "timing", "rf_rows_ns" / "rf_shared_ns" (HIP-event
   time of k_rf_rows + k_rf_patch and of k_rf_shared or k_rf_pairs, summed over the chunks; the memset of the chunk's matrix is in neither).  Test option "rf_chunk_columns" (default 0: sized by the memory budget; k > 0: chunks
   of k columns, rounded up to a multiple of 32).  "split_key_bits" and "split_overflow" apply to this call as to the summary. */
enum { MPF_RF_ALL_PAIRS = 0, MPF_RF_ADJACENT = 1, MPF_RF_TWO_SETS = 2 };
int mpf_rf_distances(mpf_engine *e, int32_t mode, int32_t n_trees, const int32_t *backs /* [n_trees][3 (2 n_taxa - 1)] */,
                     int32_t n_trees2, const int32_t *backs2 /* MPF_RF_TWO_SETS only, else 0 / NULL */, int64_t cap, int32_t *rf);
/* The four split products on sets that mix record-format trees and trees given as neighbour lists: what back[] cannot hold -- the
   consensus tree mpf_consensus_tree returns, user trees with polytomies (the reference takes them through MTree::convertSplits,
   which has no degree limit) -- beside the trees of a run.  A list tree is handed over as the mpf_polytomy_* calls take it: tips
   are nodes 1 .. n_taxa, inner node i is node n_taxa + 1 + i, with the same conditions (MPF_E_INVALID): 1 <= n_inner <= n_taxa - 2,
   every inner degree >= 3, symmetric adjacency, every tip exactly once, n_taxa + n_inner - 1 edges, connected.  It has exactly
   n_inner - 1 non-trivial splits: one for every inner node other than the node next to tip 1, the tips on that node's side away
   from tip 1.  A star (n_inner = 1) has none; a list tree with n_inner = n_taxa - 2 is fully resolved and gives in every call, bit
   for bit, what its record form gives.  Everything is integer and exact, true key collisions included ("split_key_bits").

   The index of a tree within a set counts the records first, then the lists; weights[] runs in that order.  The contracts are those
   of mpf_split_counts, mpf_split_support, mpf_consensus_tree and mpf_rf_distances: the contract order, the sizing protocol, weights
   >= 0 with NULL = all 1 and weight-0 trees contributing nothing, the modes and result layouts, the MPF_E_INVALID /
   MPF_E_UNSUPPORTED conditions.  A message names a record-format tree "tree k" and a list tree "list tree k", k counted from 0
   within the records and within the lists ("second set, list tree k" in the second set of mpf_rf_distances_set).  The limits:
   2047 taxa, and 2^27 cluster slots, (trees of the call) (n_taxa - 3): a list tree takes as many slots as a record-format one.
   The differences:
     mpf_split_support_set  the target is a list tree; the branches come back in the walk order of mpf_polytomy_branch_substitutions
                            from root_taxon = 1, so that the two calls' arrays line up; *n = n_taxa + n_inner - 1; -1 on a leaf
                            branch and on the branch at tip 1, whose inner end holds every other tip and is no split.
     mpf_rf_distances_set   RF(i, j) = c_i + c_j - 2 shared(i, j), c_t the number of non-trivial splits of tree t (the reference's
                            size(A) + size(B) - 2 common, mtreeset.cpp:484-660).  s2 is NULL unless mode is MPF_RF_TWO_SETS.
   The device: k_split_keys walks the record-format trees and k_split_keys_lists the list trees (one workgroup per tree, the lists
   in LDS, children in list order -- a resolved list tree has its record form's splits, not its DFS order --) into the same arrays; then insert, count and compact run once over all of them.  A call without
   list trees launches what the record calls launch.  No current tree is needed and none is changed, an attached tracker books
   nothing, the tie stream does not move; either engine (Fitch or weighted) serves the calls.
   Not served: unequal taxon sets (RF_TWO_TREE_SETS_EXTENDED), split-weight thresholds, incompatible-split counts, .rfinfo / .rftree,
   more than 2047 taxa. */
typedef struct mpf_tree_set {
  int32_t n_records; const int32_t *backs;    /* [n_records][3 (2 n_taxa - 1)] as mpf_split_counts takes them; 0 / NULL = none */
  int32_t n_lists;   const int32_t *n_inner;  /* [n_lists]; 0 / NULL = none */
  const int32_t *first;   /* the trees' first[] one behind the other: n_inner[t] + 1 entries each, each starting at 0 */
  const int32_t *nbr;     /* the trees' nbr[] one behind the other: first[n_inner[t]] entries each */
} mpf_tree_set;
int mpf_split_counts_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, int32_t cap,
                         uint32_t *bits /* [cap][ceil(n_taxa / 32)] */, int64_t *count /* [cap] */, int32_t *n_distinct, int64_t *total_weight);
int mpf_split_support_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, int32_t target_n_inner, const int32_t *target_first,
                          const int32_t *target_nbr, int32_t cap, int32_t *node1, int32_t *node2, int64_t *support, int32_t *n,
                          int64_t *total_weight);
int mpf_consensus_tree_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, double threshold, int32_t *n_inner, int32_t *first,
                           int32_t *nbr, int64_t *support_of_inner, int64_t *total_weight);
int mpf_rf_distances_set(mpf_engine *e, int32_t mode, const mpf_tree_set *s1, const mpf_tree_set *s2 /* MPF_RF_TWO_SETS only, else NULL */,
                         int64_t cap, int32_t *rf);
/* The same climb under -bb (save_all_trees == 2), with the UFBoot tracker of mpf_ufboot_attach booking every tree the climb looks
   at through IQTree::saveCurrentTree, in the reference's order: at the start of every step that is not a rollback step the current
   tree with curScore (iqtree.cpp:2181-2183), then for every branch the step evaluates, in evaluation order, the tree after move 0
   and the tree after move 1 with the length optimizeOneBranch returned (getBestNNIForBran, phylotree.cpp:3907-3939) -- all of
   them, not only the positive ones; nothing in a rollback step.  pllComputePatternParsimony is skipped on this path
   (iqtree.cpp:3363), _pattern_pars is the booked tree's own row (phylotree.cpp:956-957, :986-987): on a re-weighted (ratchet)
   climb the length the cut-off test sees and treels_logl records is the booked tree's OWN length on the attach-time weights
   (iqtree.cpp:3283-3294), and a tree that fails the cut-off closes no gate.  The tracker's tie draws come from the shared stream
   (mpf_seed_ties / mpf_set_tie_state / mpf_set_rand) in this booking order; the climb itself draws nothing.  Lengths are the
   engine's: patterns it drops (keep_all_sites 0) count 0.
   Served: the default update rule, -mulhits, mpf_ufboot_set_cutoff, -cutoff_from_btrees, ratchet booking; under
   mpf_ufboot_set_ratchet_booking(e, 0) a re-weighted climb runs without booking (the plain climb).  NOT served, MPF_E_UNSUPPORTED:
   the weighted engine (but see below); -storetrees, -mulhits -topboot, -distinct_iter_top_boot and a sample-sharded tracker unless
   the option "nni_tracked_rules" (mpf_set_option, default 0) is 1: then the booked trees go through the rule in force exactly as an
   SPR climb's do (mpf_ufboot_set_iteration gives -distinct_iter_top_boot its iteration), and on a tracker attached with
   mpf_ufboot_attach_sharded every rank makes the same call: ONE exchange per scoring step (tags 0x40000000 + step, a closing one
   0xFFFFFFFE per climb) carries the step's events and the current tree's scores under the rank's samples.
   Arguments, results, swap log (mpf_get_nni_moves) and counters as mpf_optimize_nni; MPF_E_STATE without a tracker or a tree.
   Read-only option "nni_booked": trees NNI climbs have handed to saveCurrentTree since the attach.

   The weighted engine (-cost m -nni_pars -bb, and -hclimb1_nni under -cost -bb).  Option "nni_weighted_tracked" (mpf_set_option,
   default 0; accepted and without effect on a Fitch engine): with 0 this entry refuses a weighted engine as above, with 1 -- and
   "nni_weighted" 1 -- it is served there.  The climb is the weighted one of mpf_optimize_nni (ParsTree scoring, NO rollback,
   iqtree.cpp:2258: a kept-worse step is followed by an ordinary scoring step, which books the current tree under the longer
   curScore); the trees booked and their order are those above (iqtree.cpp:2181-2183, phylotree.cpp:3907-3939).  _pattern_pars is
   again the booked tree's own row, since pllComputePatternParsimony is skipped (iqtree.cpp:3363):
     - a candidate's: the per-pattern minima min_i( Y[i] + m(X)[i] ) ParsTree::computeParsimonyBranch has just written
       (parstree.cpp:460-461, :482-529), the tree rooted at the scored branch with node2's side the parent;
     - the current tree's: the row ParsTree::computeParsimony() wrote at the edge of the leaf root_taxon (parstree.cpp:101-116,
       reached through optimizeAllBranches, phylotree.cpp:3255-3259).  At the FIRST step the reference's _pattern_pars is whatever
       the host's last computeParsimonyBranch left; the engine books the root-leaf row there too.  A host whose last evaluation
       before the call was at another edge differs for that one call, and only under a matrix that is not symmetric.
   On a ratchet climb (iqtree.cpp:3283-3294) the length the cut-off test sees and treels_logl records is that row times the
   attach-time weights; a tree that fails the cut-off closes no gate.  Served and refused tracker forms as above; mpf_optimize_nni
   with a tracker attached and mpf_nni_pattern_terms stay MPF_E_UNSUPPORTED.  Whatever mpf_ufboot_attach demands of a weighted
   engine is the only condition on the costs. */
int mpf_ufboot_optimize_nni(mpf_engine *e, int32_t root_taxon, int32_t speednni, int32_t max_steps, uint32_t *score, int32_t *nni_count,
                            int32_t *nni_steps);

/* accepted moves of the last mpf_optimize_spr / mpf_make_parsimony_tree: (remove rec, insert rec, length) */
int mpf_get_moves(const mpf_engine *e, int32_t cap, int32_t *remove_rec, int32_t *insert_rec, uint32_t *score,
                  int32_t *n_moves);

/* Lower-bound helpers of the reference's parsimony path (host arithmetic, no device needed).  The reference uses them
   to leave its CPU loops early (REPS skip iqtree.cpp:3435-3445, Sankoff evaluate sprparsimony.cpp:946-955); the engine
   computes exact full sums, so nothing in this library depends on them.
     mpf_min_pars_score_patterns : pllCalcMinParsScorePattern (sprparsimony.cpp:2513-2547) for every pattern
     mpf_mst_scores              : ParsTree::findMstScore (parstree.cpp:606-680) for every pattern
     mpf_segment_patterns        : IQTree::doSegmenting (iqtree.cpp:3793-3820)
     mpf_remain_bounds           : IQTree::pllComputeRellRemainBound (iqtree.cpp:3842-3853) / pllRemainderLowerBounds
                                   (sprparsimony.cpp:2813-2819) for one weight vector */
/* ParsTree::loadCostMatrixFile (parstree.cpp:31-95): `file_or_keyword` = "fitch" | "e" (unit costs for
   n_states_alignment states) or the path of a text file "<nstates>  nstates x nstates entries"; the matrix is then closed
   under the triangle inequality by the reference's own k-i-j loop (:74-80; *changed = 1 if that altered an entry).
   cost has room for cap_states x cap_states entries.  The result is what mpf_engine_create_sankoff takes (the reference
   copies it into pllCostMatrix, iqtree.cpp:601-615). */
int mpf_cost_matrix_load(const char *file_or_keyword, int32_t n_states_alignment, int32_t cap_states, uint32_t *cost /* [cap*cap] */,
                         int32_t *n_states, int32_t *changed);
int mpf_cost_matrix_triangle_fix(int32_t n_states, uint32_t *cost /* [S*S], in place */, int32_t *changed);
int mpf_min_pars_score_patterns(int32_t datatype, int32_t n_taxa, int32_t n_patterns, const uint8_t *codes /* [n][P] PLL tip codes */,
                                int32_t *min_score /* [P] */);
int mpf_mst_scores(int32_t n_states, const uint32_t *cost /* [S*S] */, int32_t n_taxa, int32_t n_patterns,
                   const int8_t *states /* [n][P] IQ-TREE state codes */, uint32_t *mst /* [P] */);
int mpf_segment_patterns(int32_t n_patterns, int32_t n_informative, int32_t vcsize, const int32_t *ras_pars_score,
                         const int32_t *frequency, int32_t *segment_upper /* [P] */, int32_t *n_segments);
int mpf_remain_bounds(int32_t n_units, int32_t n_segments, const int32_t *segment_upper, const int32_t *min_unit_pars,
                      const uint16_t *weight, int32_t *remain /* [n_segments - 1] */);

/* Online UFBoot-MP bookkeeping -- what IQTree::saveCurrentTree (iqtree.cpp:3271-3785, default options) does when
   testInsertParsimony calls it after EVERY insertion test of pllOptimizeSprParsimony (sprparsimony.cpp:2163-2166,
   perSiteScores = gbo_replicates > 0, :3245).  With a tracker attached, mpf_optimize_spr additionally
     - applies the logl_cutoff filter (:3343) and appends the candidate's score to treels_logl (:3345-3348),
     - computes its REPS against all n_samples weight vectors on the device (ufboot.hip),
     - applies the per-sample update rule (:3684-3731) in the reference's order, drawing its tie-breaks from the same
       random stream as the SPR tie-breaks (mpf_seed_ties / mpf_set_rand_callback).
   samples = boot_samples_pars (iqtree.cpp:213-313), [n_samples][n_patterns] uint16.  epsilon = params->ufboot_epsilon
   (0.5, tools.cpp:725); any value in (0, 1) is equivalent for integer scores, others are MPF_E_UNSUPPORTED.
   Both engines: on the weighted (Sankoff, -cost) engine the per-pattern lengths are those pllComputeSankoffPatternParsimony
   reads (sprparsimony.cpp:3341-3355) -- with a matrix that is not symmetric the current tree is booked at every prune node's
   visit with the length and the per-pattern lengths it has at that node's edge (:2285) --, sample sharding (below) included.  Climbs under other weights than the attach-time
   ones (ratchet iterations) are booked as the reference books them (iqtree.cpp:3283-3295) unless
   mpf_ufboot_set_ratchet_booking(e, 0) (-no_hclimb1_bb, :3280); weights that take an attach-time pattern out of the
   alignment altogether rest the tracker until the attach-time weights are back. */
int mpf_ufboot_attach(mpf_engine *e, int32_t n_samples, const uint16_t *samples, double epsilon);
/* Batched bootstrap refinement -- IQTree::optimizeBootTrees' default branch (iqtree.cpp:2797-2862: per sample modifyPatternFreq
   :2520, the parsimony structures rebuilt, ONE pllOptimizeSprParsimony from the sample's tree :2837) for every attached sample
   whose tree is the engine's CURRENT tree, at once.  Fitch state sets do not depend on pattern weights, only the counts do: the
   first sweep of all those climbs is one masked scan + one mask x weight product on the matrix cores; every sample's sweep
   (testInsertParsimony's tie rule sprparsimony.cpp:2168-2176, the sweep's accept rule :3306-3311) is then replayed from the few
   (insertion test, sample) pairs that reach the sample's running best, with the sample's own tie stream (seeded like
   mpf_seed_ties(e, MPF_TIE_RANDOM, tie_seeds[b]); NULL: seed b).
     scores[b]  = length of the current tree under sample b's weights (what the climb starts from)
     stable[b]  = 1: that sweep accepts no move -- mpf_set_weights(sample b) + mpf_optimize_spr from this tree would return
                  scores[b] and leave the tree as it is; 0: it accepts one (first_move_visit[b] = 1-based position in the sweep's
                  visiting order, mpf_get_node_order) -- the caller runs that sample's climb alone
   All three arrays have n_samples entries of the attach call (a sample-sharded tracker fills the entries of its own samples);
   any may be NULL.  Needs the attach-time weights in force, the random tie rule (any maxtrav, both engines).  The
   tracker's saveCurrentTree bookkeeping is not touched.  (ABI 5) */
int mpf_ufboot_refine_sweep(mpf_engine *e, int32_t maxtrav, const int32_t *tie_seeds, uint32_t *scores, uint8_t *stable,
                            int32_t *first_move_visit);
/* Multi-GPU online phase: the samples are sharded over the GPUs, the search chain is not.  Every rank runs the same
   mpf_optimize_spr calls (same tree, same tie seed) on its own engine, which holds only n_local of the n_samples weight
   vectors (sample_ids[c] = run-wide index of local vector c) and so does 1/n_gpus of the REPS work.  After each scan batch
   the engine hands its (candidate, sample, score) events to `exchange`, which must return the events of ALL ranks (any
   order; an all-gather -- RCCL on the GPU box); every rank then replays the same merged list, so tie draws, accepted
   moves and all bookkeeping arrays are identical on every rank and identical to the unsharded run. */
typedef struct { uint32_t idx, sample, score; } mpf_ufb_event;
/* tag: position of the call in the run (batch counter; 0xFFFFFFFF closes a climb).  The ranks advance in lock step, so
   an exchange that sees different tags must fail (return non-zero): the engine then stops with MPF_E_STATE instead of
   waiting forever.  Returns 0 on success; *all stays valid until the next call. */
typedef int (*mpf_ufb_exchange_fn)(void *arg, uint32_t tag, const mpf_ufb_event *local, uint32_t n_local,
                                   const mpf_ufb_event **all, uint32_t *n_all);
int mpf_ufboot_attach_sharded(mpf_engine *e, int32_t n_samples, int32_t n_local, const int32_t *sample_ids,
                              const uint16_t *samples_local /* [n_local][n_patterns] */, double epsilon,
                              mpf_ufb_exchange_fn exchange, void *arg);
int mpf_ufboot_detach(mpf_engine *e);
/* The exchanges of the multi-GPU path, native (ABI 7; mpboot_amd/host/rccl_exchange.cpp): RCCL over xGMI from inside the library,
   librccl opened at run time.  One communicator per process / GPU: rank 0 makes the id (mpf_rccl_unique_id, 128 bytes) and hands
   it to the others by whatever the host has; everybody calls mpf_rccl_create.  mpf_rccl_exchange IS an mpf_ufb_exchange_fn --
   pass it with the communicator as `arg` to mpf_ufboot_attach_sharded: one all-gather of fixed-size event blocks per scan
   batch on a stream of its own, a second one only when some rank has more than 4096 events.  mpf_rccl_allreduce_min: the
   "single all-reduce of best scores per round" of independent units (start trees, replicates).  The reference has nothing
   distributed: these replace what a multi-GPU mpboot host would otherwise write with MPI. */
typedef struct mpf_rccl mpf_rccl;
int mpf_rccl_available(void);
int mpf_rccl_unique_id(uint8_t *out /* [128] */);
int mpf_rccl_create(mpf_rccl **out, const uint8_t *id /* [128] */, int32_t rank, int32_t world, int32_t device);
void mpf_rccl_destroy(mpf_rccl *c);
int mpf_rccl_exchange(void *arg /* mpf_rccl* */, uint32_t tag, const mpf_ufb_event *local, uint32_t n_local,
                      const mpf_ufb_event **all, uint32_t *n_all);
int mpf_rccl_allreduce_min(mpf_rccl *c, uint32_t *vals, int32_t n);
int mpf_rccl_counters(const mpf_rccl *c, uint64_t *exchanges, uint64_t *overflows);
int mpf_ufboot_set_cutoff(mpf_engine *e, double logl_cutoff);            /* IQTree::logl_cutoff; 0 = none */
/* Climbs under other pattern weights than the attach-time ones (ratchet iterations: mpf_set_weights between attach and
   mpf_optimize_spr) are booked as the reference's default books them (iqtree.cpp:3283-3295): the length a candidate is
   filtered and recorded with is the ORIGINAL-alignment length of the tree booked last (of the climb's start tree for
   the first candidate) -- saveCurrentTree recomputes cur_logl from _pattern_pars before refreshing that array --, the
   per-sample REPS are the candidate's own.  on = 0 is params->no_hclimb1_bb (iqtree.cpp:3280): such climbs run without
   saveCurrentTree.  Takes effect at the next mpf_set_weights.  Weights that give an attach-time pattern weight 0 suspend
   the bookkeeping in either case (mpboot's ratchet only adds copies of sites). */
int mpf_ufboot_set_ratchet_booking(mpf_engine *e, int32_t on);
/* the main loop's per-iteration cut-off update, "top percent %" rule (iqtree.cpp:1662-1676, cutoff_percent = 10) */
/* params->multiple_hits (-mulhits): the update rule of iqtree.cpp:3498-3540 replaces the default one (:3684-3731) -- every
   tree whose REPS reaches a sample's best joins that sample's set (boot_trees_parsimony), a better one clears the set first;
   trees of one topology share the index of the first of them that hit (the reference's treels string map, :3500-3514); no
   random draws, boot_counts / boot_trees stay untouched.  Call right after the attach, before any tree is booked.
   (-topboot and -distinct_iter_top_boot: below.) */
int mpf_ufboot_set_mulhits(mpf_engine *e, int32_t on);
/* params->store_candidate_trees (-storetrees; off by default, tools.cpp:736): iqtree.cpp:3302-3346 -- every tree that reaches
   saveCurrentTree is looked up by topology (printTree(WT_TAXON_ID | WT_SORT_TAXA) as the key) BEFORE the cut-off test.  One
   met before counts as a duplicate (duplication_counter, mpf_ufboot_get_duplicates) and is skipped, unless its length
   improved on the recorded treels_logl entry (this happens on ratchet climbs, whose lengths come from _pattern_pars as it
   stands): then the entry is updated and the tree goes through the update rule under its OLD index, without the cut-off
   test.  Combines with every update rule.  Costs one canonical form per insertion test on the host (the reference prints,
   re-reads and prints the tree per test).  Call right after the attach, before any tree is booked. */
int mpf_ufboot_set_store_trees(mpf_engine *e, int32_t on);
int mpf_ufboot_get_duplicates(const mpf_engine *e, uint64_t *n);
/* params->store_top_boot_trees (-topboot N, together with -mulhits): the rule of iqtree.cpp:3542-3585 -- per sample the N best
   NEW trees (a tree whose topology was booked before is never added), best first, with boot_threshold behaving as in the
   reference (-INT_MAX until the first replacement in a full list).  After mpf_ufboot_set_mulhits(e, 1), before any tree is
   booked; n_top = 0 switches back to plain -mulhits.  mpf_ufboot_get_sample_top: boot_trees_parsimony_top[sample] as
   (tree index, rell) pairs, *n = its length, *threshold = boot_threshold[sample]. */
int mpf_ufboot_set_topboot(mpf_engine *e, int32_t n_top);
int mpf_ufboot_get_sample_top(const mpf_engine *e, int32_t sample, int64_t *trees, int32_t *rell, int32_t cap, int32_t *n, int32_t *threshold);
/* params->distinct_iter_top_boot (-distinct_iter_top_boot k, without -mulhits): the rule of iqtree.cpp:3587-3680 -- per sample at
   most k trees, one representative per search iteration, accepted against boot_threshold (the list's worst score) with a
   k / boot_counts tie draw from the shared random stream; boot_trees / boot_logl / boot_counts are maintained as that rule
   maintains them (mpf_ufboot_get_state), the list is read with mpf_ufboot_get_sample_top and the iteration each entry stands
   for with mpf_ufboot_get_sample_iters.  Before any tree is booked.  mpf_ufboot_set_iteration: IQTree::curIt, before each
   mpf_optimize_spr of a new search iteration. */
int mpf_ufboot_set_distinct_iter(mpf_engine *e, int32_t k);
int mpf_ufboot_set_iteration(mpf_engine *e, int32_t cur_it);
int mpf_ufboot_get_sample_iters(const mpf_engine *e, int32_t sample, int32_t *iters, int32_t cap, int32_t *n);
/* boot_trees_parsimony[sample] in increasing order: *n = its size, the first min(*n, cap) entries written to out (may be NULL) */
int mpf_ufboot_get_sample_trees(const mpf_engine *e, int32_t sample, int64_t *out, int32_t cap, int32_t *n);
int mpf_ufboot_next_cutoff(const mpf_engine *e, int32_t percent, double *logl_cutoff);
/* -cutoff_from_btrees (params->cutoff_from_btrees, tools.cpp:2442; ABI 7): boot_tree_orig_logl[b] (iqtree.h:766) = the logl under which
   sample b's tree was booked -- set at every acceptance of the default and the -distinct_iter_top_boot rule (iqtree.cpp:3716-3718,
   :3617-3619), only ever raised from its initial 0 by -mulhits (:3523-3527: with negative logls, never) --, and
   mpf_ufboot_next_cutoff returns their minimum (:1657-1660) instead of the percentile of the saved trees.  Any time after the
   attach; the array is kept whether or not the switch is on. */
int mpf_ufboot_set_cutoff_from_btrees(mpf_engine *e, int32_t on);
int mpf_ufboot_get_orig_logl(const mpf_engine *e, int32_t *out /* [n_samples] */);
int mpf_ufboot_num_trees(const mpf_engine *e, int64_t *n_trees);         /* treels_logl.size() */
int mpf_ufboot_tree_logl(const mpf_engine *e, double *out /* [n_trees] */);
/* boot_logl / boot_counts / boot_trees (any may be NULL) */
int mpf_ufboot_get_state(const mpf_engine *e, double *boot_logl, int32_t *boot_counts, int32_t *boot_trees);
/* topology of a tree some sample currently points to (boot_trees[b]), as back[] */
int mpf_ufboot_get_tree(const mpf_engine *e, int64_t tree_index, int32_t *back);
/* Iteration-parallel -bb (the reference's parallel form distributes the ITERATIONS of doTreeSearch over processes that meet from time
   to time, README.md:71-78): books another chain of the same run keeps.  Update k offers sample[k] the tree tree_of[k] (one of
   n_trees topologies, backs[n_trees][3 (2n - 1)], lengths[] = their lengths on the original alignment) at REPS length score[k]; a
   sample takes it when it is STRICTLY shorter than what it holds (the strict branch of saveCurrentTree's rule, iqtree.cpp:3686,
   :3710-3720; equal lengths keep the holder, no draw).  Default update rule, unsharded tracker, between two climbs. */
int mpf_ufboot_adopt(mpf_engine *e, int32_t n_updates, const int32_t *sample, const uint32_t *score, const int32_t *tree_of, int32_t n_trees,
                     const int32_t *backs, const uint32_t *lengths, int32_t *n_taken);
int mpf_ufboot_get_counters(const mpf_engine *e, uint64_t *tie_draws, uint64_t *events, uint64_t *reps_rows, double *reps_kernel_ms);

/* REPS -- resampling parsimony scores of candidate trees under B bootstrap weight vectors, the inner loop of
   IQTree::saveCurrentTree (iqtree.cpp:3411-3449): rell[m][b] = -sum_ptn pattern_pars[m][ptn] * boot[b][ptn].
   boot_samples_pars as IQTree::setParams builds them (iqtree.cpp:213-313), uploaded once; pattern_pars rows as
   mpf_pattern_scores / mpf_compute_parsimony return them.  Exact 32-bit sums. */
typedef struct mpf_reps mpf_reps;
int mpf_reps_create(mpf_reps **out, int32_t device, int32_t n_samples, int32_t n_patterns, const uint16_t *boot /* [B][P] */);
int mpf_reps_scores(mpf_reps *r, int32_t n_trees, const uint16_t *pattern_pars /* [M][P] */, int32_t *rell /* [M][B] */);
void mpf_reps_destroy(mpf_reps *r);

/* ---- The steps of IQTree::doTreeSearch BETWEEN two climbs (iqtree.cpp:1631-1965), device-free, on `back` records: for hosts
   without IQ-TREE's tree classes (bench.py, tests, a C++ driver) that want to run the flow the reference runs -- candidate tree ->
   floor(0.5 (n - 3)) random NNIs, or every second iteration a re-weighted alignment -> climb.  All draws come from the host's
   random_double() stream, handed over by state like the climb's own (mpf_set_tie_state / mpf_get_tie_state).  mpboot keeps its own
   code for these steps; the engine never calls them.  (mpboot_amd/host/iqflow.cpp; second witness oracle/iqflow_slow.py.)

   mpf_iq_random_nnis      IQTree::doRandomNNIs(numNNI) (iqtree.cpp:1083-1106) + PhyloTree::doOneRandomNNI (phylotree.cpp:3665-3711):
                           per NNI one random_int(n - 3) for the branch and two random_int(1) (always 0: the first neighbour at each
                           end); a branch that touches a node already used re-lists the branches and takes the same index (:1096-1103).
                           The listing order and which neighbour is "first" are this library's (ring order from tip 1).
   mpf_iq_perturb_weights  Alignment::createPerturbAlignment (alignment.cpp:1915-1969; -ratchet_percent 50, -ratchet_wgt 1,
                           tools.cpp:778-780): n_informative_sites * percent / 100 distinct sites of informative patterns, `add` more
                           copies of each one's pattern.  out[n_patterns].
   mpf_iq_topology_key     128-bit digest of the canonical unrooted topology: the key of CandidateSet::topologies (candidateset.cpp:110-150). */
int mpf_iq_random_nnis(int32_t n_taxa, int32_t *back, int32_t num_nni, uint64_t *tie_state, int32_t *n_relists);
int mpf_iq_perturb_weights(int32_t n_patterns, const int32_t *weights, const uint8_t *informative, int32_t percent, int32_t add,
                           uint64_t *tie_state, int32_t *out);
int mpf_iq_topology_key(int32_t n_taxa, const int32_t *back, uint64_t key[2]);

int mpf_get_stats(const mpf_engine *e, mpf_stats *out);
int mpf_reset_stats(mpf_engine *e);
/* tuning knobs (none of them changes a result):
     "scan_batch"      prune nodes speculated per launch at the start of a climb (then adaptive)
     "words_per_lane"  1|2|4 32-site words per lane in the Fitch kernels
     "reduce"          0 = DPP wave reduction, 1 = ds_bpermute
     "xcd_map"         1 = XCD-aware workgroup -> tile map of the scan kernel
     "scan_mode"       1 = device-walked SPR scan (radius <= 8), 0 = host-planned scan programs
     "scan_prog"       device-walked mode, DNA, radius <= 6: 1 = batches of more than "prog_min_descs" scan parts are first
                       turned into DFS programs on the device (k_walk_plan) and run with the children's vectors requested
                       one expansion ahead (k_scan_prog); 2 = every batch; 0 = never (k_scan_walk walks the tree itself)
     "prog_min_descs"  see "scan_prog" (default 256)
     "views_mode"      2 = chained refresh (stale paths run in registers, one launch; Fitch mode), 1 = all dependency
                       levels of a refresh in one launch, 0 = one launch per level
     "views_pipe"      level kernel, one word per lane: 1 (default) = a tile of "views_tile" words per workgroup, 64 / tile ops
                       per wave instruction, the next round's operands requested before this round's stores, tiles dealt
                       to the XCDs in contiguous runs; 0 = 32-word tiles, half a wave per op
     "views_tile"      32 | 16 | 8 | 4, or 0 (default) = the smallest of them that gives at most 256 workgroups
     "chain_max_ops"   refreshes of up to this many vectors use the chained kernel (default 512; larger ones are wide
                       rather than deep and take the level kernel)
     "split_below"     batches of at most this many prune nodes are cut into four scan parts each
     "split_cands"     larger batches: a prune node's P or Q neighbourhood is cut into four parts only when it holds more
                       insertion tests than this (default 64)
     "sankoff_short"   1 = two 16-bit costs per lane in the weighted kernels when no intermediate can overflow
                       (the reference's default arithmetic), 0 = always 32-bit (its -short_off)
     "plan_cache"      1 (default) = what the host prepares per topology -- the whole-tree refresh schedule, a sweep's scan
                       descriptors and its device program -- is kept while the topology stands (the same tree handed over again,
                       re-weighted, re-evaluated); 0 = everything is planned again every time
     "host_poll"       1 (default) = small batches: the host waits for the flag word the scan's last workgroup raises behind the
                       results it writes to pinned memory, instead of a stream synchronisation
     "check_counts"    1 = compare the kernel's candidate counts with the host's, and check the view bookkeeping
     "force_big"       1 = 64-bit addressing in the scan kernel even below 2 GiB of vectors (set before the first tree); on a
                       weighted engine: 64-bit pointers per row in the scan (k_snk_scan / k_snk_scan_deep) and in the per-branch
                       kernels, what a half of the store of 4 GiB and more takes by itself -- read-only "snk_scan_wide" /
                       "snk_scan_deep" tell what the launcher dispatched for the last weighted scan batch (rows through 64-bit
                       pointers / k_snk_scan_deep), "snk_deep_batches" / "snk_deep_launches" count the deep batches since
                       creation and the launches they were cut into (option "deep_scratch_kwords")
     "timing"          1 = HIP events around the scan kernels (mpf_stats scan_kernel_ms_total), 2 = around the refresh
                       kernels too (view_kernel_ms_total); an event pair costs about 10 us on the stream */
int mpf_set_option(mpf_engine *e, const char *key, int64_t value);
/* diagnostic (option "scan_trace" = 1): timeline of the last planned-program scan launch, four 64-bit words per workgroup:
   begin, end (100 MHz counter), XCC_ID << 32 | HW_ID, scan << 32 | tile << 16 | insertion tests.  *n_words is always set;
   out is filled when cap >= *n_words. */
int mpf_get_scan_trace(mpf_engine *e, uint64_t *out, uint64_t cap, uint64_t *n_words);
/* current value of an option of mpf_set_option; read-only: "kernel_states" = state rows the kernels carry (4: DNA and binary,
   20: protein and multistate data with at most 20 symbols in use, 32: multistate data beyond that or under a cost matrix) */
int mpf_get_option(const mpf_engine *e, const char *key, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* MPFITCH_H */
