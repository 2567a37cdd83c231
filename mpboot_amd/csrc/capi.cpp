// capi.cpp -- the extern "C" boundary declared in include/mpfitch.h.
#include <cstring>
#include <new>

#include "engine.hpp"
#include "place.hpp"

namespace mpf { const std::string &last_error(); }

struct mpf_engine {
  mpf::Engine eng;
};

using mpf::set_error;

#define NEED(e)                                                                                                        \
  do {                                                                                                                 \
    if (!(e)) { set_error("null engine handle"); return MPF_E_INVALID; }                                               \
    if ((e)->eng.broken()) { set_error("engine unusable: a device launch did not come back (destroy it)"); return MPF_E_STATE; } \
    (e)->eng.activate();                                                                                               \
  } while (0)

extern "C" {

const char *mpf_last_error(void) { return mpf::last_error().c_str(); }
int mpf_abi_version(void) { return MPF_ABI_VERSION; }

int mpf_engine_create(mpf_engine **out, const mpf_config *cfg, const uint8_t *codes, const int32_t *weights)
{
  if (!out || !cfg) { set_error("mpf_engine_create: null argument"); return MPF_E_INVALID; }
  *out = nullptr;
  mpf_engine *e = new (std::nothrow) mpf_engine();
  if (!e) { set_error("out of host memory"); return MPF_E_NOMEM; }
  int rc = e->eng.init(*cfg, codes, weights);
  if (rc != MPF_OK) { delete e; return rc; }
  *out = e;
  return MPF_OK;
}

int mpf_engine_create_sankoff(mpf_engine **out, const mpf_config *cfg, const uint8_t *codes, const int32_t *weights,
                              const uint32_t *cost)
{
  if (!out || !cfg || !cost) { set_error("mpf_engine_create_sankoff: null argument"); return MPF_E_INVALID; }
  *out = nullptr;
  mpf_engine *e = new (std::nothrow) mpf_engine();
  if (!e) { set_error("out of host memory"); return MPF_E_NOMEM; }
  int rc = e->eng.init(*cfg, codes, weights, cost);
  if (rc != MPF_OK) { delete e; return rc; }
  *out = e;
  return MPF_OK;
}

void mpf_engine_destroy(mpf_engine *e)
{
  if (e) e->eng.activate();
  delete e;
}

int mpf_set_weights(mpf_engine *e, const int32_t *weights)
{
  NEED(e);
  if (!weights) { set_error("null weights"); return MPF_E_INVALID; }
  return e->eng.set_weights(weights);
}

int mpf_get_geometry(const mpf_engine *e, int32_t *states, int32_t *words_per_row, int32_t *n_informative, int32_t *words_padded)
{
  NEED(e);
  if (states) *states = e->eng.S();
  if (words_per_row) *words_per_row = e->eng.Wref();
  if (n_informative) *n_informative = e->eng.n_informative();
  if (words_padded) *words_padded = e->eng.Wp();
  return MPF_OK;
}

int mpf_get_informative(const mpf_engine *e, int32_t *flags)
{
  NEED(e);
  const auto &v = e->eng.informative();
  std::memcpy(flags, v.data(), v.size() * sizeof(int32_t));
  return MPF_OK;
}

int mpf_get_tip_vector(mpf_engine *e, int32_t tip, uint32_t *out) { NEED(e); return e->eng.tip_vector(tip, out); }

int mpf_set_tree(mpf_engine *e, const int32_t *back)
{
  NEED(e);
  if (!back) { set_error("null topology"); return MPF_E_INVALID; }
  return e->eng.set_tree(back);
}

int mpf_get_tree(const mpf_engine *e, int32_t *back) { NEED(e); e->eng.get_tree(back); return MPF_OK; }
int mpf_reset_node_order(mpf_engine *e) { NEED(e); e->eng.reset_node_order(); return MPF_OK; }
int mpf_score_tree(mpf_engine *e, uint32_t *score) { NEED(e); return e->eng.score_tree(score); }

int mpf_score_trees(mpf_engine *e, int32_t n_trees, const int32_t *backs, uint32_t *scores)
{
  NEED(e);
  const size_t len = 3 * (size_t)(2 * e->eng.n() - 1);
  for (int t = 0; t < n_trees; t++) {
    int rc = e->eng.set_tree(backs + (size_t)t * len);
    if (rc) return rc;
    rc = e->eng.score_tree(scores + t);
    if (rc) return rc;
  }
  return MPF_OK;
}

int mpf_pattern_scores(mpf_engine *e, uint16_t *ptn_pars, int32_t *total) { NEED(e); return e->eng.pattern_scores(ptn_pars, total); }

int mpf_site_scores(mpf_engine *e, int32_t *site_pars, int32_t n_sites, int32_t *total)
{
  NEED(e);
  if (!site_pars || n_sites < 0) { set_error("mpf_site_scores: bad argument"); return MPF_E_INVALID; }
  return e->eng.site_scores(site_pars, n_sites, total);
}

int mpf_compute_parsimony(mpf_engine *e, const int32_t *back, uint32_t *score, uint16_t *pattern_pars)
{
  return mpf_compute_parsimony_at(e, back, 0, score, pattern_pars);
}

int mpf_compute_parsimony_at(mpf_engine *e, const int32_t *back, int32_t root_taxon, uint32_t *score, uint16_t *pattern_pars)
{
  NEED(e);
  if (back) { int rc = e->eng.set_tree(back); if (rc) return rc; }
  if (root_taxon < 0 || root_taxon > e->eng.n()) { set_error("mpf_compute_parsimony_at: root taxon out of range"); return MPF_E_INVALID; }
  // (the tree is evaluated at the edge of the leaf in start_; 0 keeps the engine's own -- tr->start = taxon 1)
  uint32_t s = 0;
  int rc = e->eng.score_tree(&s);            // (nodeRectifierPars puts start_ back on taxon 1: the guard goes behind it)
  if (rc) return rc;
  mpf::Engine::StartGuard guard(e->eng, root_taxon);
  if (root_taxon > 1) rc = e->eng.tree_length_at_start(&s);
  if (rc) return rc;
  if (score) *score = s;
  if (pattern_pars) {
    int32_t total = 0;
    rc = e->eng.pattern_scores(pattern_pars, &total);
    if (rc) return rc;
    if ((uint32_t)total != s) { set_error("per-pattern lengths do not add up to the tree length"); return MPF_E_STATE; }  // iqtree.cpp:3366-3367
  }
  return MPF_OK;
}

int mpf_encode_iqtree_states(int32_t datatype, const int8_t *states, int64_t count, uint8_t *codes)
{
  if (!states || !codes || count < 0) { set_error("mpf_encode_iqtree_states: null argument"); return MPF_E_INVALID; }
  for (int64_t i = 0; i < count; i++) {
    const int st = states[i];
    int code = -1;
    if (datatype == MPF_DNA) {
      if (st >= 0 && st < 4) code = 1 << st;
      else if (st == 18) code = 15;                       // STATE_UNKNOWN
      else if (st >= 4 && st <= 17) code = st - 3;        // ambiguity: mask + 3 (phylotree.cpp:1135-1137)
      if (code == 15 && st != 18) code = -1;              // 1+2+4+8+3 is not produced by convertState
    } else if (datatype == MPF_AA) {
      if (st >= 0 && st <= 22) code = st;                 // same numbering, B = 20, Z = 21, unknown = 22
    } else if (datatype == MPF_BIN) {
      if (st == 0 || st == 1) code = 1 << st;             // SEQ_BINARY: '0' -> 0, '1' -> 1 (alignment.cpp:846-851)
      else if (st == 2) code = 3;                         // STATE_UNKNOWN = num_states
    } else if (datatype == MPF_GENERIC) {
      if (st >= 0 && st <= 32) code = st;                 // SEQ_MORPH: symbol index, STATE_UNKNOWN = num_states <= 32 handed over as 32
    } else {
      set_error("mpf_encode_iqtree_states: unsupported data type");
      return MPF_E_UNSUPPORTED;
    }
    if (code <= 0 && !((datatype == MPF_AA || datatype == MPF_GENERIC) && code == 0)) { set_error("state outside the alphabet (STATE_INVALID)"); return MPF_E_INVALID; }
    codes[i] = (uint8_t)code;
  }
  return MPF_OK;
}

int mpf_seed_ties(mpf_engine *e, int32_t tie_mode, int32_t seed)
{
  NEED(e);
  if (tie_mode != MPF_TIE_FIRST && tie_mode != MPF_TIE_RANDOM) { set_error("bad tie mode"); return MPF_E_INVALID; }
  e->eng.seed_ties(tie_mode, seed);
  return MPF_OK;
}

int mpf_set_rand_callback(mpf_engine *e, double (*fn)(void *), void *arg) { NEED(e); e->eng.set_rand(fn, arg); return MPF_OK; }

int mpf_set_tie_state(mpf_engine *e, uint64_t state)
{
  NEED(e);
  e->eng.set_rand(nullptr, nullptr);
  e->eng.set_tie_state(state);
  return MPF_OK;
}

uint64_t mpf_tie_state_after(uint64_t state, uint64_t n_draws) { return mpf::lcg64_skip(state, n_draws); }

int mpf_get_tie_state(const mpf_engine *e, uint64_t *state)
{
  NEED(e);
  if (!state) { set_error("null argument"); return MPF_E_INVALID; }
  *state = e->eng.tie_state();
  return MPF_OK;
}

int mpf_spr_scan(mpf_engine *e, int32_t rec, int32_t mintrav, int32_t maxtrav, int32_t cap, int32_t *q_recs,
                 uint32_t *mp, int32_t *n_p, int32_t *n_total)
{
  NEED(e);
  std::vector<int32_t> q;
  std::vector<uint32_t> m;
  int np = 0;
  int rc = e->eng.spr_scan(rec, mintrav, maxtrav, q, m, np);
  if (rc) return rc;
  if (n_total) *n_total = (int32_t)q.size();
  if (n_p) *n_p = np;
  if ((int)q.size() > cap) { set_error("mpf_spr_scan: output capacity too small"); return MPF_E_INVALID; }
  if (!q.empty()) {
    std::memcpy(q_recs, q.data(), q.size() * sizeof(int32_t));
    std::memcpy(mp, m.data(), m.size() * sizeof(uint32_t));
  }
  return MPF_OK;
}

int mpf_spr_sweep_scan(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint64_t *n_tests, uint32_t *min_mp)
{
  NEED(e);
  return e->eng.sweep_scan(mintrav, maxtrav, n_tests, min_mp);
}

int mpf_spr_sweep_costs(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint64_t cap, uint32_t *mp, uint64_t *offsets, uint64_t *n_tests)
{
  NEED(e);
  if (!n_tests || (cap && !mp)) { set_error("mpf_spr_sweep_costs: null output"); return MPF_E_INVALID; }
  return e->eng.sweep_costs(mintrav, maxtrav, cap, mp, offsets, n_tests);
}

int mpf_get_node_order(mpf_engine *e, int32_t *recs)
{
  NEED(e);
  if (!recs) { set_error("null output"); return MPF_E_INVALID; }
  return e->eng.node_order(recs);
}

int mpf_optimize_spr(mpf_engine *e, int32_t mintrav, int32_t maxtrav, uint32_t *score) { NEED(e); return e->eng.optimize_spr(mintrav, maxtrav, score); }

int mpf_optimize_spr_many(mpf_engine **engines, int32_t n_engines, int32_t mintrav, int32_t maxtrav, uint32_t *final_scores)
{
  if (n_engines < 0 || (n_engines && (!engines || !final_scores))) { set_error("mpf_optimize_spr_many: bad argument"); return MPF_E_INVALID; }
  std::vector<mpf::Engine *> es((size_t)n_engines);
  for (int k = 0; k < n_engines; k++) {
    if (!engines[k]) { set_error("mpf_optimize_spr_many: null engine"); return MPF_E_INVALID; }
    for (int j = 0; j < k; j++) if (engines[j] == engines[k]) { set_error("mpf_optimize_spr_many: an engine is listed twice"); return MPF_E_INVALID; }
    es[(size_t)k] = &engines[k]->eng;
  }
  return mpf::Engine::climb_many(es.data(), n_engines, mintrav, maxtrav, final_scores);
}

int mpf_optimize_spr_many_round(mpf_engine **engines, int32_t n_engines, int32_t mintrav, int32_t maxtrav, uint8_t *state, uint32_t *final_scores)
{
  if (n_engines < 0 || (n_engines && (!engines || !final_scores || !state))) { set_error("mpf_optimize_spr_many_round: bad argument"); return MPF_E_INVALID; }
  std::vector<mpf::Engine *> es((size_t)n_engines);
  for (int k = 0; k < n_engines; k++) {
    if (!engines[k]) { set_error("mpf_optimize_spr_many_round: null engine"); return MPF_E_INVALID; }
    // (two workgroups of one launch on one vector store)
    for (int j = 0; j < k; j++) if (engines[j] == engines[k]) { set_error("mpf_optimize_spr_many_round: an engine is listed twice"); return MPF_E_INVALID; }
    es[(size_t)k] = &engines[k]->eng;
  }
  return mpf::Engine::climb_many_round(es.data(), n_engines, mintrav, maxtrav, state, final_scores);
}

int mpf_make_parsimony_tree(mpf_engine *e, int64_t seed, int32_t spr_dist, uint32_t *score)
{
  NEED(e);
  return e->eng.make_parsimony_tree(seed, spr_dist, score);
}

int mpf_stepwise_addition(mpf_engine *e, int64_t seed, uint32_t *best_per_step, int32_t *insert_per_step, uint32_t *score)
{
  NEED(e);
  return e->eng.stepwise_addition(seed, best_per_step, insert_per_step, score);
}

// IQTree::optimizeNNI (reference iqtree.cpp:2173-2302), MP mode
int mpf_optimize_nni(mpf_engine *e, int32_t root_taxon, int32_t speednni, int32_t max_steps, uint32_t *score, int32_t *nni_count,
                     int32_t *nni_steps)
{
  NEED(e);
  return e->eng.optimize_nni(root_taxon, speednni != 0, max_steps, score, nni_count, nni_steps);
}

// IQTree::optimizeNNI with save_all_trees == 2 (-bb): saveCurrentTree at iqtree.cpp:2181-2183 and phylotree.cpp:3907-3939
int mpf_ufboot_optimize_nni(mpf_engine *e, int32_t root_taxon, int32_t speednni, int32_t max_steps, uint32_t *score, int32_t *nni_count,
                            int32_t *nni_steps)
{
  NEED(e);
  return e->eng.ufboot_optimize_nni(root_taxon, speednni != 0, max_steps, score, nni_count, nni_steps);
}

// IQTree::evalNNIs() (iqtree.cpp:3144-3159) with getBestNNIForBran (phylotree.cpp:3807-3980)
int mpf_nni_scores(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> l;
  const int rc = e->eng.nni_scores(root_taxon, br, l);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !len)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    len[2 * i] = l[2 * i];
    len[2 * i + 1] = l[2 * i + 1];
  }
  return MPF_OK;
}

// PhyloTree::fixNegativeBranch's branch_subst for every branch of the current tree (host/brlen.cpp)
int mpf_branch_substitutions(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *subst, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> s;
  const int rc = e->eng.branch_substitutions(root_taxon, br, s);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !subst)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    subst[i] = s[i];
  }
  return MPF_OK;
}

// the length fixNegativeBranch(force = true) makes of a branch's count (phylotree.cpp:3608-3614), in double precision on the host
static double parsimony_branch_length(int branch_subst, int n_sites, int S)
{
  double branch_length = (branch_subst > 0) ? ((double)branch_subst / n_sites) : (1.0 / n_sites);
  const double z = (double)S / (S - 1);
  const double x = 1.0 - (z * branch_length);
  if (x > 0) branch_length = -std::log(x) / z;
  if (branch_length < 1e-6) branch_length = 1e-6;      // MIN_BRANCH_LEN (phylotree.h:35)
  return branch_length;
}

// ... and the lengths fixNegativeBranch(force = true) makes of them (phylotree.cpp:3608-3614), in double precision on the host
int mpf_branch_lengths(mpf_engine *e, int32_t root_taxon, int32_t n_sites, int32_t unit_cost_parstree, int32_t cap, int32_t *node1,
                       int32_t *node2, double *length, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  if (n_sites < 1) { set_error("mpf_branch_lengths: n_sites must be positive"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> s;
  int rc = e->eng.branch_substitutions(root_taxon, br, s);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !length)) { set_error("null output"); return MPF_E_INVALID; }
  if (unit_cost_parstree && !e->eng.weighted()) {
    // a ParsTree under -cost fitch | e runs on the Fitch engine, but its computeParsimonyBranch is the override that hands back
    // tree_pars (parstree.cpp:534-535): every branch takes the length of the tree
    uint32_t len = 0;
    rc = e->eng.tree_length(&len);
    if (rc) return rc;
    std::fill(s.begin(), s.end(), len);
  }
  const int S = e->eng.S();
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    length[i] = parsimony_branch_length((int)s[i], n_sites, S);
  }
  return MPF_OK;
}

// ---- multifurcating trees (host/polytomy.cpp): computeParsimony() and fixNegativeBranch on a tree given as neighbour lists
int mpf_polytomy_parsimony(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, uint32_t *score,
                           uint16_t *pattern_pars)
{
  NEED(e);
  return e->eng.polytomy_parsimony(n_inner, first, nbr, root_taxon, score, pattern_pars);
}

int mpf_polytomy_branch_substitutions(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t cap,
                                      int32_t *node1, int32_t *node2, uint32_t *subst, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> s;
  const int rc = e->eng.polytomy_branch_substitutions(n_inner, first, nbr, root_taxon, br, s);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !subst)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    subst[i] = s[i];
  }
  return MPF_OK;
}

int mpf_polytomy_branch_lengths(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t n_sites,
                                int32_t unit_cost_parstree, int32_t cap, int32_t *node1, int32_t *node2, double *length, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  if (n_sites < 1) { set_error("mpf_polytomy_branch_lengths: n_sites must be positive"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> s;
  uint32_t len = 0;
  const bool unit = unit_cost_parstree && !e->eng.weighted();
  const int rc = e->eng.polytomy_branch_substitutions(n_inner, first, nbr, root_taxon, br, s, unit ? &len : nullptr);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !length)) { set_error("null output"); return MPF_E_INVALID; }
  if (unit) std::fill(s.begin(), s.end(), len);        // ParsTree under -cost fitch | e: every branch takes the tree's length (parstree.cpp:534-535)
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    length[i] = parsimony_branch_length((int)s[i], n_sites, e->eng.S());
  }
  return MPF_OK;
}

// ---- taxon insertion (host/place.cpp): addTaxonMPFast's tests on a backbone given as neighbour lists, computeParsimonyTree
int mpf_insertion_costs(mpf_engine *e, int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t n_query,
                        const int32_t *query_taxa, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *cost, int32_t *n, uint32_t *tree_length)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> d;
  uint32_t len = 0;
  const bool fill = (int64_t)cap >= 2 * (int64_t)n_inner + 1;       // (a binary backbone of m = n_inner + 2 tips has 2 m - 3 branches)
  const int rc = e->eng.place_costs(n_inner, first, nbr, root_taxon, n_query, query_taxa, br, fill ? &d : nullptr, nullptr, &len);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (tree_length) *tree_length = len;
  if (cap < *n) return MPF_OK;
  if (!node1 || !node2 || (n_query > 0 && !cost)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
  }
  const uint32_t base = e->eng.weighted() ? 0u : len;       // (the weighted kernel writes full lengths: there is no additive backbone length)
  for (int q = 0; q < n_query; q++)
    for (size_t i = 0; i < br.size(); i++) cost[(size_t)q * (size_t)cap + i] = base + d[(size_t)q * br.size() + i];
  return MPF_OK;
}

// ---- TBR (host/tbr.cpp): no reference function
int mpf_tbr_scan(mpf_engine *e, int32_t rec, int32_t maxtrav, int32_t cap_f, int32_t cap_g, int32_t *f_recs, int32_t *g_recs, uint32_t *cost,
                 int32_t *n_f, int32_t *n_g)
{
  NEED(e);
  if (!n_f || !n_g) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<int32_t> f, g;
  std::vector<uint32_t> c;
  // the lists first: the matrix is made only where it can be handed over
  int rc = e->eng.tbr_scan(rec, maxtrav, f, g, nullptr);
  if (rc) return rc;
  *n_f = (int32_t)f.size();
  *n_g = (int32_t)g.size();
  if ((int64_t)cap_f < (int64_t)f.size() || (int64_t)cap_g < (int64_t)g.size()) return MPF_OK;
  if ((!f.empty() && !f_recs) || (!g.empty() && !g_recs)) { set_error("null output"); return MPF_E_INVALID; }
  if (cost) {
    rc = e->eng.tbr_scan(rec, maxtrav, f, g, &c);
    if (rc) return rc;
    std::memcpy(cost, c.data(), c.size() * sizeof(uint32_t));
  }
  if (!f.empty()) std::memcpy(f_recs, f.data(), f.size() * sizeof(int32_t));
  if (!g.empty()) std::memcpy(g_recs, g.data(), g.size() * sizeof(int32_t));
  return MPF_OK;
}

int mpf_tbr_sweep_best(mpf_engine *e, int32_t maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs)
{
  NEED(e);
  if (!best_cost || !best_f || !best_g) { set_error("null output"); return MPF_E_INVALID; }
  return e->eng.tbr_sweep_best(maxtrav, best_cost, best_f, best_g, n_pairs);
}

int mpf_apply_tbr(mpf_engine *e, int32_t rec, int32_t f_rec, int32_t g_rec, uint32_t *score) { NEED(e); return e->eng.apply_tbr(rec, f_rec, g_rec, score); }

int mpf_optimize_tbr(mpf_engine *e, int32_t maxtrav, int32_t max_moves, uint32_t *score, int32_t *n_moves)
{
  NEED(e);
  return e->eng.optimize_tbr(maxtrav, max_moves, score, n_moves);
}

int mpf_get_tbr_moves(const mpf_engine *e, int32_t cap, int32_t *rec, int32_t *f_rec, int32_t *g_rec, uint32_t *score, int32_t *n_moves)
{
  NEED(e);
  const auto &mv = e->eng.tbr_moves();
  if (n_moves) *n_moves = (int32_t)mv.size();
  const size_t k = std::min((size_t)std::max(cap, 0), mv.size());
  for (size_t i = 0; i < k; i++) {
    if (rec) rec[i] = mv[i].rec;
    if (f_rec) f_rec[i] = mv[i].f_rec;
    if (g_rec) g_rec[i] = mv[i].g_rec;
    if (score) score[i] = mv[i].score;
  }
  return MPF_OK;
}

// ... under -bb: every entry of every visit booked through the tracker (host/tbr.cpp, "under -bb")
int mpf_ufboot_tbr_sweep(mpf_engine *e, int32_t maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs)
{
  NEED(e);
  if (!best_cost || !best_f || !best_g) { set_error("null output"); return MPF_E_INVALID; }
  return e->eng.ufboot_tbr_sweep(maxtrav, best_cost, best_f, best_g, n_pairs);
}

int mpf_ufboot_optimize_tbr(mpf_engine *e, int32_t maxtrav, int32_t max_moves, uint32_t *score, int32_t *n_moves)
{
  NEED(e);
  return e->eng.ufboot_optimize_tbr(maxtrav, max_moves, score, n_moves);
}

int mpf_tbr_pattern_terms(mpf_engine *e, int32_t rec, int32_t maxtrav, int64_t cap_entries, uint8_t *terms, int32_t *n_f, int32_t *n_g)
{
  NEED(e);
  if (!n_f || !n_g) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<int32_t> f, g;
  std::vector<uint8_t> t;
  // the lists first: the rows are made only where they can be handed over
  int rc = e->eng.tbr_pattern_terms(rec, maxtrav, f, g, nullptr);
  if (rc) return rc;
  *n_f = (int32_t)f.size();
  *n_g = (int32_t)g.size();
  if (cap_entries < (int64_t)(1 + f.size()) * (int64_t)(1 + g.size())) return MPF_OK;
  if (!terms) { set_error("null output"); return MPF_E_INVALID; }
  rc = e->eng.tbr_pattern_terms(rec, maxtrav, f, g, &t);
  if (rc) return rc;
  std::memcpy(terms, t.data(), t.size());
  return MPF_OK;
}

int mpf_tbr_pattern_lengths(mpf_engine *e, int32_t rec, int32_t maxtrav, int64_t cap_entries, uint16_t *rows, int32_t *n_f, int32_t *n_g)
{
  NEED(e);
  if (!n_f || !n_g) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<int32_t> f, g;
  std::vector<uint16_t> t;
  // the lists first: the rows are made only where they can be handed over
  int rc = e->eng.tbr_pattern_lengths(rec, maxtrav, f, g, nullptr);
  if (rc) return rc;
  *n_f = (int32_t)f.size();
  *n_g = (int32_t)g.size();
  if (cap_entries < (int64_t)(1 + f.size()) * (int64_t)(1 + g.size())) return MPF_OK;
  if (!rows) { set_error("null output"); return MPF_E_INVALID; }
  rc = e->eng.tbr_pattern_lengths(rec, maxtrav, f, g, &t);
  if (rc) return rc;
  std::memcpy(rows, t.data(), t.size() * sizeof(uint16_t));
  return MPF_OK;
}

int mpf_place_taxa(mpf_engine *e,int32_t n_inner, const int32_t *first, const int32_t *nbr, int32_t root_taxon, int32_t n_query,
                   const int32_t *query_taxa, int32_t *best_branch, int32_t *best_node1, int32_t *best_node2, uint32_t *best_length,
                   uint32_t *tree_length)
{
  NEED(e);
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<mpf::Engine::PlaceBest> best;
  uint32_t len = 0;
  const int rc = e->eng.place_costs(n_inner, first, nbr, root_taxon, n_query, query_taxa, br, nullptr, &best, &len);
  if (rc) return rc;
  if (tree_length) *tree_length = len;
  for (int q = 0; q < n_query; q++) {
    const mpf::Engine::NniBranch at = br[(size_t)best[(size_t)q].branch];
    if (best_branch) best_branch[q] = (int32_t)best[(size_t)q].branch;
    if (best_node1) best_node1[q] = at.node1;
    if (best_node2) best_node2[q] = at.node2;
    if (best_length) best_length[q] = (e->eng.weighted() ? 0u : len) + best[(size_t)q].delta;
  }
  return MPF_OK;
}

int mpf_iq_parsimony_tree(mpf_engine *e, uint64_t *tie_state, int32_t *order, int32_t *first, int32_t *nbr, uint32_t *length_per_step,
                          uint32_t *score)
{
  NEED(e);
  if (!order || !first || !nbr) { set_error("mpf_iq_parsimony_tree: null argument"); return MPF_E_INVALID; }
  const int n = e->eng.n();
  if (tie_state) mpf::place_shuffle_order(n, tie_state, order);
  std::vector<int32_t> f, nb;
  std::vector<uint32_t> len((size_t)std::max(n - 2, 1), 0u);
  const int rc = e->eng.parsimony_tree(order, f, nb, len.data());
  if (rc) return rc;
  std::copy(f.begin(), f.end(), first);
  std::copy(nb.begin(), nb.end(), nbr);
  if (length_per_step) std::copy(len.begin(), len.end(), length_per_step);
  if (score) *score = len.back();
  return MPF_OK;
}

// ---- the summary of a -bb run (host/splits.cpp): MTreeSet::convertSplits, the supports on a tree, computeConsensusTree
static int split_counts_out(const mpf::splitsets::SplitTable &t, int32_t cap, uint32_t *bits, int64_t *count, int32_t *n_distinct)
{
  if (n_distinct) *n_distinct = (int32_t)t.size();
  const size_t m = std::min<size_t>(t.size(), cap > 0 ? (size_t)cap : 0);
  if (m && (!bits || !count)) { set_error("null output"); return MPF_E_INVALID; }
  if (m) {
    std::memcpy(bits, t.bits.data(), m * (size_t)t.words * sizeof(uint32_t));
    std::memcpy(count, t.count.data(), m * sizeof(int64_t));
  }
  return MPF_OK;
}

static int consensus_out(const mpf::splitsets::ListTree &t, int32_t *n_inner, int32_t *first, int32_t *nbr, int64_t *support_of_inner)
{
  if (!n_inner || !first || !nbr) { set_error("null output"); return MPF_E_INVALID; }
  *n_inner = t.n_inner();
  std::copy(t.first.begin(), t.first.end(), first);
  std::copy(t.nbr.begin(), t.nbr.end(), nbr);
  if (support_of_inner) std::copy(t.support.begin(), t.support.end(), support_of_inner);
  return MPF_OK;
}

int mpf_split_counts(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, int32_t cap, uint32_t *bits, int64_t *count,
                     int32_t *n_distinct, int64_t *total_weight)
{
  NEED(e);
  if (!n_distinct) { set_error("null output"); return MPF_E_INVALID; }
  mpf::splitsets::SplitTable t;
  const int rc = e->eng.split_counts(n_trees, backs, weights, t);
  if (rc) return rc;
  if (total_weight) *total_weight = t.total;
  return split_counts_out(t, cap, bits, count, n_distinct);
}

int mpf_split_support(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, const int32_t *target_back, int32_t cap,
                      int32_t *node1, int32_t *node2, int64_t *support, int32_t *n, int64_t *total_weight)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<int64_t> sup;
  const int rc = e->eng.split_support(n_trees, backs, weights, target_back, br, sup, total_weight);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !support)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    support[i] = sup[i];
  }
  return MPF_OK;
}

int mpf_consensus_tree(mpf_engine *e, int32_t n_trees, const int32_t *backs, const int32_t *weights, double threshold, int32_t *n_inner,
                       int32_t *first, int32_t *nbr, int64_t *support_of_inner, int64_t *total_weight)
{
  NEED(e);
  mpf::splitsets::ListTree t;
  const int rc = e->eng.consensus_tree(n_trees, backs, weights, threshold, t, total_weight);
  if (rc) return rc;
  return consensus_out(t, n_inner, first, nbr, support_of_inner);
}

// MTreeSet::computeRFDist (host/rf.cpp)
static_assert(MPF_RF_ALL_PAIRS == mpf::splitsets::RF_ALL_PAIRS && MPF_RF_ADJACENT == mpf::splitsets::RF_ADJACENT &&
              MPF_RF_TWO_SETS == mpf::splitsets::RF_TWO_SETS, "the modes of mpf_rf_distances");
int mpf_rf_distances(mpf_engine *e, int32_t mode, int32_t n_trees, const int32_t *backs, int32_t n_trees2, const int32_t *backs2, int64_t cap,
                     int32_t *rf)
{
  NEED(e);
  return e->eng.rf_distances(mode, n_trees, backs, n_trees2, backs2, cap, rf);
}

// ---- the same four results on sets that mix record-format trees and trees given as neighbour lists (host/splits.cpp, host/rf.cpp)
static mpf::splitsets::TreeSet tree_set_of(const mpf_tree_set *s)
{
  mpf::splitsets::TreeSet t;
  if (!s) return t;
  t.n_records = s->n_records;
  t.backs = s->backs;
  t.n_lists = s->n_lists;
  t.n_inner = s->n_inner;
  t.first = s->first;
  t.nbr = s->nbr;
  return t;
}

int mpf_split_counts_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, int32_t cap, uint32_t *bits, int64_t *count,
                         int32_t *n_distinct, int64_t *total_weight)
{
  NEED(e);
  if (!n_distinct) { set_error("null output"); return MPF_E_INVALID; }
  mpf::splitsets::SplitTable t;
  const int rc = e->eng.split_counts(tree_set_of(s), weights, t);
  if (rc) return rc;
  if (total_weight) *total_weight = t.total;
  return split_counts_out(t, cap, bits, count, n_distinct);
}

int mpf_split_support_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, int32_t target_n_inner, const int32_t *target_first,
                          const int32_t *target_nbr, int32_t cap, int32_t *node1, int32_t *node2, int64_t *support, int32_t *n,
                          int64_t *total_weight)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<int64_t> sup;
  mpf::splitsets::TreeRef target;
  target.n_inner = target_n_inner;
  target.first = target_first;
  target.nbr = target_nbr;
  const int rc = e->eng.split_support(tree_set_of(s), weights, target, br, sup, total_weight);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !support)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    support[i] = sup[i];
  }
  return MPF_OK;
}

int mpf_consensus_tree_set(mpf_engine *e, const mpf_tree_set *s, const int32_t *weights, double threshold, int32_t *n_inner, int32_t *first,
                           int32_t *nbr, int64_t *support_of_inner, int64_t *total_weight)
{
  NEED(e);
  mpf::splitsets::ListTree t;
  const int rc = e->eng.consensus_tree(tree_set_of(s), weights, threshold, t, total_weight);
  if (rc) return rc;
  return consensus_out(t, n_inner, first, nbr, support_of_inner);
}

int mpf_rf_distances_set(mpf_engine *e, int32_t mode, const mpf_tree_set *s1, const mpf_tree_set *s2, int64_t cap, int32_t *rf)
{
  NEED(e);
  return e->eng.rf_distances(mode, tree_set_of(s1), tree_set_of(s2), cap, rf);
}

int mpf_ufboot_summary_trees(mpf_engine *e, int32_t rule, int32_t cap, int64_t *tree_index, int32_t *weights, int32_t *backs, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<int32_t> bk, w;
  std::vector<int64_t> idx;
  const int rc = e->eng.ufboot_summary_trees(rule, bk, w, idx);
  if (rc) return rc;
  *n = (int32_t)idx.size();
  if (cap < *n) return MPF_OK;
  if (tree_index) std::copy(idx.begin(), idx.end(), tree_index);
  if (weights) std::copy(w.begin(), w.end(), weights);
  if (backs) std::copy(bk.begin(), bk.end(), backs);
  return MPF_OK;
}

int mpf_ufboot_summarize(mpf_engine *e, int32_t rule, mpf_bb_summary *s)
{
  NEED(e);
  if (!s) { set_error("null argument"); return MPF_E_INVALID; }
  std::vector<int32_t> bk, w;
  std::vector<int64_t> idx;
  int rc = e->eng.ufboot_summary_trees(rule, bk, w, idx);
  if (rc) return rc;
  const int32_t T = (int32_t)idx.size();
  s->n_trees = T;
  s->n_distinct = s->n_branches = s->n_inner = 0;
  s->total_weight = 0;
  for (int32_t x : w) s->total_weight += x;
  {
    mpf::splitsets::SplitTable t;
    rc = e->eng.split_counts(T, bk.data(), w.data(), t);
    if (rc) return rc;
    rc = split_counts_out(t, s->bits && s->count ? s->split_cap : 0, s->bits, s->count, &s->n_distinct);
    if (rc) return rc;
  }
  if (s->target_back) {
    std::vector<mpf::Engine::NniBranch> br;
    std::vector<int64_t> sup;
    rc = e->eng.split_support(T, bk.data(), w.data(), s->target_back, br, sup, nullptr);
    if (rc) return rc;
    s->n_branches = (int32_t)br.size();
    if (s->branch_cap >= s->n_branches && s->node1 && s->node2 && s->support)
      for (size_t i = 0; i < br.size(); i++) {
        s->node1[i] = br[i].node1;
        s->node2[i] = br[i].node2;
        s->support[i] = sup[i];
      }
  }
  if (s->first && s->nbr) {
    mpf::splitsets::ListTree t;
    rc = e->eng.consensus_tree(T, bk.data(), w.data(), s->threshold, t, nullptr);
    if (rc) return rc;
    rc = consensus_out(t, &s->n_inner, s->first, s->nbr, s->support_of_inner);
    if (rc) return rc;
  }
  return MPF_OK;
}

// mpf_nni_scores by the mask-writing kernel of the tracked climb, its rows per pattern
int mpf_nni_pattern_terms(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len, uint8_t *terms, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> l;
  std::vector<uint8_t> t;
  const int rc = e->eng.nni_pattern_terms(root_taxon, br, l, t);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (*n && (!node1 || !node2 || !len || !terms)) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    len[2 * i] = l[2 * i];
    len[2 * i + 1] = l[2 * i + 1];
  }
  std::copy(t.begin(), t.end(), terms);
  return MPF_OK;
}

// ... by the row-writing kernel of the tracked weighted climb, its rows per pattern
int mpf_nni_pattern_lengths(mpf_engine *e, int32_t root_taxon, int32_t cap, int32_t *node1, int32_t *node2, uint32_t *len, uint16_t *rows, int32_t *n)
{
  NEED(e);
  if (!n) { set_error("null output"); return MPF_E_INVALID; }
  std::vector<mpf::Engine::NniBranch> br;
  std::vector<uint32_t> l;
  std::vector<uint16_t> r;
  const int rc = e->eng.nni_pattern_lengths(root_taxon, br, l, r);
  if (rc) return rc;
  *n = (int32_t)br.size();
  if (cap < *n) return MPF_OK;
  if (!rows || (*n && (!node1 || !node2 || !len))) { set_error("null output"); return MPF_E_INVALID; }
  for (size_t i = 0; i < br.size(); i++) {
    node1[i] = br[i].node1;
    node2[i] = br[i].node2;
    len[2 * i] = l[2 * i];
    len[2 * i + 1] = l[2 * i + 1];
  }
  std::copy(r.begin(), r.end(), rows);
  return MPF_OK;
}

// the PhyloTree::doNNI calls (phylotree.cpp:3715-3742) of the last climb
int mpf_get_nni_moves(const mpf_engine *e, int32_t cap, int32_t *node1, int32_t *slot1, int32_t *node2, int32_t *slot2, int32_t *n)
{
  NEED(e);
  const auto &lg = e->eng.nni_log();
  if (n) *n = (int32_t)lg.size();
  const size_t k = std::min((size_t)std::max(cap, 0), lg.size());
  for (size_t i = 0; i < k; i++) {
    if (node1) node1[i] = lg[i].node1;
    if (slot1) slot1[i] = lg[i].slot1;
    if (node2) node2[i] = lg[i].node2;
    if (slot2) slot2[i] = lg[i].slot2;
  }
  return MPF_OK;
}

int mpf_get_moves(const mpf_engine *e, int32_t cap, int32_t *remove_rec, int32_t *insert_rec, uint32_t *score, int32_t *n_moves)
{
  NEED(e);
  const auto &mv = e->eng.moves();
  if (n_moves) *n_moves = (int32_t)mv.size();
  const size_t k = std::min((size_t)std::max(cap, 0), mv.size());
  for (size_t i = 0; i < k; i++) {
    if (remove_rec) remove_rec[i] = mv[i].remove_rec;
    if (insert_rec) insert_rec[i] = mv[i].insert_rec;
    if (score) score[i] = mv[i].score;
  }
  return MPF_OK;
}

int mpf_ufboot_attach(mpf_engine *e, int32_t n_samples, const uint16_t *samples, double epsilon)
{
  NEED(e);
  return e->eng.ufboot_attach(n_samples, samples, epsilon);
}
int mpf_ufboot_attach_sharded(mpf_engine *e, int32_t n_samples, int32_t n_local, const int32_t *sample_ids,
                              const uint16_t *samples_local, double epsilon, mpf_ufb_exchange_fn exchange, void *arg)
{
  NEED(e);
  if (n_local < 1 || n_local > n_samples || !sample_ids || !exchange) { set_error("mpf_ufboot_attach_sharded: bad argument"); return MPF_E_INVALID; }
  return e->eng.ufboot_attach(n_samples, samples_local, epsilon, n_local, sample_ids, exchange, arg);
}
int mpf_ufboot_detach(mpf_engine *e) { NEED(e); e->eng.ufboot_detach(); return MPF_OK; }
int mpf_ufboot_set_cutoff(mpf_engine *e, double logl_cutoff) { NEED(e); return e->eng.ufboot_set_cutoff(logl_cutoff); }
int mpf_ufboot_set_ratchet_booking(mpf_engine *e, int32_t on) { NEED(e); return e->eng.ufboot_set_ratchet_booking(on); }
int mpf_ufboot_set_mulhits(mpf_engine *e, int32_t on) { NEED(e); return e->eng.ufboot_set_mulhits(on); }
int mpf_ufboot_set_cutoff_from_btrees(mpf_engine *e, int32_t on) { NEED(e); return e->eng.ufboot_set_cutoff_from_btrees(on); }
int mpf_ufboot_get_orig_logl(const mpf_engine *e, int32_t *out)
{
  if (!e || !out) { set_error("mpf_ufboot_get_orig_logl: bad argument"); return MPF_E_INVALID; }
  e->eng.activate();
  return e->eng.ufboot_orig_logl(out);
}
int mpf_ufboot_set_store_trees(mpf_engine *e, int32_t on) { NEED(e); return e->eng.ufboot_set_store_trees(on); }
int mpf_ufboot_get_duplicates(const mpf_engine *e, uint64_t *n) { NEED(e); return e->eng.ufboot_duplicates(n); }
int mpf_ufboot_set_topboot(mpf_engine *e, int32_t n_top) { NEED(e); return e->eng.ufboot_set_topboot(n_top); }
int mpf_ufboot_get_sample_top(const mpf_engine *e, int32_t sample, int64_t *trees, int32_t *rell, int32_t cap, int32_t *n, int32_t *threshold)
{
  NEED(e);
  int k = 0;
  int rc = e->eng.ufboot_sample_top(sample, trees, rell, cap, &k, threshold);
  if (!rc && n) *n = k;
  return rc;
}
int mpf_ufboot_set_distinct_iter(mpf_engine *e, int32_t k) { NEED(e); return e->eng.ufboot_set_distinct_iter(k); }
int mpf_ufboot_set_iteration(mpf_engine *e, int32_t cur_it) { NEED(e); return e->eng.ufboot_set_iteration(cur_it); }
int mpf_ufboot_get_sample_iters(const mpf_engine *e, int32_t sample, int32_t *iters, int32_t cap, int32_t *n)
{
  NEED(e);
  int k = 0;
  int rc = e->eng.ufboot_sample_iters(sample, iters, cap, &k);
  if (!rc && n) *n = k;
  return rc;
}
int mpf_ufboot_get_sample_trees(const mpf_engine *e, int32_t sample, int64_t *out, int32_t cap, int32_t *n)
{
  NEED(e);
  int k = 0;
  int rc = e->eng.ufboot_sample_trees(sample, out, cap, &k);
  if (!rc && n) *n = k;
  return rc;
}
int mpf_ufboot_next_cutoff(const mpf_engine *e, int32_t percent, double *logl_cutoff)
{
  NEED(e);
  if (!logl_cutoff || percent < 0 || percent > 100) { set_error("mpf_ufboot_next_cutoff: bad argument"); return MPF_E_INVALID; }
  if (!e->eng.ufboot_attached()) { set_error("no UFBoot tracker attached"); return MPF_E_STATE; }
  *logl_cutoff = e->eng.ufboot_next_cutoff(percent);
  return MPF_OK;
}
int mpf_ufboot_num_trees(const mpf_engine *e, int64_t *n_trees)
{
  NEED(e);
  if (!n_trees) { set_error("null output"); return MPF_E_INVALID; }
  if (!e->eng.ufboot_attached()) { set_error("no UFBoot tracker attached"); return MPF_E_STATE; }
  *n_trees = e->eng.ufboot_n_trees();
  return MPF_OK;
}
int mpf_ufboot_tree_logl(const mpf_engine *e, double *out) { NEED(e); if (!out) { set_error("null output"); return MPF_E_INVALID; } return e->eng.ufboot_tree_logl(out); }
int mpf_ufboot_get_state(const mpf_engine *e, double *boot_logl, int32_t *boot_counts, int32_t *boot_trees)
{
  NEED(e);
  return e->eng.ufboot_state(boot_logl, boot_counts, boot_trees);
}
int mpf_ufboot_get_tree(const mpf_engine *e, int64_t tree_index, int32_t *back)
{
  NEED(e);
  if (!back) { set_error("null output"); return MPF_E_INVALID; }
  return e->eng.ufboot_tree(tree_index, back);
}
int mpf_ufboot_adopt(mpf_engine *e, int32_t n_updates, const int32_t *sample, const uint32_t *score, const int32_t *tree_of, int32_t n_trees,
                     const int32_t *backs, const uint32_t *lengths, int32_t *n_taken)
{
  NEED(e);
  return e->eng.ufboot_adopt(n_updates, sample, score, tree_of, n_trees, backs, lengths, n_taken);
}
int mpf_ufboot_refine_sweep(mpf_engine *e, int32_t maxtrav, const int32_t *tie_seeds, uint32_t *scores, uint8_t *stable, int32_t *first_move_visit)
{
  NEED(e);
  return e->eng.ufboot_refine_sweep(maxtrav, tie_seeds, scores, stable, first_move_visit);
}

int mpf_ufboot_get_counters(const mpf_engine *e, uint64_t *tie_draws, uint64_t *events, uint64_t *reps_rows, double *reps_kernel_ms)
{
  NEED(e);
  return e->eng.ufboot_counters(tie_draws, events, reps_rows, reps_kernel_ms);
}

int mpf_get_stats(const mpf_engine *e, mpf_stats *out) { NEED(e); *out = e->eng.stats; return MPF_OK; }
int mpf_reset_stats(mpf_engine *e) { NEED(e); e->eng.reset_stats(); return MPF_OK; }

int mpf_set_option(mpf_engine *e, const char *key, int64_t value)
{
  NEED(e);
  if (!key) { set_error("null option key"); return MPF_E_INVALID; }
  return e->eng.set_option(key, value);
}
int mpf_get_scan_trace(mpf_engine *e, uint64_t *out, uint64_t cap, uint64_t *n_words)
{
  NEED(e);
  if (!n_words || (cap && !out)) { set_error("null output"); return MPF_E_INVALID; }
  return e->eng.scan_trace(out, cap, n_words);
}

int mpf_get_option(const mpf_engine *e, const char *key, int64_t *value)
{
  NEED(e);
  if (!key || !value) { set_error("null argument"); return MPF_E_INVALID; }
  return e->eng.get_option(key, value);
}

}  // extern "C"
