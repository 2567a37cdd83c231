// polytomy.cpp -- multifurcating trees: length, per-pattern lengths and the branch substitutions of a tree given as neighbour lists.
//
// Every -bb run of the reference ends on one: computeConsensusTree writes the bootstrap consensus, the host reads it back, calls
// fixNegativeBranch(true) and computeParsimony() on it and prints "Parsimony score of consensus tree" (phyloanalysis.cpp:2263-2307);
// a majority-rule consensus is rarely fully resolved.  User trees with polytomies reach -comppars, -wspars-user-tree and -parsbran
// the same way.  back[] holds three records per inner node and cannot express such a tree, so it comes as CSR neighbour lists and
// never becomes the engine's own tree: the calls are stateless towards it.
//
// The rules at a node of degree > 3 are the reference's generic ones (polytomy.hip).  The Fitch one counts ONE step per node with an
// empty intersection whatever the degree, so it undercounts a hard polytomy and depends on the root leaf; it is what the reference
// prints.  Store: the Sum deg <= 3 (n - 2) directed views of the inner nodes go into the engine's own inner slots (row-major half
// only) and every vector of the engine's tree is marked stale afterwards -- the next call on that tree refreshes them, and with
// nothing valid the word-major copy has nothing to disagree with (Engine::invalidate_vectors).
#include <string>

#include "ufboot_common.hpp"

namespace mpf {

// items of the view launch (listtree::plan_views): up views by height, the root edge (Fitch), down views by depth
int Engine::polytomy_views(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, bool all_views, PolyTree &t, bool checked)
{
  std::string why;
  if (!checked && !listtree::check(n_, n_inner, first, nbr, root_taxon, false, t.shape, &why)) { set_error("polytomy tree: " + why); return MPF_E_INVALID; }
  // whatever the engine's own tree has under way is finished first; its vectors are about to be overwritten
  if (cnt_copy_pending_) {
    HIPCHK(hipMemcpyAsync(h_cnt(), d_cnt(), nslots_ * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    cnt_copy_pending_ = false;
  }
  HIPCHK(hipStreamSynchronize(st_));
  finish_views();
  invalidate_vectors();
  listtree::ViewPlan &pl = t.plan;
  if (!listtree::plan_views(n_, n_inner, first, nbr, t.shape, all_views, !sankoff_, pl)) { set_error("polytomy tree: inconsistent neighbour lists"); return MPF_E_INVALID; }
  const size_t n_items = pl.items.size();
  const int n_lev = pl.n_lev;
  // one upload: items | outs | inputs | level offsets
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_items = 0, o_outs = al(o_items + n_items * sizeof(PolyItem)), o_in = al(o_outs + pl.outs.size() * sizeof(PolyOut)),
               o_lev = al(o_in + pl.inputs.size() * sizeof(uint32_t)), bytes = al(o_lev + pl.lev_off.size() * sizeof(int32_t));
  HIPCHK(h_poly_stage_.reserve(bytes));
  HIPCHK(d_poly_stage_.reserve(bytes));
  std::memcpy(h_poly_stage_.p + o_items, pl.items.data(), n_items * sizeof(PolyItem));
  std::memcpy(h_poly_stage_.p + o_outs, pl.outs.data(), pl.outs.size() * sizeof(PolyOut));
  std::memcpy(h_poly_stage_.p + o_in, pl.inputs.data(), pl.inputs.size() * sizeof(uint32_t));
  std::memcpy(h_poly_stage_.p + o_lev, pl.lev_off.data(), pl.lev_off.size() * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(d_poly_stage_.p, h_poly_stage_.p, bytes, hipMemcpyHostToDevice, st_));
  if (!sankoff_) HIPCHK(d_poly_masks_.reserve((size_t)pl.n_rows * (size_t)g_.Wp));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  HIPCHK(launch_poly_views(st_, g_, vec_rows(), reinterpret_cast<const PolyItem *>(d_poly_stage_.p + o_items),
                           reinterpret_cast<const PolyOut *>(d_poly_stage_.p + o_outs), reinterpret_cast<const uint32_t *>(d_poly_stage_.p + o_in),
                           reinterpret_cast<const int32_t *>(d_poly_stage_.p + o_lev), n_lev, d_poly_masks_.p, poly_tile_));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  poly_view_timed_ = timing_ != 0;
  poly_launches_++;
  poly_views_ += pl.outs.size() - (sankoff_ ? 0 : 1);
  return MPF_OK;
}

void Engine::polytomy_view_time()
{
  float ms = 0.f;
  if (poly_view_timed_ && hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) poly_view_ns_ += (uint64_t)((double)ms * 1e6);
  poly_view_timed_ = false;
}

// PhyloTree::computeParsimony() / ParsTree::computeParsimony() at the root leaf: computeParsimonyBranch(root->neighbors[0], root)
int Engine::polytomy_parsimony(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, uint32_t *score, uint16_t *pattern_pars)
{
  PolyTree &t = poly_tree_;
  int rc = polytomy_views(n_inner, first, nbr, root_taxon, false, t);
  if (rc) return rc;
  const uint32_t rest = t.plan.up_slot[(size_t)t.shape.tip_nb[(size_t)root_taxon]], leaf = (uint32_t)(root_taxon - 1);
  uint32_t len = 0;
  if (sankoff_) {
    // min_i( rest[i] + min_j( leaf[j] + cost[i][j] ) ): the rest of the tree as the parent side, as mpf_compute_parsimony_at
    EvOp op{rest, leaf, 0, 0};
    DevBuf<uint16_t> &d_p = d_poly_ptn_;
    PinBuf<uint16_t> &hp = h_poly_ptn_;
    HIPCHK(d_evops_.reserve(1));
    HIPCHK(reserve_results(1));
    HIPCHK(d_p.reserve((size_t)g_.Wp));
    HIPCHK(hp.reserve((size_t)g_.Wp));
    HIPCHK(hipMemcpyAsync(d_evops_.p, &op, sizeof(op), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemsetAsync(d_out(), 0, clear_words(1) * sizeof(uint32_t), st_));
    HIPCHK(launch_evaluate(st_, g_, vec_rows(), d_evops_.p, 1, d_out()));
    HIPCHK(hipMemcpyAsync(h_out(), d_out(), sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    if (pattern_pars) {
      HIPCHK(launch_sankoff_pattern(st_, g_, vec_rows(), rest, leaf, d_p.p));
      HIPCHK(hipMemcpyAsync(hp.p, d_p.p, (size_t)g_.Wp * sizeof(uint16_t), hipMemcpyDeviceToHost, st_));
    }
    HIPCHK(hipStreamSynchronize(st_));
    polytomy_view_time();
    len = h_out()[0];
    if (pattern_pars) {
      for (int k = 0; k < P_; k++) pattern_pars[k] = 0;
      for (int j = 0; j < ninf_; j++) pattern_pars[inf_index_[(size_t)j]] = hp.p[(size_t)j];
    }
  } else {
    const size_t rows = (size_t)t.plan.n_rows;
    DevBuf<uint32_t> &planes = d_poly_planes_;
    DevBuf<uint16_t> &d_ptn = d_poly_ptn_;
    HIPCHK(d_poly_cnt_.reserve(rows));
    HIPCHK(h_poly_cnt_.reserve(rows));
    HIPCHK(launch_poly_rowsum(st_, g_, d_poly_masks_.p, (int)rows, d_poly_cnt_.p));
    HIPCHK(hipMemcpyAsync(h_poly_cnt_.p, d_poly_cnt_.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    if (pattern_pars) {
      HIPCHK(planes.reserve(site_planes_words(g_, (int)rows)));
      HIPCHK(d_ptn.reserve((size_t)P_));
      HIPCHK(h_poly_ptn_.reserve((size_t)P_));
      if (poly_first_gen_ != pack_gen_) {               // the patterns' first sites follow the packing: uploaded once per re-pack
        HIPCHK(d_poly_first_.reserve((size_t)P_));
        HIPCHK(hipMemcpyAsync(d_poly_first_.p, first_site_.data(), (size_t)P_ * sizeof(int32_t), hipMemcpyHostToDevice, st_));
        poly_first_gen_ = pack_gen_;
      }
      HIPCHK(launch_poly_site_counts(st_, g_, d_poly_masks_.p, (int)rows, planes.p, d_poly_first_.p, P_, d_ptn.p));
      HIPCHK(hipMemcpyAsync(h_poly_ptn_.p, d_ptn.p, (size_t)P_ * sizeof(uint16_t), hipMemcpyDeviceToHost, st_));
    }
    HIPCHK(hipStreamSynchronize(st_));
    polytomy_view_time();
    if (pattern_pars) std::copy(h_poly_ptn_.p, h_poly_ptn_.p + P_, pattern_pars);
    for (size_t i = 0; i < rows; i++) len += h_poly_cnt_.p[i];
  }
  if (pattern_pars) {
    long sum = 0;
    for (int k = 0; k < P_; k++) sum += (long)pattern_pars[k] * wgt_[(size_t)k];
    if ((uint32_t)sum != len) { set_error("per-pattern lengths do not add up to the tree length"); return MPF_E_STATE; }
  }
  if (score) *score = len;
  return MPF_OK;
}

// fixNegativeBranch's computeParsimonyBranch(.., &branch_subst) for every branch: the contract of Engine::branch_substitutions with
// the two sides of a branch made by the k-ary rule.  fitch_len (Fitch engine, may be null): the tree's length, for unit_cost_parstree
int Engine::polytomy_branch_substitutions(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, std::vector<NniBranch> &br,
                                          std::vector<uint32_t> &subst, uint32_t *fitch_len)
{
  PolyTree &t = poly_tree_;
  int rc = polytomy_views(n_inner, first, nbr, root_taxon, true, t);
  if (rc) return rc;
  const int n = n_;
  listtree::branches(t.shape, br);
  const size_t nb = br.size();
  subst.assign(nb, 0u);
  HIPCHK(h_br_desc_.reserve(nb));
  HIPCHK(d_br_desc_.reserve(nb));
  HIPCHK(h_br_out_.reserve(nb));
  HIPCHK(d_br_out_.reserve(nb));
  if (!listtree::branch_sides(n, n_inner, first, nbr, t.shape, t.plan, h_br_desc_.p)) { set_error("polytomy tree: inconsistent walk"); return MPF_E_STATE; }
  // the orientation of Engine::branch_substitutions (parstree.cpp:439-541 and the leaf swap at :449-457)
  if (sankoff_)
    for (size_t i = 0; i < nb; i++)
      if (br[i].node2 <= n) std::swap(h_br_desc_.p[i].a, h_br_desc_.p[i].b);
  const int vw = tile_shape(brlen_vw_, false).vw;                                  // (the row-major store only: no word-major copy of these views)
  HIPCHK(hipMemcpyAsync(d_br_desc_.p, h_br_desc_.p, nb * sizeof(BranchDesc), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(d_br_out_.p, 0, nb * sizeof(uint32_t), st_));
  if (timing_) HIPCHK(hipEventRecord(ev2_, st_));
  if (sankoff_) HIPCHK(launch_snk_branch_eval(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, force_big_ != 0));
  else HIPCHK(launch_branch_subst(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, vw, false));
  if (timing_) HIPCHK(hipEventRecord(ev3_, st_));
  HIPCHK(hipMemcpyAsync(h_br_out_.p, d_br_out_.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  const size_t rows = (size_t)t.plan.n_rows;
  if (fitch_len && !sankoff_) {
    HIPCHK(d_poly_cnt_.reserve(rows));
    HIPCHK(h_poly_cnt_.reserve(rows));
    HIPCHK(launch_poly_rowsum(st_, g_, d_poly_masks_.p, (int)rows, d_poly_cnt_.p));
    HIPCHK(hipMemcpyAsync(h_poly_cnt_.p, d_poly_cnt_.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  }
  HIPCHK(hipStreamSynchronize(st_));
  polytomy_view_time();
  float ms = 0.f;
  if (timing_ && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) poly_branch_ns_ += (uint64_t)((double)ms * 1e6);
  std::copy(h_br_out_.p, h_br_out_.p + nb, subst.begin());
  if (fitch_len && !sankoff_) {
    uint32_t len = 0;
    for (size_t i = 0; i < rows; i++) len += h_poly_cnt_.p[i];
    *fitch_len = len;
  }
  return MPF_OK;
}

}  // namespace mpf
