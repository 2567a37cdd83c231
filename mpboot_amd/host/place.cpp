// place.cpp -- taxon insertion: what it costs to attach taxon t to branch b of a tree that does not hold t yet.
//
// Reference: PhyloTree::addTaxonMPFast (phylotree.cpp:1322-1378) under PhyloTree::computeParsimonyTree (phylotree.cpp:1243-1320, the
// start tree of -starttree PARS) and IQTree::reinsertLeavesByParsimony (iqtree.cpp:981-1016).  The backbone is a binary tree over a
// subset of the tips, handed over as the polytomy calls take their lists (device-free: host/list_tree.hpp holds the check, the walk,
// the view plan and the sides of a branch, host/place_tree.hpp the rule of insertion alone, the first-minimum rule and the growth of
// the lists).  All its directed views come from ONE k_poly_views launch
// (Engine::polytomy_views, all views); k_place_costs (place.hip) then joins the two views of every branch on the way into LDS and
// counts, per query, the sites that share no state with the query tip's own vector.
//
// Stateless towards the engine's own tree exactly as the polytomy calls are: its topology stays, its vectors are marked stale, a
// tracker books nothing.
//
// The weighted (-cost) engine, under the option "place_weighted" (default 0: refused as before): the same lists, the same check,
// the same one view launch (k_poly_snk_views writes every view with its min-plus transform), then k_place_costs over the min-plus algebra: the FULL
// length of the completed tree evaluated at the new taxon's edge, the taxon the transformed side (parstree.cpp:439-541 with the
// leaf swap at :449-457).  There is no additive backbone length: *tree_length (the backbone at root_taxon, k_snk_evaluate as
// mpf_polytomy_parsimony forms it) is reported next to the costs, not added to them.
#include <string>

#include "../csrc/place.hpp"
#include "place_tree.hpp"
#include "ufboot_common.hpp"

namespace mpf {

int Engine::place_costs(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, int n_query, const int32_t *query_taxa,
                        std::vector<NniBranch> &br, std::vector<uint32_t> *delta, std::vector<PlaceBest> *best, uint32_t *tree_length)
{
  const int n = n_;
  if (sankoff_ && !place_weighted_) {
    set_error("taxon insertion: not served on the weighted (-cost) engine (its cost is a min-plus product rooted at the branch)");
    return MPF_E_UNSUPPORTED;
  }
  PolyTree &t = poly_tree_;
  listtree::Shape &w = t.shape;                        // checked once, here: polytomy_views takes it as it is
  std::string err;
  const int verdict = placetree::check(n, n_inner, first, nbr, root_taxon, w, err);
  if (verdict) { set_error(err); return verdict == placetree::PT_UNSUPPORTED ? MPF_E_UNSUPPORTED : MPF_E_INVALID; }
  if (n_query < 0 || (n_query && !query_taxa)) { set_error("taxon insertion: bad query list"); return MPF_E_INVALID; }
  {
    std::vector<char> seen((size_t)n + 1, 0);
    for (int q = 0; q < n_query; q++) {
      const int u = query_taxa[q];
      if (u < 1 || u > n) { set_error("taxon insertion: query taxon out of range"); return MPF_E_INVALID; }
      if (w.tip_nb[(size_t)u]) { set_error("taxon insertion: query taxon " + std::to_string(u) + " is in the backbone"); return MPF_E_INVALID; }
      if (seen[(size_t)u]) { set_error("taxon insertion: query taxon " + std::to_string(u) + " is listed twice"); return MPF_E_INVALID; }
      seen[(size_t)u] = 1;
    }
  }
  int rc = polytomy_views(n_inner, first, nbr, root_taxon, true, t, true);
  if (rc) return rc;
  listtree::branches(t.shape, br);
  const size_t nb = br.size(), Q = (delta || best) ? (size_t)n_query : 0, rows = (size_t)t.plan.n_rows;      // (nothing wanted: the checks, the branches, the length)
  if (delta) delta->assign(Q * nb, 0u);
  if (best) best->assign(Q, PlaceBest{0u, 0u});
  HIPCHK(h_br_desc_.reserve(nb));
  HIPCHK(d_br_desc_.reserve(nb));
  if (!listtree::branch_sides(n, n_inner, first, nbr, t.shape, t.plan, h_br_desc_.p)) { set_error("taxon insertion: inconsistent walk"); return MPF_E_STATE; }
  HIPCHK(hipMemcpyAsync(d_br_desc_.p, h_br_desc_.p, nb * sizeof(BranchDesc), hipMemcpyHostToDevice, st_));
  // pinned: [query slots Q | the root edge's op (weighted engine)]
  static_assert(sizeof(EvOp) == 4 * sizeof(uint32_t), "the op rides behind the query slots");
  HIPCHK(h_place_q_.reserve(Q + 4));
  if (sankoff_) {
    // the backbone at its root leaf, the rest of the tree the parent side (Engine::polytomy_parsimony); the op goes up from pinned
    // memory, so the copy is queued behind the view launch and the host does not wait for it here
    const EvOp op{t.plan.up_slot[(size_t)t.shape.tip_nb[(size_t)root_taxon]], (uint32_t)(root_taxon - 1), 0, 0};
    std::memcpy(h_place_q_.p + Q, &op, sizeof(op));
    HIPCHK(d_evops_.reserve(1));
    HIPCHK(reserve_results(1));
    HIPCHK(hipMemcpyAsync(d_evops_.p, h_place_q_.p + Q, sizeof(op), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemsetAsync(d_out(), 0, clear_words(1) * sizeof(uint32_t), st_));
    HIPCHK(launch_evaluate(st_, g_, vec_rows(), d_evops_.p, 1, d_out()));
    HIPCHK(hipMemcpyAsync(h_out(), d_out(), sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  } else {
    HIPCHK(d_poly_cnt_.reserve(rows));
    HIPCHK(h_poly_cnt_.reserve(rows));
    HIPCHK(launch_poly_rowsum(st_, g_, d_poly_masks_.p, (int)rows, d_poly_cnt_.p));
    HIPCHK(hipMemcpyAsync(h_poly_cnt_.p, d_poly_cnt_.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  }
  if (Q) {
    // device: [query slots | delta Q x nb | best 2 Q]
    const size_t o_best = Q * nb, out_words = o_best + 2 * Q;
    HIPCHK(d_place_q_.reserve(Q));
    HIPCHK(d_place_out_.reserve(out_words));
    HIPCHK(h_place_out_.reserve(delta ? out_words : 2 * Q));
    for (size_t q = 0; q < Q; q++) h_place_q_.p[q] = (uint32_t)(query_taxa[q] - 1);
    HIPCHK(hipMemcpyAsync(d_place_q_.p, h_place_q_.p, Q * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    if (timing_) HIPCHK(hipEventRecord(ev2_, st_));
    place_shape_ = place_pick((int)Q, (int)nb, place_tile_, sankoff_ ? place_snk_narrow_below(g_.S, g_.snk16 != 0) : place_narrow_below());
    if (sankoff_)
      HIPCHK(launch_snk_place_costs(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_place_q_.p, (int)Q, d_place_out_.p, (int)nb, place_tile_, force_big_ != 0));
    else HIPCHK(launch_place_costs(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_place_q_.p, (int)Q, d_place_out_.p, (int)nb, place_tile_));
    if (best) HIPCHK(launch_place_best(st_, d_place_out_.p, (int)nb, (int)Q, (int)nb, d_place_out_.p + o_best));
    if (timing_) HIPCHK(hipEventRecord(ev3_, st_));
    place_launches_++;
    if (delta) HIPCHK(hipMemcpyAsync(h_place_out_.p, d_place_out_.p, (best ? out_words : o_best) * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    else HIPCHK(hipMemcpyAsync(h_place_out_.p, d_place_out_.p + o_best, 2 * Q * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  }
  HIPCHK(hipStreamSynchronize(st_));
  polytomy_view_time();
  float ms = 0.f;
  if (Q && timing_ && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) place_kernel_ns_ += (uint64_t)((double)ms * 1e6);
  uint32_t len = 0;
  if (sankoff_) len = h_out()[0];
  else for (size_t i = 0; i < rows; i++) len += h_poly_cnt_.p[i];
  if (tree_length) *tree_length = len;
  if (Q && delta) std::copy(h_place_out_.p, h_place_out_.p + Q * nb, delta->begin());
  if (Q && best) {
    const uint32_t *hb = h_place_out_.p + (delta ? Q * nb : 0);
    for (size_t q = 0; q < Q; q++) {
      if (hb[2 * q + 1] >= nb) { set_error("taxon insertion: the device reported no best branch"); return MPF_E_STATE; }
      (*best)[q] = PlaceBest{hb[2 * q], hb[2 * q + 1]};
    }
  }
  return MPF_OK;
}

void place_shuffle_order(int n, uint64_t *state, int32_t *order) { placetree::shuffle_order(n, *state, order); }

int Engine::parsimony_tree(const int32_t *order, std::vector<int32_t> &first, std::vector<int32_t> &nbr, uint32_t *length_per_step)
{
  const int n = n_;
  if (n < 3) { set_error("parsimony tree: fewer than three taxa"); return MPF_E_INVALID; }
  {
    std::vector<char> seen((size_t)n + 1, 0);
    for (int i = 0; i < n; i++) {
      if (order[i] < 1 || order[i] > n || seen[(size_t)order[i]]) { set_error("parsimony tree: order[] is no permutation of 1 .. n_taxa"); return MPF_E_INVALID; }
      seen[(size_t)order[i]] = 1;
    }
  }
  if (sankoff_ && !place_weighted_) {
    set_error("taxon insertion: not served on the weighted (-cost) engine (its cost is a min-plus product rooted at the branch)");
    return MPF_E_UNSUPPORTED;
  }
  placetree::star(order, first, nbr);
  std::vector<NniBranch> br;
  std::vector<PlaceBest> best;
  uint32_t len = 0;
  for (int k = 3; k < n; k++) {
    // addTaxonMPFast from the root leaf order[0] on the tree of the first k taxa (all views made again, as the reference clears them)
    const int32_t q = order[k];
    int rc = place_costs((int)first.size() - 1, first.data(), nbr.data(), order[0], 1, &q, br, nullptr, &best, &len);
    if (rc) return rc;
    const NniBranch at = br[(size_t)best[0].branch];
    if (k == 3 && length_per_step) length_per_step[0] = len;
    if (!placetree::insert_tip(n, first, nbr, q, at.node1, at.node2)) { set_error("parsimony tree: inconsistent lists"); return MPF_E_STATE; }
    // Fitch: the backbone's length plus the added steps; weighted: addTaxonMPFast's score is the full length at the new taxon's edge
    len = sankoff_ ? best[0].delta : len + best[0].delta;
    if (length_per_step) length_per_step[k - 2] = len;
  }
  if (n == 3) {
    // the star alone: its length from an empty placement
    int rc = place_costs(1, first.data(), nbr.data(), order[0], 0, nullptr, br, nullptr, nullptr, &len);
    if (rc) return rc;
    if (length_per_step) length_per_step[0] = len;
  }
  return MPF_OK;
}

}  // namespace mpf
