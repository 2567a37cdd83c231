// brlen.cpp -- parsimony branch lengths: PhyloTree::fixNegativeBranch (reference phylotree.cpp:3597-3633), which an MP run calls on
// every tree it hands on (phyloanalysis.cpp:1153, :1180, :1336, :1501, :2280).  Per tree the reference calls
// computeParsimonyBranch(.., &branch_subst) once for each of the 2n - 3 branches, each call on the scalar computePartialParsimony in
// both directions.
//
// The engine keeps both directional vectors of every edge, so one branch's count is a join of vec[r] and vec[back[r]] and all
// branches are ONE launch (k_branch_subst; k_snk_branch_eval on the weighted engine) and one copy back.  What stays on the host is
// the walk that fixes the branch order and, in capi.cpp, the length formula (:3608-3614).
#include <string>

#include "ufboot_common.hpp"

namespace mpf {

// fixNegativeBranch(force, node = root, dad = NULL): FOR_NEIGHBOR_IT(node, dad, it) { the branch node--(*it)->node; recurse }, i.e. a
// pre-order walk from the root leaf, neighbours in slot order, every branch met once from its root side -- the order of evalNNIs
// (nni_full_order) with the pendant branches included.  node1 = the end nearer the root leaf
void Engine::branch_order(int root_taxon, std::vector<NniBranch> &br) const
{
  struct F { int node, dad; };
  std::vector<F> st{F{root_taxon, 0}};
  while (!st.empty()) {
    const F f = st.back();
    st.pop_back();
    if (f.dad) br.push_back(NniBranch{f.dad, f.node});
    for (int s = (f.node > n_ ? 2 : 0); s >= 0; s--) {
      const int nb = num(back_[3 * f.node + s]);
      if (nb != f.dad) st.push_back(F{nb, f.node});
    }
  }
}

int Engine::branch_substitutions(int root_taxon, std::vector<NniBranch> &br, std::vector<uint32_t> &subst)
{
  if (!have_tree_) { set_error("no tree set"); return MPF_E_STATE; }
  if (ntips_ != n_) { set_error("branch substitutions: the tree is not complete"); return MPF_E_STATE; }
  if (root_taxon < 1 || root_taxon > n_) { set_error("branch substitutions: root_taxon must be in 1 .. n_taxa"); return MPF_E_INVALID; }
  // both directions of every edge: only what is stale is made again
  if (!views_valid_) { int rc = update_views(); if (rc) return rc; }
  br.clear();
  branch_order(root_taxon, br);
  const size_t nb = br.size();
  subst.assign(nb, 0u);
  if (!nb) return MPF_OK;
  HIPCHK(h_br_desc_.reserve(nb));
  HIPCHK(d_br_desc_.reserve(nb));
  HIPCHK(h_br_out_.reserve(nb));
  HIPCHK(d_br_out_.reserve(nb));
  for (size_t i = 0; i < nb; i++) {
    const int v1 = br[i].node1, v2 = br[i].node2;
    int r1 = -1;
    for (int s = 0; s < (v1 > n_ ? 3 : 1); s++)
      if (num(back_[3 * v1 + s]) == v2) r1 = 3 * v1 + s;
    if (r1 < 0) { set_error("branch substitutions: inconsistent tree"); return MPF_E_STATE; }
    const int r2 = back_[r1];
    // vec[r1] = the rest of the tree seen from node2, vec[r2] = the subtree at node2 (a leaf: its own vector).  Weighted engine,
    // ParsTree::computeParsimonyBranch((*it), node) (parstree.cpp:439-541): dad_branch = the subtree at node2 enters as it is,
    // node_branch = the rest of the tree is the transformed side; a leaf node2 swaps the two (:449-457)
    if (sankoff_ && v2 <= n_) h_br_desc_.p[i] = BranchDesc{slot(r1), slot(r2)};
    else h_br_desc_.p[i] = BranchDesc{slot(r2), slot(r1)};
  }
  const auto [vw, wm] = tile_shape(brlen_vw_);
  HIPCHK(hipMemcpyAsync(d_br_desc_.p, h_br_desc_.p, nb * sizeof(BranchDesc), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(d_br_out_.p, 0, nb * sizeof(uint32_t), st_));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  if (sankoff_) HIPCHK(launch_snk_branch_eval(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, force_big_ != 0));
  else HIPCHK(launch_branch_subst(st_, g_, wm ? vec_base() : vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, vw, wm));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  HIPCHK(hipMemcpyAsync(h_br_out_.p, d_br_out_.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  float ms = 0.f;
  if (timing_ && hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) brlen_kernel_ns_ += (uint64_t)((double)ms * 1e6);
  std::copy(h_br_out_.p, h_br_out_.p + nb, subst.begin());
  brlen_launches_++;
  return MPF_OK;
}

}  // namespace mpf
