// nni.cpp -- mpboot's NNI hill climb (-nni_pars, and the ratchet's first climb under -hclimb1_nni): IQTree::optimizeNNI
// (reference iqtree.cpp:2173-2302) as it runs in MP mode with the defaults there (Fitch, nni5 off, leastSquareNNI off, speednni on).
//
// Scoring one NNI needs the four directional vectors around its branch and nothing else, so every branch a step scores goes into
// ONE k_nni_eval launch (both moves of every branch) and one copy back.  What stays on the host is what is sequential in the
// reference: which branches a step scores (evalNNIs, :3144-3159, or the speednni set updateBrans2Eval builds, :2304-2311), the
// order of the positive moves (libstdc++ std::sort of plusNNIs with NNIMove::operator<, phylotree.h:225), the greedy choice of
// non-conflicting moves (genNonconfNNIs, :3020-3035), the swaps (doNNI, phylotree.cpp:3715-3742) and the rollback.
#include <algorithm>
#include <map>
#include <string>

#include "ufboot_common.hpp"

namespace mpf {

int Engine::nni_check(int root_taxon) const
{
  // the weighted climb (ParsTree scoring, no rollback: iqtree.cpp:2258) is served under the option "nni_weighted" only; an attached
  // tracker would have to book every NNI (saveCurrentTree from getBestNNIForBran, phylotree.cpp:3937): the plain entries refuse it
  if (sankoff_ && !nni_weighted_) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }
  if (ufb_) { set_error("NNI climb: not served with a UFBoot tracker attached"); return MPF_E_UNSUPPORTED; }
  return nni_check_tree(root_taxon);
}

// ... the part every NNI entry shares, whatever it makes of a tracker
int Engine::nni_check_tree(int root_taxon) const
{
  if (sankoff_ && !nni_weighted_) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }
  if (!have_tree_) { set_error("no tree set"); return MPF_E_STATE; }
  if (root_taxon < 1 || root_taxon > n_) { set_error("NNI climb: root_taxon must be in 1 .. n_taxa"); return MPF_E_INVALID; }
  return MPF_OK;
}

// evalNNIs() (iqtree.cpp:3144-3159): pre-order DFS from the root tip, neighbours in slot order; branch (node, dad) when both are inner
void Engine::nni_full_order(int root_taxon, std::vector<NniBranch> &br) const
{
  struct F { int node, dad; };
  std::vector<F> st{F{root_taxon, 0}};
  while (!st.empty()) {
    const F f = st.back();
    st.pop_back();
    if (f.node > n_ && f.dad > n_) br.push_back(NniBranch{f.node, f.dad});
    for (int s = (f.node > n_ ? 2 : 0); s >= 0; s--) {
      const int nb = num(back_[3 * f.node + s]);
      if (nb != f.dad) st.push_back(F{nb, f.node});
    }
  }
}

// getBestNNIForBran for every branch (phylotree.cpp:3807-3980): a = node1's first neighbour other than node2 in slot order, b the
// other, c0 / c1 node2's two in slot order; move k swaps a with c_k.  len[2i + k] = length of the tree after move k of branch i,
// moves[2i + k] = that swap
int Engine::nni_eval(const std::vector<NniBranch> &br, std::vector<uint32_t> &len, std::vector<NniSwap> *moves, bool masks)
{
  if (!views_valid_) { int rc = update_views(); if (rc) return rc; }
  const size_t nb = br.size();
  len.assign(2 * nb, 0u);
  if (moves) moves->assign(2 * nb, NniSwap{0, 0, 0, 0});
  const bool snk_rows = sankoff_ && masks;         // (the current tree's row is made even when no branch is scored)
  if (!nb && !snk_rows) return MPF_OK;
  HIPCHK(h_nni_desc_.reserve(std::max<size_t>(nb, 1)));
  HIPCHK(d_nni_desc_.reserve(std::max<size_t>(nb, 1)));
  HIPCHK(h_nni_out_.reserve(std::max<size_t>(nb, 1)));
  HIPCHK(d_nni_out_.reserve(std::max<size_t>(nb, 1)));
  std::vector<uint32_t> base(nb);
  auto score = [&](int r) { return tip(r) ? 0u : sc_[r]; };
  for (size_t i = 0; i < nb; i++) {
    const int v1 = br[i].node1, v2 = br[i].node2;
    int s1[2], s2[2], k1 = 0, k2 = 0;
    for (int s = 0; s < 3; s++) {
      if (num(back_[3 * v1 + s]) != v2 && k1 < 2) s1[k1++] = s;
      if (num(back_[3 * v2 + s]) != v1 && k2 < 2) s2[k2++] = s;
    }
    if (k1 != 2 || k2 != 2 || v1 <= n_ || v2 <= n_) { set_error("NNI climb: a scored branch is not an inner branch"); return MPF_E_STATE; }
    const int ra = back_[3 * v1 + s1[0]], rb = back_[3 * v1 + s1[1]], rc0 = back_[3 * v2 + s2[0]], rc1 = back_[3 * v2 + s2[1]];
    h_nni_desc_.p[i] = NniDesc{slot(ra), slot(rb), slot(rc0), slot(rc1)};
    base[i] = sankoff_ ? 0u : score(ra) + score(rb) + score(rc0) + score(rc1);      // weighted: the kernel returns full lengths
    if (moves) {
      (*moves)[2 * i] = NniSwap{v1, s1[0], v2, s2[0]};
      (*moves)[2 * i + 1] = NniSwap{v1, s1[0], v2, s2[1]};
    }
  }
  const auto [vw, wm] = tile_shape(nni_vw_);
  if (nb) {
    HIPCHK(hipMemcpyAsync(d_nni_desc_.p, h_nni_desc_.p, nb * sizeof(NniDesc), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemsetAsync(d_nni_out_.p, 0, nb * sizeof(unsigned long long), st_));
  }
  if (snk_rows) {
    if (!nni_weighted_tracked_) { set_error("NNI climb: the tracked climb is not served on the weighted engine"); return MPF_E_UNSUPPORTED; }
    HIPCHK(d_nni_vals_.reserve((2 * nb + 1) * (size_t)g_.Wp));
    HIPCHK(d_nni_vmax_.reserve(4));
    HIPCHK(h_nni_vmax_.reserve(4));
    HIPCHK(hipMemsetAsync(d_nni_vmax_.p, 0, sizeof(uint32_t), st_));
  }
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  if (snk_rows) {
    // tracked climb: the same lengths, and the rows _pattern_pars holds when each tree is booked (k_snk_nni_eval_vals)
    HIPCHK(launch_snk_nni_eval(st_, g_, vec_rows(), d_nni_desc_.p, (int)nb, d_nni_out_.p, force_big_ != 0, d_nni_vals_.p, d_nni_vmax_.p));
  } else if (sankoff_) {
    // ParsTree::computeParsimonyBranch(node1->findNeighbor(node2), node1) for both moves of every branch (k_snk_nni_eval)
    HIPCHK(launch_snk_nni_eval(st_, g_, vec_rows(), d_nni_desc_.p, (int)nb, d_nni_out_.p, force_big_ != 0));
  } else if (masks) {
    // tracked climb: the two bit planes of (h, c_0, c_1) per branch, each padded to the product's row tile
    const size_t rows_p = (size_t)round_up((int)(3 * nb), kUfbRowTile);
    HIPCHK(d_nni_planes_.reserve(2 * rows_p * (size_t)g_.Wp));
    // (the padding rows are multiplied along with the others when a product takes every row: zero, as ufb_current_tree_reps keeps its own)
    for (int bp = 0; bp < 2 && rows_p > 3 * nb; bp++)
      HIPCHK(hipMemsetAsync(d_nni_planes_.p + ((size_t)bp * rows_p + 3 * nb) * (size_t)g_.Wp, 0, (rows_p - 3 * nb) * (size_t)g_.Wp * sizeof(uint32_t), st_));
    HIPCHK(launch_nni_eval_masks(st_, g_, wm ? vec_base() : vec_rows(), d_nni_desc_.p, (int)nb, d_nni_out_.p, vw, wm, d_nni_planes_.p, d_nni_planes_.p + rows_p * (size_t)g_.Wp));
  } else
    HIPCHK(launch_nni_eval(st_, g_, wm ? vec_base() : vec_rows(), d_nni_desc_.p, (int)nb, d_nni_out_.p, vw, wm));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  if (snk_rows) {
    // row 2 nb: the current tree at the root leaf's edge, the rest of the tree the parent -- what ParsTree::computeParsimony() wrote
    // (parstree.cpp:101-116) and the row whose weighted sum is tree_length() under the caller's StartGuard
    HIPCHK(launch_sankoff_pattern(st_, g_, vec_rows(), slot(back_[start_]), slot(start_), d_nni_vals_.p + 2 * nb * (size_t)g_.Wp, d_nni_vmax_.p));
    HIPCHK(hipMemcpyAsync(h_nni_vmax_.p, d_nni_vmax_.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  }
  if (nb) HIPCHK(hipMemcpyAsync(h_nni_out_.p, d_nni_out_.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  float ms = 0.f;
  if (timing_ && hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) nni_kernel_ns_ += (uint64_t)((double)ms * 1e6);
  for (size_t i = 0; i < nb; i++) {
    const unsigned long long o = h_nni_out_.p[i];
    len[2 * i] = base[i] + (uint32_t)(o & 0xFFFFFFFFull);
    len[2 * i + 1] = base[i] + (uint32_t)(o >> 32);
  }
  if (nb) nni_launches_++;
  nni_branches_ += nb;
  return MPF_OK;
}

// doNNI: the two neighbours trade slots, their back links follow.  The vectors that change are those whose subtree holds node1 or
// node2; the device copy of the topology (kids[]) changes at the records of the end nodes and of the two subtree roots.
void Engine::nni_swap(const NniSwap &m)
{
  const int p = 3 * m.node1 + m.slot1, q = 3 * m.node2 + m.slot2;
  const int rp = back_[p], rq = back_[q];
  hookup(p, rq);
  hookup(q, rp);
  invalidate_node(m.node1);
  invalidate_node(m.node2);
  invalidate_node(num(rp));
  invalidate_node(num(rq));
  nni_log_.push_back(m);
}

int Engine::nni_scores(int root_taxon, std::vector<NniBranch> &br, std::vector<uint32_t> &len)
{
  int rc = nni_check(root_taxon);
  if (rc) return rc;
  br.clear();
  nni_full_order(root_taxon, br);
  return nni_eval(br, len, nullptr);
}

int Engine::optimize_nni(int root_taxon, bool speednni, int max_steps, uint32_t *score, int32_t *nni_count, int32_t *nni_steps)
{
  int rc = nni_check(root_taxon);
  if (rc) return rc;
  return nni_climb(root_taxon, speednni, max_steps, false, score, nni_count, nni_steps);
}

// tracked: every tree the climb looks at goes to saveCurrentTree (nni_book_step)
int Engine::nni_climb(int root_taxon, bool speednni, int max_steps, bool tracked, uint32_t *score, int32_t *nni_count, int32_t *nni_steps)
{
  int rc;
  if (max_steps < 0) { set_error("NNI climb: max_steps must be >= 0"); return MPF_E_INVALID; }
  nni_log_.clear();
  // weighted: curScore is ParsTree::computeParsimony(), the length at the edge of IQ-TREE's root leaf (parstree.cpp:101-116) --
  // with a matrix that is not symmetric the length depends on that edge
  StartGuard at_root(*this, sankoff_ ? root_taxon : 0);
  uint32_t cur = 0;
  rc = tree_length(&cur);
  if (rc) return rc;
  // brans2Eval: std::map<string, Branch> keyed by the two IQ-TREE ids written one behind the other (Branch::getKey, node.h:311-337);
  // a later branch with the same key is not inserted
  std::map<std::string, NniBranch> brans;
  auto add = [&](int x, int y) {
    const int lo = std::min(x, y), hi = std::max(x, y);
    brans.emplace(std::to_string(lo - 1) + std::to_string(hi - 1), NniBranch{lo, hi});
  };
  // MTree::getInBranches (mtree.cpp:816-827)
  auto in_branches = [&](auto &self, int depth, int node, int dad) -> void {
    if (depth == 0) return;
    for (int s = 0; s < 3; s++) {
      const int nb = num(back_[3 * node + s]);
      if (nb == dad || nb <= n_) continue;
      add(node, nb);
      self(self, depth - 1, nb, node);
    }
  };
  std::vector<NniScored> chosen, plus;
  std::vector<NniBranch> br;
  std::vector<uint32_t> len;
  std::vector<NniSwap> mv;
  bool rollback = false;
  int count = 0, num_nnis = 0, step;
  for (step = 1; step <= max_steps; step++) {
    const uint32_t old = cur;
    if (!rollback) {
      br.clear();
      if (speednni && !brans.empty()) for (const auto &kv : brans) br.push_back(kv.second);
      else nni_full_order(root_taxon, br);
      rc = nni_eval(br, len, &mv, tracked);
      if (rc) return rc;
      if (tracked) { rc = sankoff_ ? nni_book_step_snk(br, len, mv, cur) : nni_book_step(br, len, mv, cur); if (rc) return rc; }
      plus.clear();
      for (size_t i = 0; i < br.size(); i++) {
        const int k = len[2 * i] < len[2 * i + 1] ? 0 : 1;               // :3971-3975
        if (len[2 * i + k] < cur) plus.push_back(NniScored{mv[2 * i + k], len[2 * i + k]});
      }
      std::sort(plus.begin(), plus.end(), [](const NniScored &a, const NniScored &b) { return a.len < b.len; });
      if (plus.empty()) break;
      chosen.clear();
      for (const NniScored &m : plus) {
        bool ok = true;
        for (const NniScored &c : chosen)
          if (m.mv.node1 == c.mv.node1 || m.mv.node2 == c.mv.node1 || m.mv.node1 == c.mv.node2 || m.mv.node2 == c.mv.node2) { ok = false; break; }
        if (ok) chosen.push_back(m);
      }
      num_nnis = (int)chosen.size();
    }
    for (int i = 0; i < num_nnis; i++) nni_swap(chosen[(size_t)i].mv);
    if (speednni) {
      brans.clear();
      for (int i = 0; i < num_nnis; i++) {
        const NniSwap &m = chosen[(size_t)i].mv;
        add(m.node1, m.node2);
        in_branches(in_branches, 2, m.node1, m.node2);
        in_branches(in_branches, 2, m.node2, m.node1);
      }
    }
    rc = tree_length(&cur);
    if (rc) return rc;
    if (tracked) ufb_->rt_valid = false;         // several non-conflicting NNIs are not additive per site: R_T is made again from the tree
    if (cur <= chosen[0].len) {
      count += num_nnis;
      rollback = false;
    } else if (sankoff_) {
      // iqtree.cpp:2258, `if(globalParam->sankoff_cost_file) continue;`: no rollback under -cost -- the moves stay, curScore stays
      // the worse length, nni_count does not grow, and the next step scores the speednni set just built from these moves
      nni_kept_worse_++;
    } else {
      for (int i = 0; i < num_nnis; i++) nni_swap(chosen[(size_t)i].mv);
      rollback = true;
      num_nnis = 1;
      cur = old;
      nni_rollbacks_++;
    }
  }
  if (score) *score = cur;
  if (nni_count) *nni_count = count;
  if (nni_steps) *nni_steps = step;
  return MPF_OK;
}

// one full evaluation by the mask-writing kernel, its rows read back per pattern: terms[(3 i + r) * P + p] = how many of the three
// joins at branch i have no common state at pattern p -- r = 0 in the current tree (h), r = 1 / 2 after move 0 / 1 (c_0, c_1); 0
// for a pattern the engine drops
int Engine::nni_pattern_terms(int root_taxon, std::vector<NniBranch> &br, std::vector<uint32_t> &len, std::vector<uint8_t> &terms)
{
  if (sankoff_) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }   // (the mask rows are Fitch joins)
  int rc = nni_check_tree(root_taxon);
  if (rc) return rc;
  br.clear();
  nni_full_order(root_taxon, br);
  rc = nni_eval(br, len, nullptr, true);
  if (rc) return rc;
  const size_t nb = br.size(), Wp = (size_t)g_.Wp, rows_p = (size_t)round_up((int)(3 * nb), kUfbRowTile);
  terms.assign(3 * nb * (size_t)P_, 0);
  if (!nb) return MPF_OK;
  std::vector<uint32_t> h(2 * rows_p * Wp);
  HIPCHK(hipMemcpy(h.data(), d_nni_planes_.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < 3 * nb; r++)
    for (int p = 0; p < P_; p++) {
      const int site = first_site_[(size_t)p];
      if (site < 0 || (size_t)site >= 32 * Wp) continue;      // (weight 0 behind the last site of a full row: k_pattern_sum)
      const size_t w = r * Wp + (size_t)(site >> 5);
      terms[r * (size_t)P_ + (size_t)p] = (uint8_t)(((h[w] >> (site & 31)) & 1u) + 2u * ((h[rows_p * Wp + w] >> (site & 31)) & 1u));
    }
  return MPF_OK;
}

// the weighted counterpart: one full evaluation by k_snk_nni_eval_vals, its rows read back per pattern
int Engine::nni_pattern_lengths(int root_taxon, std::vector<NniBranch> &br, std::vector<uint32_t> &len, std::vector<uint16_t> &rows)
{
  if (!sankoff_) { set_error("NNI pattern lengths: weighted engines only (a Fitch engine has mpf_nni_pattern_terms)"); return MPF_E_UNSUPPORTED; }
  if (!nni_weighted_ || !nni_weighted_tracked_) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }
  int rc = nni_check_tree(root_taxon);
  if (rc) return rc;
  StartGuard at_root(*this, root_taxon);           // (the current tree's row is the one at this leaf's edge)
  br.clear();
  nni_full_order(root_taxon, br);
  rc = nni_eval(br, len, nullptr, true);
  if (rc) return rc;
  const size_t nb = br.size(), Wp = (size_t)g_.Wp;
  rows.assign((1 + 2 * nb) * (size_t)P_, 0);
  std::vector<uint16_t> h((2 * nb + 1) * Wp);
  HIPCHK(hipMemcpy(h.data(), d_nni_vals_.p, h.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
  for (int p = 0; p < P_; p++) {
    const int j = first_site_[(size_t)p];          // (weighted engine: the pattern's place among the kept ones)
    if (j < 0) continue;
    rows[(size_t)p] = h[2 * nb * Wp + (size_t)j];
    for (size_t c = 0; c < 2 * nb; c++) rows[(1 + c) * (size_t)P_ + (size_t)p] = h[c * Wp + (size_t)j];
  }
  return MPF_OK;
}

// ---- what the two booking steps share: the replay of one step's 1 + 2 nb trees in the reference's order (as in spr_sweeps_ufboot)
struct Engine::NniReplay {
  Engine &e;
  UfbState &u;
  const std::vector<NniSwap> &mv;
  std::vector<int32_t> bk;
  std::string cand_key;
  const UfbDeferCtx dctx{};

  NniReplay(Engine &eng, const std::vector<NniSwap> &moves) : e(eng), u(*eng.ufb_), mv(moves) {}
  // the tree after candidate c's swap
  void swapped(uint32_t c, std::vector<int32_t> &t) const
  {
    t = e.back_;
    const NniSwap &m = mv[c];
    const int p = 3 * m.node1 + m.slot1, q = 3 * m.node2 + m.slot2, rp = t[(size_t)p], rq = t[(size_t)q];
    t[(size_t)p] = rq; t[(size_t)rq] = p;
    t[(size_t)q] = rp; t[(size_t)rp] = q;
  }
  const std::string &topology_key(uint32_t cand_code)
  {
    if (cand_code == 0xFFFFFFFFu) {
      if (u.self_key_epoch != (uint64_t)e.topo_epoch_) { e.canonical_topology(e.back_, u.self_key); u.self_key_epoch = (uint64_t)e.topo_epoch_; }
      return u.self_key;
    }
    swapped(cand_code, bk);
    e.canonical_topology(bk, cand_key);
    return cand_key;
  }
  int64_t lookup_topology(int64_t tree_index, uint32_t cand_code)
  {
    u.lookups++;
    return u.topo_index.emplace(topology_key(cand_code), tree_index).first->second;
  }
  // the current tree under self_len, every sample offered R_T (u.h_rt) on the host; merged (a sample-sharded tracker): R_T lives in
  // pieces on the ranks -- the offers are the events of index 0 the ranks have exchanged
  void book_self(uint32_t self_len, bool pass, const std::vector<UfbEvent> *merged = nullptr)
  {
    u.cur_logl_now = -(int32_t)self_len;
    int64_t tree_index = e.ufb_book_tree(self_len, pass, 0xFFFFFFFFu, u.store_trees, [&](uint32_t cc) -> const std::string & { return topology_key(cc); });
    if (tree_index < 0) return;
    bool looked_up = u.store_trees;                // (-storetrees: tree_str is set at the top, no lookup per sample)
    if (merged) {
      for (size_t ep = 0; ep < merged->size() && (*merged)[ep].idx == 0u; ep++)
        e.ufb_one_event((*merged)[ep].b, (*merged)[ep].s, tree_index, looked_up, 0xFFFFFFFFu,
                        [&](int64_t ti, uint32_t cc) { return lookup_topology(ti, cc); }, dctx);
      return;
    }
    for (int c2 = 0; c2 < u.Bl; c2++)
      e.ufb_one_event((uint32_t)u.ids[(size_t)c2], (uint32_t)u.h_rt.p[c2], tree_index, looked_up, 0xFFFFFFFFu,
                      [&](int64_t ti, uint32_t cc) { return lookup_topology(ti, cc); }, dctx);
  }
  // the candidates in evaluation order, move 0 then move 1 (candidate c has output index 1 + c); then the trees some sample took
  void book_candidates(const std::vector<uint32_t> &blen, const std::vector<uint8_t> &pass, const std::vector<UfbEvent> &events)
  {
    size_t ep = 0;
    for (uint32_t c = 0; c < (uint32_t)blen.size(); c++) {
      u.cur_logl_now = -(int32_t)blen[c];
      int64_t tree_index = e.ufb_book_tree(blen[c], pass[c] != 0, c, u.store_trees, [&](uint32_t cc) -> const std::string & { return topology_key(cc); });
      if (tree_index < 0) continue;
      const uint32_t idx = 1u + c;
      while (ep < events.size() && events[ep].idx < idx) ep++;
      bool looked_up = u.store_trees;
      for (; ep < events.size() && events[ep].idx == idx; ep++)
        e.ufb_one_event(events[ep].b, events[ep].s, tree_index, looked_up, c, [&](int64_t ti, uint32_t cc) { return lookup_topology(ti, cc); }, dctx);
    }
    // a tree a sample accepted is remembered as (this step's tree, swap) and materialised only if still referenced
    for (const UfbState::Pending &pe : u.pending) {
      if (u.refs[(size_t)pe.tree_index] <= 0 || u.store.count(pe.tree_index)) continue;
      if (pe.cand == 0xFFFFFFFFu) u.store.emplace(pe.tree_index, e.back_);
      else { swapped(pe.cand, bk); u.store.emplace(pe.tree_index, bk); }
      u.stored++;
    }
    u.pending.clear();
  }
};

// (One step's event extraction, nni_extract_events, is in ufboot_common.hpp: the tracked TBR sweep, host/tbr.cpp, runs it too.)

// A sample-sharded tracker: the product and the extraction ran over this rank's columns, R_T (u.h_rt) holds its samples only.  ONE
// exchange per scoring step: the step's local events and, as index 0, the current tree's score under every local sample; every rank
// then replays the union in (candidate, sample) order, so books and draws stay identical everywhere.  Tags 0x40000000 + step: the
// scan batches of an SPR climb count from 0, and the exchanges keep 31 bits of a tag.
int Engine::nni_exchange_events(uint32_t n_idx, std::vector<UfbEvent> &events)
{
  UfbState &u = *ufb_;
  for (int c2 = 0; c2 < u.Bl; c2++) events.push_back(UfbEvent{0u, (uint32_t)u.ids[(size_t)c2], (uint32_t)u.h_rt.p[c2]});
  int rc = ufb_gather_events(events, 0x40000000u | (u.nni_tag++ & 0x3FFFFFFFu), "tracked NNI climb");
  if (rc) return rc;
  std::vector<UfbEvent> tmp;
  std::vector<uint32_t> count;
  sort_events(events, tmp, count, n_idx, (uint32_t)u.B);
  return MPF_OK;
}

// ---------------------------------------------------------------- the climb under -bb
//
// With save_all_trees == 2 a scoring step of optimizeNNI hands 1 + 2 * branches trees to IQTree::saveCurrentTree, in this order:
// the current tree (iqtree.cpp:2181-2183), then move 0 and move 1 of every evaluated branch (getBestNNIForBran,
// phylotree.cpp:3907-3939) -- all of them, not only the positive ones; a rollback step, the applied moves and the rollback
// itself book nothing.  pllComputePatternParsimony is skipped on this path (iqtree.cpp:3363): _pattern_pars is the booked tree's
// own row (computeParsimonyBranch has just written it, phylotree.cpp:956-957 / :986-987), so on a ratchet climb the length the
// cut-off test sees and treels_logl records is the booked tree's OWN length on the original alignment (:3283-3294), and a tree
// that fails the cut-off closes no gate.
//
// k_nni_eval_masks has left per branch the rows h, c_0, c_1 (two bit planes each).  REPS of all candidates in one product,
// C = plane0 x W + 2 * plane1 x W; candidate (branch i, move k) scores R_T[b] - C[h_i][b] + C[c_ik][b] under sample b.  Index
// space of the extraction: 0 = the current tree (offered from R_T on the host), 1 + 2 i + k = the candidates in evaluation
// order, 1 + 2 nb + i = the home slot of branch i (its h row); the events are replayed with the tracker's update rule and the
// shared tie stream exactly as the SPR climb's are (ufb_one_event, ufb_book_tree).  Under a cut-off only the rows of candidates
// that pass are multiplied (rowsel); a ratchet climb multiplies every row, since the column of original frequencies is what
// gives each candidate the length the cut-off test looks at.
int Engine::nni_book_step(const std::vector<NniBranch> &br, const std::vector<uint32_t> &len, const std::vector<NniSwap> &mv, uint32_t cur)
{
  UfbState &u = *ufb_;
  const uint32_t nb = (uint32_t)br.size(), n_idx = 1u + 3u * nb;
  const bool ratchet = u.ratchet;
  const int oc = u.Bl;                             // the column of the original pattern frequencies
  const size_t Wp = (size_t)g_.Wp;
  u.nni_booked += 1u + 2u * (uint64_t)nb;
  u.batches++;
  const UfbCutoff cut = ufb_cutoff(u.logl_cutoff);     // iqtree.cpp:3343: booked iff  -len > logl_cutoff - 1e-4
  // -storetrees (iqtree.cpp:3302-3341): a topology met before is counted, and booked again when its length improved, whatever the
  // cut-off says -- no step is skipped, every row is multiplied, every candidate takes part in the extraction and the replay decides
  const bool store_trees = u.store_trees, sharded = u.exchange != nullptr;
  if (cut.none_pass && !store_trees) return MPF_OK;
  const double t0 = now_ms();
  if (!u.rt_valid) { int rc = ufb_current_tree_reps(); if (rc) return rc; }       // (uses C: in front of the product)
  UCHK(u.h_rt.reserve((size_t)u.Bp));
  UCHK(hipMemcpyAsync(u.h_rt.p, u.rt.p, (size_t)(u.Bl + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  const int mask_rows_p = round_up((int)(3u * nb), kUfbRowTile);
  const uint32_t *plane[2] = {d_nni_planes_.p, d_nni_planes_.p + (size_t)mask_rows_p * Wp};
  auto product = [&](int rows_p, const uint32_t *d_sel) -> int {      // C = plane 0 x W + 2 * plane 1 x W, its rows counted once
    UCHK(u.C.reserve((size_t)rows_p * (size_t)u.Bp));
    int rc = ufb_mask_product(plane[0], rows_p, u.C.p, kUfbOverwrite, d_sel);
    return rc ? rc : ufb_mask_product(plane[1], rows_p, u.C.p, kUfbAccumulate | kUfbUncounted, d_sel, nullptr, 1);
  };
  std::vector<uint32_t> blen(2 * (size_t)nb);      // the length each candidate is booked under
  bool have_C = false;
  if (ratchet && nb) {
    int rc = product(mask_rows_p, nullptr);
    if (rc) return rc;
    have_C = true;
    UCHK(u.d_col.reserve((size_t)mask_rows_p));
    UCHK(u.h_col.reserve((size_t)mask_rows_p));
    UCHK(launch_ufb_column(st_, u.C.p, u.Bp, oc, 3u * nb, u.d_col.p));
    UCHK(hipMemcpyAsync(u.h_col.p, u.d_col.p, (size_t)(3u * nb) * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  }
  UCHK(hipStreamSynchronize(st_));
  u.rt_orig = (uint32_t)u.h_rt.p[oc];
  for (uint32_t i = 0; i < nb; i++)
    for (uint32_t k = 0; k < 2; k++)
      blen[2 * i + k] = ratchet ? (uint32_t)((int64_t)u.rt_orig - (int64_t)u.h_col.p[3 * i] + (int64_t)u.h_col.p[3 * i + 1 + k]) : len[2 * i + k];
  NniReplay replay(*this, mv);

  // ---- the current tree: its own length (ratchet: its length on the original alignment), every sample from R_T
  const uint32_t self_len = ratchet ? u.rt_orig : cur;
  const bool self_pass = cut.passes(self_len);
  if (!sharded) replay.book_self(self_len, self_pass);

  // ---- the candidates that pass: product (unless a ratchet step has it), extraction
  std::vector<uint8_t> pass(2 * (size_t)nb), take(2 * (size_t)nb);       // pass: the cut-off test; take: part of the extraction
  uint32_t n_pass = 0;
  for (size_t c = 0; c < pass.size(); c++) { pass[c] = cut.passes(blen[c]); take[c] = store_trees || pass[c]; n_pass += take[c]; }
  std::vector<UfbEvent> events;
  if (n_pass) {
    const bool compact = cut.have_cut && !ratchet && !store_trees;
    std::vector<uint32_t> sel_rows, home(nb), part((size_t)n_idx, 0xFFFFFFFFu);
    std::vector<uint32_t> crow((size_t)n_idx, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < nb; i++) {
      home[i] = 1u + 2u * nb + i;
      part[1 + 2 * i] = part[2 + 2 * i] = i;
      if (!take[2 * i] && !take[2 * i + 1]) continue;
      if (!compact) {
        crow[1 + 2 * i] = 3 * i + 1; crow[2 + 2 * i] = 3 * i + 2; crow[1 + 2 * nb + i] = 3 * i;
        continue;
      }
      crow[1 + 2 * nb + i] = (uint32_t)sel_rows.size(); sel_rows.push_back(3 * i);
      for (uint32_t k = 0; k < 2; k++)
        if (take[2 * i + k]) { crow[1 + 2 * i + k] = (uint32_t)sel_rows.size(); sel_rows.push_back(3 * i + 1 + k); }
    }
    const int rows_p = compact ? round_up((int)sel_rows.size(), kUfbRowTile) : mask_rows_p;
    int rc = nni_extract_events(n_idx, home, part, crow, take, compact ? &sel_rows : nullptr, rows_p, have_C, product, events);
    if (rc) return rc;
  }
  if (sharded) {
    // (the bounds the extraction ran under are those in front of the current tree's own booking: more events at most, each of
    //  which the rule looks at again)
    int rc = nni_exchange_events(n_idx, events);
    if (rc) return rc;
    replay.book_self(self_len, self_pass, &events);
  }
  const double t1 = now_ms();
  u.t_dev += t1 - t0;
  replay.book_candidates(blen, pass, events);
  u.t_replay += now_ms() - t1;
  return MPF_OK;
}

// ---------------------------------------------------------------- ... on the weighted engine (-cost m -nni_pars -bb)
//
// The same 1 + 2 nb trees in the same order; no rollback steps (iqtree.cpp:2258), so a kept-worse step is followed by an ordinary
// scoring step that books the current tree under the longer curScore.  _pattern_pars of a candidate is the row of per-pattern minima
// ParsTree::computeParsimonyBranch has just written (parstree.cpp:460-461, :482-529), of the current tree the row
// ParsTree::computeParsimony() wrote at the root leaf's edge (:101-116): nni_eval has left them as rows 2 i + k and 2 nb of
// d_nni_vals_, 16 bits per pattern.  The chain is spr_sweeps_ufboot_snk's: K = bits of the largest value, k_vals_planes, K runs of
// k_bitgemm per weight plane.  A tree's score under sample b is its OWN product row -- R_T is the current tree's row (launch_colsum
// of one row) and the home row of every candidate, so that R_T - C[home] + C[c] = C[c]; there is no ufb_current_tree_reps pass and no
// join mask.  Output indices: 0 = the current tree, 1 + c = candidate c, 1 + 2 nb = the one home slot.
int Engine::nni_book_step_snk(const std::vector<NniBranch> &br, const std::vector<uint32_t> &len, const std::vector<NniSwap> &mv, uint32_t cur)
{
  UfbState &u = *ufb_;
  const uint32_t nb = (uint32_t)br.size(), n_idx = 2u + 2u * nb, R = 2u * nb;       // R: the current tree's row of vals
  const bool ratchet = u.ratchet;
  const int oc = u.Bl;
  u.nni_booked += 1u + 2u * (uint64_t)nb;
  u.batches++;
  const UfbCutoff cut = ufb_cutoff(u.logl_cutoff);     // iqtree.cpp:3343
  const bool store_trees = u.store_trees, sharded = u.exchange != nullptr;      // (-storetrees: as in nni_book_step)
  if (cut.none_pass && !store_trees) return MPF_OK;
  std::vector<uint32_t> blen(len.begin(), len.begin() + 2 * (size_t)nb);
  std::vector<uint8_t> pass(2 * (size_t)nb), take(2 * (size_t)nb, 1);
  uint32_t n_pass = 0;
  if (!ratchet) {
    for (size_t c = 0; c < pass.size(); c++) { pass[c] = cut.passes(blen[c]); n_pass += pass[c]; }
    if (!store_trees && !n_pass && !cut.passes(cur)) return MPF_OK;    // nothing of this step is booked: nothing to multiply
  }
  const double t0 = now_ms();
  // ---- K from vmax (nni_eval has waited for it), the bit planes of all 2 nb + 1 rows
  const uint32_t rows = 2u * nb + 1u;
  UfbPlanes P;
  { int rc = ufb_vals_planes(d_nni_vals_.p, rows, h_nni_vmax_.p[0], P); if (rc) return rc; }
  const int plane_rows_p = P.rows_p;
  uint32_t cur_row = R;                            // the current tree's row of C
  bool timed = false;
  auto product = [&](int rows_p, const uint32_t *d_sel) -> int {
    timed = timing_;
    { int rc = ufb_weighted_product(P, rows_p, d_sel, cur_row); if (rc) return rc; }       // (R_T = the current tree's own row; ev2_ .. ev3_)
    UCHK(u.h_rt.reserve((size_t)u.Bp));
    UCHK(hipMemcpyAsync(u.h_rt.p, u.rt.p, (size_t)(u.Bl + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
    return MPF_OK;
  };
  bool have_C = false;
  uint32_t self_len = cur;
  if (ratchet) {
    // every row: the column of original frequencies gives each tree the length it is booked under (iqtree.cpp:3283-3294)
    int rc = product(plane_rows_p, nullptr);
    if (rc) return rc;
    have_C = true;
    UCHK(u.d_col.reserve((size_t)plane_rows_p));
    UCHK(u.h_col.reserve((size_t)plane_rows_p));
    UCHK(launch_ufb_column(st_, u.C.p, u.Bp, oc, rows, u.d_col.p));
    UCHK(hipMemcpyAsync(u.h_col.p, u.d_col.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
    UCHK(hipStreamSynchronize(st_));
    u.rt_orig = self_len = (uint32_t)u.h_col.p[R];
    for (size_t c = 0; c < pass.size(); c++) { blen[c] = (uint32_t)u.h_col.p[c]; pass[c] = cut.passes(blen[c]); n_pass += pass[c]; }
  }
  if (!store_trees) take = pass;
  // ---- product of the rows that are booked (unless a ratchet step has it), extraction
  const bool compact = cut.have_cut && !ratchet && !store_trees;
  std::vector<uint32_t> sel_rows, home(1, 1u + 2u * nb), part((size_t)n_idx, 0xFFFFFFFFu), crow((size_t)n_idx, 0xFFFFFFFFu);
  for (uint32_t c = 0; c < 2 * nb; c++) {
    part[1 + c] = 0u;
    if (!compact) crow[1 + c] = c;
    else if (take[c]) { crow[1 + c] = (uint32_t)sel_rows.size(); sel_rows.push_back(c); }
  }
  if (compact) { cur_row = (uint32_t)sel_rows.size(); sel_rows.push_back(R); }
  crow[1 + 2 * nb] = cur_row;
  const int rows_p = compact ? round_up((int)sel_rows.size(), kUfbRowTile) : plane_rows_p;
  std::vector<UfbEvent> events;
  int rc = nni_extract_events(n_idx, home, part, crow, take, compact ? &sel_rows : nullptr, rows_p, have_C, product, events);
  if (rc) return rc;
  if (sharded) { rc = nni_exchange_events(n_idx, events); if (rc) return rc; }
  if (!ratchet) u.rt_orig = (uint32_t)u.h_rt.p[oc];
  float ms = 0.f;
  if (timed && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) u.gemm_ms += ms;
  const double t1 = now_ms();
  u.t_dev += t1 - t0;
  // ---- host replay: the current tree (every sample from R_T), then the candidates
  NniReplay replay(*this, mv);
  replay.book_self(self_len, cut.passes(self_len), sharded ? &events : nullptr);
  replay.book_candidates(blen, pass, events);
  u.t_replay += now_ms() - t1;
  return MPF_OK;
}

// IQTree::optimizeNNI under -bb (iqtree.cpp:2173-2302 with save_all_trees == 2)
int Engine::ufboot_optimize_nni(int root_taxon, bool speednni, int max_steps, uint32_t *score, int32_t *nni_count, int32_t *nni_steps)
{
  if (sankoff_ && !(nni_weighted_ && nni_weighted_tracked_)) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }
  if (!ufb_) { set_error("no UFBoot tracker attached"); return MPF_E_STATE; }
  if (!have_tree_) { set_error("no tree set"); return MPF_E_STATE; }
  const UfbState &u = *ufb_;
  // option "nni_tracked_rules": the three optional rules and a sample-sharded tracker are served (nni_book_step); 0: refused as ever
  const bool rules = nni_tracked_rules_ != 0;
  if ((u.exchange || u.Bl != u.B) && !(rules && u.exchange)) { set_error("tracked NNI climb: not served with a sample-sharded tracker"); return MPF_E_UNSUPPORTED; }
  if (u.store_trees && !rules) { set_error("tracked NNI climb: -storetrees is not served"); return MPF_E_UNSUPPORTED; }
  if (u.topboot && !rules) { set_error("tracked NNI climb: -mulhits -topboot is not served"); return MPF_E_UNSUPPORTED; }
  if (u.distinct && !rules) { set_error("tracked NNI climb: -distinct_iter_top_boot is not served"); return MPF_E_UNSUPPORTED; }
  if (root_taxon < 1 || root_taxon > n_) { set_error("NNI climb: root_taxon must be in 1 .. n_taxa"); return MPF_E_INVALID; }
  // (suspended: other weights than the attach-time ones under -no_hclimb1_bb, or an attach-time pattern without a site --
  //  saveCurrentTree is not called, iqtree.cpp:3280: the plain climb)
  const bool tracked = !u.suspended;
  if (tracked) ufb_->rt_valid = false;
  ufb_->nni_tag = 0;
  const int rc = nni_climb(root_taxon, speednni, max_steps, tracked, score, nni_count, nni_steps);
  ufb_->rt_valid = false;
  // closing handshake, as the SPR climb has one: a rank that took another path would be in the middle of a step here
  if (rc == MPF_OK && tracked) return ufb_close_exchange(0xFFFFFFFEu, "tracked NNI climb: ranks out of step at the end of the climb");
  return rc;
}

}  // namespace mpf
