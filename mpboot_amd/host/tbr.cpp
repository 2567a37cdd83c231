// tbr.cpp -- the TBR (tree bisection and reconnection) neighbourhood of the engine's tree: one visit's matrix, the best of every
// visit of a sweep, the edit, and a steepest-descent climb.
//
// There is no reference function: MPBoot 1.1.1 has SPR and NNI only.  What coincides with it: row 0 and column 0 of a visit's matrix
// are the insertion tests of rearrangeParsimony (sprparsimony.cpp:2259-2376, testInsertParsimony :2106-2188 on the branches
// addTraverseParsimony :2208-2218 reaches), and the edit is two removeNodeParsimony + insertParsimony steps.
//
// Everything that follows from back[] alone is in tbr_plan.hpp (the lists, the chain programs, the chunks, the tiles, the edit).
// Here: the views are brought up to date (all of them stay resident), k_tbr_roots writes the root sets of a chunk of visits into a
// scratch store, k_tbr_costs forms every visit's matrix from a flat tile list, k_tbr_best leaves three words per visit.  A sweep's
// root sets run to several GB at full size, so it goes chunk by chunk; the result does not depend on the chunking.
//
// The weighted (-cost) engine, under the option "tbr_weighted" (default 0: refused as before): the same lists, chunks and tiles; the
// root sets are sums of stored min-plus transforms (k_tbr_snk_roots), an entry is the FULL length of the joined tree (no base), a
// vector is S rows of We elements (patterns, or pairs of patterns in the 16-bit store).  Symmetric cost matrices only: with any
// other the length depends on the evaluation edge, and TBR has no reference function that would fix one.
//
// Under -bb (a UFBoot tracker attached): ufboot_tbr_sweep / ufboot_optimize_tbr book every entry of every visit through the tracker
// (tbr_book_chunk, k_tbr_masks; "under -bb" below); the default rule, -mulhits, a cut-off, -cutoff_from_btrees.  The weighted
// engine serves them under the option "tbr_weighted_tracked" (with "tbr_weighted"; default 0: refused as before) through
// tbr_book_chunk_snk and k_tbr_snk_vals ("... on the weighted engine" below).
//
// Not served: a cost matrix that is not symmetric, the plain entries with a UFBoot tracker attached (nothing would be booked), the
// tracked ones on the weighted engine without its option, under -storetrees, -mulhits -topboot, -distinct_iter_top_boot, on a sample-sharded tracker or
// in a ratchet state; random ties, a device-resident climb.
#include <functional>
#include <string>

#include "ufboot_common.hpp"
#include "../csrc/tbr.hpp"

namespace mpf {

struct TbrBuffers {
  DevBuf<uint32_t> store, deep, out, best;
  DevBuf<tbrplan::Op> ops;
  DevBuf<TbrSide> sides;
  DevBuf<TbrVisit> visits;
  DevBuf<tbrplan::Item> items[2];                  // narrow | wide
  PinBuf<uint32_t> h_best, h_out;
  // under a tracker (tbr_book_chunk) and for tbr_pattern_terms: the mask rows of a batch and the lists k_tbr_masks walks
  DevBuf<uint32_t> masks;
  DevBuf<tbrplan::MaskRun> mruns;
  DevBuf<tbrplan::MaskCol> mcols;
  // ... on the weighted engine (tbr_book_chunk_snk, tbr_pattern_lengths): the 16-bit rows of a batch and their largest value
  DevBuf<uint16_t> vals;
  DevBuf<uint32_t> vmax;
  PinBuf<uint32_t> h_vmax;
  std::vector<tbrplan::Op> v_ops;
  std::vector<TbrSide> v_sides;
  std::vector<TbrVisit> v_visits;
  std::vector<tbrplan::Item> v_items[2];
};

int Engine::tbr_check(const char *what, int maxtrav, bool tracked)
{
  if (sankoff_ && !tbr_weighted_) {
    set_error(std::string(what) + ": TBR is not served on the weighted (-cost) engine (its cost is a min-plus product rooted at the new edge)");
    return MPF_E_UNSUPPORTED;
  }
  if (sankoff_ && g_.costT) {
    set_error(std::string(what) + ": TBR is not served with a cost matrix that is not symmetric (the length depends on the evaluation edge)");
    return MPF_E_UNSUPPORTED;
  }
  if (ufb_ && !tracked) {
    set_error(std::string(what) + ": TBR is not served with a UFBoot tracker attached (nothing would be booked)");
    return MPF_E_UNSUPPORTED;
  }
  if (!have_tree_) { set_error("no tree set"); return MPF_E_STATE; }
  if (ntips_ != n_) { set_error(std::string(what) + ": the tree is not complete"); return MPF_E_STATE; }
  if (maxtrav < 1 || maxtrav > 255) { set_error(std::string(what) + ": maxtrav must be in 1 .. 255"); return MPF_E_INVALID; }
  return MPF_OK;
}

// the matrices of the visits recs[0 .. count): vis = their lists; matrix (one visit only) = its costs; best = per visit the first
// minimum behind [0][0]; n_pairs = entries scored
int Engine::tbr_run(const int32_t *recs, size_t count, int maxtrav, std::vector<tbrplan::Visit> &vis, std::vector<uint32_t> *matrix,
                    std::vector<TbrBest> *best, uint64_t *n_pairs, const TbrChunkFn *chunk_fn)
{
  if (!views_valid_ || pending_scores_) { int rc = update_views(); if (rc) return rc; }
  if (!tbr_buf_) tbr_buf_ = std::make_shared<TbrBuffers>();
  TbrBuffers &b = *tbr_buf_;
  const int n = n_, S = g_.S, LD = tbr_lds_levels(S);
  const int32_t *back = back_.data();
  vis.resize(count);
  std::vector<size_t> need(count), entries(count);
  uint64_t pairs = 0;
  for (size_t i = 0; i < count; i++) {
    tbrplan::visit(n, back, recs[i], maxtrav, vis[i]);
    need[i] = vis[i].vectors();
    entries[i] = vis[i].rows() * vis[i].cols();
    pairs += entries[i];
  }
  if (n_pairs) *n_pairs = pairs;
  if (best) best->assign(count, TbrBest{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu});
  const bool weighted = sankoff_ != 0;
  const size_t vec_words = (size_t)S * (size_t)tbr_row_words(g_);      // (weighted: S rows of We elements)
  const size_t cap = tbr_chunk_vectors_ > 0 ? (size_t)tbr_chunk_vectors_ : std::max<size_t>(1, ((size_t)256 << 20) / (vec_words * sizeof(uint32_t)));
  const auto chunks = tbrplan::chunks(need, cap, entries);
  tbr_chunks_ = (int)chunks.size();
  tbrplan::Side scratch_side;
  for (const auto &ch : chunks) {
    const size_t nv = ch.second - ch.first;
    b.v_ops.clear();
    b.v_sides.clear();
    b.v_visits.clear();
    b.v_items[0].clear();
    b.v_items[1].clear();
    size_t nvec = 0, at = 0;
    for (size_t k = 0; k < nv; k++) {
      const tbrplan::Visit &v = vis[ch.first + k];
      const size_t f0 = nvec, g0 = nvec + v.F.rec.size();
      const int xs[2] = {v.q, v.p};
      for (int side = 0; side < 2; side++) {
        const uint32_t op_begin = (uint32_t)b.v_ops.size();
        tbrplan::side(n, back, xs[side], maxtrav, scratch_side, &b.v_ops, (uint32_t)nvec);
        nvec += scratch_side.rec.size();
        if (b.v_ops.size() > op_begin)
          b.v_sides.push_back(TbrSide{op_begin, (uint32_t)b.v_ops.size(), (uint32_t)std::max(0, scratch_side.max_depth + 1 - LD),
                                      weighted && side == 1 ? 1u : 0u /* a side of G is stored transformed */, 0ull});
      }
      if (nvec != g0 + v.G.rec.size()) { set_error("TBR: inconsistent plan"); return MPF_E_STATE; }
      // (weighted: an entry is the full length of the joined tree, nothing to add)
      const uint32_t base = weighted ? 0u : (tip(v.p) ? 0u : sc_[v.p]) + (tip(v.q) ? 0u : sc_[v.q]);
      b.v_visits.push_back(TbrVisit{slot(v.q), slot(v.p), (uint32_t)f0, (uint32_t)g0, (uint32_t)v.rows(), (uint32_t)v.cols(), base, 0u, (uint64_t)at});
      at += v.rows() * v.cols();
      const int shape = tbrplan::pick(S, v.rows(), v.cols(), tbr_tile_, weighted);
      tbrplan::tiles((uint32_t)k, v.rows(), v.cols(), tbrplan::tile_dims(S, shape, weighted), b.v_items[shape == tbrplan::TILE_NARROW ? 0 : 1]);
    }
    if (nvec > 0xFFFFFFFFull) { set_error("TBR: a chunk of more than 2^32 root sets"); return MPF_E_UNSUPPORTED; }
    const size_t deep_words = tbr_deep_words(g_, b.v_sides.data(), b.v_sides.size());
    HIPCHK(b.store.reserve(std::max<size_t>(1, nvec * vec_words)));
    HIPCHK(b.deep.reserve(std::max<size_t>(1, deep_words)));
    HIPCHK(b.out.reserve(at));
    HIPCHK(b.best.reserve(3 * nv));
    HIPCHK(b.ops.reserve(std::max<size_t>(1, b.v_ops.size())));
    HIPCHK(b.sides.reserve(std::max<size_t>(1, b.v_sides.size())));
    HIPCHK(b.visits.reserve(nv));
    HIPCHK(b.h_best.reserve(3 * nv));
    if (matrix || chunk_fn) HIPCHK(b.h_out.reserve(std::max<size_t>(1, at)));
    if (!b.v_ops.empty()) HIPCHK(hipMemcpyAsync(b.ops.p, b.v_ops.data(), b.v_ops.size() * sizeof(tbrplan::Op), hipMemcpyHostToDevice, st_));
    if (!b.v_sides.empty()) HIPCHK(hipMemcpyAsync(b.sides.p, b.v_sides.data(), b.v_sides.size() * sizeof(TbrSide), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemcpyAsync(b.visits.p, b.v_visits.data(), nv * sizeof(TbrVisit), hipMemcpyHostToDevice, st_));
    for (int s = 0; s < 2; s++) {
      if (b.v_items[s].empty()) continue;
      HIPCHK(b.items[s].reserve(b.v_items[s].size()));
      HIPCHK(hipMemcpyAsync(b.items[s].p, b.v_items[s].data(), b.v_items[s].size() * sizeof(tbrplan::Item), hipMemcpyHostToDevice, st_));
    }
    const uint32_t *vec = vec_rows();
    if (timing_) HIPCHK(hipEventRecord(ev2_, st_));
    HIPCHK(launch_tbr_roots(st_, g_, vec, b.ops.p, b.sides.p, b.v_sides.size(), b.store.p, b.deep.p));
    for (int s = 0; s < 2; s++) {
      if (b.v_items[s].empty()) continue;
      HIPCHK(launch_tbr_costs(st_, g_, vec, b.store.p, b.visits.p, b.items[s].p, b.v_items[s].size(), s == 0 ? tbrplan::TILE_NARROW : tbrplan::TILE_WIDE,
                              b.out.p));
      tbr_launches_++;
    }
    // (a 1 x 1 matrix has no tile: its only entry, the tree as it is, is never read by k_tbr_best; a scan hands it over from `base`)
    HIPCHK(launch_tbr_best(st_, b.visits.p, nv, b.out.p, b.best.p));
    if (timing_) HIPCHK(hipEventRecord(ev3_, st_));
    HIPCHK(hipMemcpyAsync(b.h_best.p, b.best.p, 3 * nv * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    if ((matrix || chunk_fn) && at > 1) HIPCHK(hipMemcpyAsync(b.h_out.p, b.out.p, at * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    float ms = 0.f;
    if (timing_ && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) tbr_kernel_ns_ += (uint64_t)((double)ms * 1e6);
    if (best)
      for (size_t k = 0; k < nv; k++) (*best)[ch.first + k] = TbrBest{b.h_best.p[3 * k], b.h_best.p[3 * k + 1], b.h_best.p[3 * k + 2]};
    // (the root sets of the chunk and its visit records still stand on the device)
    if (chunk_fn) { int rc = (*chunk_fn)(ch.first, nv, b.h_out.p); if (rc) return rc; }
    if (matrix) {
      if (at > 1) matrix->assign(b.h_out.p, b.h_out.p + at);
      else {
        // the tree as it is: both parts' own lengths plus the sites the two views of the edge do not share (weighted: the length at the
        // start edge, which with a symmetric matrix is the length at any edge)
        uint32_t len = 0;
        int rc = tree_length(&len);
        if (rc) return rc;
        matrix->assign(1, len);
      }
    }
  }
  return MPF_OK;
}

int Engine::tbr_scan(int rec, int maxtrav, std::vector<int32_t> &f, std::vector<int32_t> &g, std::vector<uint32_t> *cost)
{
  int rc = tbr_check("mpf_tbr_scan", maxtrav);
  if (rc) return rc;
  if (rec < 3 || rec >= 3 * (2 * n_ - 1) || back_[rec] < 0) { set_error("mpf_tbr_scan: bad record"); return MPF_E_INVALID; }
  std::vector<tbrplan::Visit> vis;
  if (cost) {
    const int32_t r = rec;
    rc = tbr_run(&r, 1, maxtrav, vis, cost, nullptr, nullptr);
    if (rc) return rc;
  } else {
    vis.resize(1);
    tbrplan::visit(n_, back_.data(), rec, maxtrav, vis[0]);
  }
  f = vis[0].F.rec;
  g = vis[0].G.rec;
  return MPF_OK;
}

int Engine::tbr_sweep_best(int maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs)
{
  int rc = tbr_check("mpf_tbr_sweep_best", maxtrav);
  if (rc) return rc;
  node_rectifier();
  std::vector<tbrplan::Visit> vis;
  std::vector<TbrBest> best;
  const size_t count = 2 * (size_t)n_ - 2;
  rc = tbr_run(nodep_.data() + 1, count, maxtrav, vis, nullptr, &best, n_pairs);
  if (rc) return rc;
  for (size_t i = 0; i < count; i++) {
    const TbrBest &t = best[i];
    const tbrplan::Visit &v = vis[i];
    if (v.rows() * v.cols() <= 1) { best_cost[i] = 0xFFFFFFFFu; best_f[i] = best_g[i] = -1; continue; }
    if (t.row >= v.rows() || t.col >= v.cols()) { set_error("TBR: the device reported no best pair"); return MPF_E_STATE; }
    best_cost[i] = t.cost;
    best_f[i] = t.row ? v.F.rec[t.row - 1] : -1;
    best_g[i] = t.col ? v.G.rec[t.col - 1] : -1;
  }
  return MPF_OK;
}

int Engine::apply_tbr(int rec, int f_rec, int g_rec, uint32_t *score)
{
  int rc = tbr_check("mpf_apply_tbr", 255);
  if (rc) return rc;
  return tbr_edit(rec, f_rec, g_rec, score);
}

int Engine::tbr_edit(int rec, int f_rec, int g_rec, uint32_t *score)
{
  int rc;
  if (rec < 3 || rec >= 3 * (2 * n_ - 1) || back_[rec] < 0) { set_error("mpf_apply_tbr: bad record"); return MPF_E_INVALID; }
  tbrplan::Visit v;
  tbrplan::visit(n_, back_.data(), rec, 255, v);
  if ((f_rec != -1 && std::find(v.F.rec.begin(), v.F.rec.end(), f_rec) == v.F.rec.end()) ||
      (g_rec != -1 && std::find(v.G.rec.begin(), v.G.rec.end(), g_rec) == v.G.rec.end())) {
    set_error("mpf_apply_tbr: the pair is not in the visit's lists");
    return MPF_E_INVALID;
  }
  std::vector<int32_t> bk(back_.begin(), back_.begin() + 3 * (size_t)(2 * n_ - 1));
  tbrplan::apply(bk.data(), rec, f_rec, g_rec);
  rc = set_tree(bk.data());
  if (rc) return rc;
  uint32_t len = 0;
  rc = score_tree(&len);
  if (rc) return rc;
  if (score) *score = len;
  return MPF_OK;
}

int Engine::optimize_tbr(int maxtrav, int max_moves, uint32_t *score, int32_t *n_moves)
{
  int rc = tbr_check("mpf_optimize_tbr", maxtrav);
  if (rc) return rc;
  return tbr_climb(maxtrav, max_moves, false, score, n_moves);
}

// tracked: every sweep's entries go to saveCurrentTree's rule (tbr_book_chunk), the last sweep, which finds nothing, included; the
// climb itself draws nothing
int Engine::tbr_climb(int maxtrav, int max_moves, bool tracked, uint32_t *score, int32_t *n_moves)
{
  int rc;
  tbr_moves_.clear();
  const size_t count = 2 * (size_t)n_ - 2;
  std::vector<tbrplan::Visit> vis;
  std::vector<TbrBest> best;
  uint32_t len = 0;
  rc = score_tree(&len);
  if (rc) return rc;
  for (;;) {
    if (max_moves > 0 && (int)tbr_moves_.size() >= max_moves) break;
    node_rectifier();
    const TbrChunkFn book = [&](size_t first, size_t nv, const uint32_t *cost) { return tbr_book_chunk(vis.data() + first, nv, cost, len); };
    rc = tbr_run(nodep_.data() + 1, count, maxtrav, vis, nullptr, &best, nullptr, tracked ? &book : nullptr);
    if (rc) return rc;
    size_t at = count;
    for (size_t i = 0; i < count; i++)
      if (vis[i].rows() * vis[i].cols() > 1 && (at == count || best[i].cost < best[at].cost)) at = i;      // (the lowest visit among equals)
    if (at == count || best[at].cost >= len) break;
    const tbrplan::Visit &v = vis[at];
    const TbrBest t = best[at];
    if (t.row >= v.rows() || t.col >= v.cols()) { set_error("TBR: the device reported no best pair"); return MPF_E_STATE; }
    const TbrMove mv{v.p, t.row ? v.F.rec[t.row - 1] : -1, t.col ? v.G.rec[t.col - 1] : -1, t.cost};
    uint32_t got = 0;
    rc = tbr_edit(mv.rec, mv.f_rec, mv.g_rec, &got);
    if (rc) return rc;
    if (tracked) ufb_->rt_valid = false;             // R_T is made again from the edited tree
    if (got != mv.score) { set_error("TBR: the edited tree does not have the length its matrix entry promised"); return MPF_E_STATE; }
    tbr_moves_.push_back(mv);
    len = got;
  }
  if (score) *score = len;
  if (n_moves) *n_moves = (int32_t)tbr_moves_.size();
  return MPF_OK;
}

// ---------------------------------------------------------------- under -bb
//
// There is no reference function, so this is the definition.  A tracked sweep hands every entry of every visit's matrix to
// saveCurrentTree's rule: the visits in sweep order (node_order()), a visit's entries in row-major order from [0][0].  [0][0] is the
// current tree under its own length -- rearrangeParsimony opens every prune node with a booking of the current tree
// (sprparsimony.cpp:2285-2289) -- every other entry the joined tree under cost[i][j]; a 1 x 1 visit books the current tree only.
// Booking is the cut-off filter (ufb_cutoff(...).passes), a new entry of treels_logl, then the per-sample update rule with its tie
// draws from the engine's one stream, in that order.  Duplicated topologies are booked as often as they occur.
//
// Cut (p, q).  The per-site Fitch length of each part does not depend on where the part is rooted, so per site
//     pattern_pars(T_ij) = pattern_pars(T) - M[0][0] + M[i][j],   M[i][j] = "R_q(F_i) and R_p(G_j) share no state"
// the word whose popcount k_tbr_costs takes; M[0][0] joins vec[q] and vec[p]: the tree as it is.  Hence REPS(T_ij)[b] = R_T[b] -
// C[home][b] + C[(i, j)][b] with C = masks x sample weights (k_bitgemm), home the visit's [0][0] row: the event formula of the SPR
// and NNI paths.  k_tbr_masks writes the rows of the entries that pass the cut-off (the costs are known from k_tbr_costs) and one home
// row per visit that has one; the current tree's bookings are offered from R_T on the host, as the SPR loop offers its self slots.
//
// A batch is a stretch of at most "tbr_book_rows" entries of that sequence (tbrplan::book_batches), a visit too large for what is
// left of a batch goes on in the next one.  Index space of a batch's extraction (nni_extract_events): 0 = unused, 1 + c = entry c of
// the batch ([0][0] entries never take part: no events), 1 + entries + r = the home slot of run r.  The device takes the samples'
// bounds as they stand in front of the batch: a superset of the events the rule can fire on, each of which the replay looks at
// again, so books and draws do not depend on the batching.
struct Engine::TbrReplay {
  Engine &e;
  UfbState &u;
  const tbrplan::Visit *vis;
  const tbrplan::BookRun *runs;
  size_t n_runs;
  std::vector<uint32_t> first;                     // first[r] = the batch entry run r begins with
  std::vector<int32_t> bk;
  std::string cand_key;
  const UfbDeferCtx dctx{};

  TbrReplay(Engine &eng, const tbrplan::Visit *v, const tbrplan::BookRun *r, size_t n) : e(eng), u(*eng.ufb_), vis(v), runs(r), n_runs(n)
  {
    uint32_t at = 0;
    for (size_t i = 0; i < n; i++) { first.push_back(at); at += (uint32_t)(r[i].end - r[i].begin); }
  }
  // batch entry c -> (visit, row, column)
  void where(uint32_t c, const tbrplan::Visit *&v, size_t &i, size_t &j) const
  {
    const size_t r = (size_t)(std::upper_bound(first.begin(), first.end(), c) - first.begin()) - 1;
    const uint64_t en = runs[r].begin + (uint64_t)(c - first[r]);
    v = vis + runs[r].visit;
    i = (size_t)(en / v->cols());
    j = (size_t)(en % v->cols());
  }
  // the tree of batch entry c
  void joined(uint32_t c, std::vector<int32_t> &t) const
  {
    const tbrplan::Visit *v;
    size_t i, j;
    where(c, v, i, j);
    t = e.back_;
    tbrplan::apply(t.data(), v->p, i ? v->F.rec[i - 1] : -1, j ? v->G.rec[j - 1] : -1);
  }
  const std::string &topology_key(uint32_t cand_code)
  {
    if (cand_code == 0xFFFFFFFFu) {
      if (u.self_key_epoch != (uint64_t)e.topo_epoch_) { e.canonical_topology(e.back_, u.self_key); u.self_key_epoch = (uint64_t)e.topo_epoch_; }
      return u.self_key;
    }
    joined(cand_code, bk);
    e.canonical_topology(bk, cand_key);
    return cand_key;
  }
  int64_t lookup_topology(int64_t tree_index, uint32_t cand_code)
  {
    u.lookups++;
    return u.topo_index.emplace(topology_key(cand_code), tree_index).first->second;
  }
  // one tree: the filter and treels_logl, then the update rule over the samples the caller walks
  template <class Offers>
  void book(uint32_t len, bool pass, uint32_t cand_code, Offers offers)
  {
    u.cur_logl_now = -(int32_t)len;
    int64_t tree_index = e.ufb_book_tree(len, pass, cand_code, false, [&](uint32_t cc) -> const std::string & { return topology_key(cc); });
    if (tree_index < 0) return;
    bool looked_up = false;
    offers([&](uint32_t b, uint32_t s) {
      e.ufb_one_event(b, s, tree_index, looked_up, cand_code, [&](int64_t ti, uint32_t cc) { return lookup_topology(ti, cc); }, dctx);
    });
  }
  // a tree a sample accepted is remembered as (batch entry) and materialised only if still referenced at the end of the batch
  void flush()
  {
    for (const UfbState::Pending &pe : u.pending) {
      if (u.refs[(size_t)pe.tree_index] <= 0 || u.store.count(pe.tree_index)) continue;
      if (pe.cand == 0xFFFFFFFFu) u.store.emplace(pe.tree_index, e.back_);
      else { joined(pe.cand, bk); u.store.emplace(pe.tree_index, bk); }
      u.stored++;
    }
    u.pending.clear();
  }
};

int Engine::tbr_book_chunk(const tbrplan::Visit *vis, size_t nv, const uint32_t *cost, uint32_t cur_len)
{
  if (sankoff_) return tbr_book_chunk_snk(vis, nv, cost, cur_len);
  UfbState &u = *ufb_;
  TbrBuffers &b = *tbr_buf_;
  const size_t Wp = (size_t)g_.Wp;
  std::vector<size_t> entries(nv), at(nv);
  std::vector<uint32_t> ncols(nv);
  size_t total = 0;
  for (size_t k = 0; k < nv; k++) {
    at[k] = total;
    entries[k] = vis[k].rows() * vis[k].cols();
    ncols[k] = (uint32_t)vis[k].cols();
    total += entries[k];
  }
  u.tbr_booked += (uint64_t)total;
  const UfbCutoff cut = ufb_cutoff(u.logl_cutoff);     // iqtree.cpp:3343: booked iff  -len > logl_cutoff - 1e-4
  if (cut.none_pass) return MPF_OK;
  if (!u.rt_valid) { int rc = ufb_current_tree_reps(); if (rc) return rc; }
  UCHK(u.h_rt.reserve((size_t)u.Bp));
  UCHK(hipMemcpyAsync(u.h_rt.p, u.rt.p, (size_t)(u.Bl + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  UCHK(hipStreamSynchronize(st_));
  u.rt_orig = (uint32_t)u.h_rt.p[u.Bl];
  // a batch's mask rows (entries + one home row at most) and its product each within 256 MiB, the figure of the chunk cap
  const size_t row_bytes = std::max(Wp, (size_t)u.Bp) * sizeof(uint32_t);
  const size_t cap = tbr_book_rows_ > 0 ? (size_t)tbr_book_rows_
                                        : std::max<size_t>(1, (((size_t)256 << 20) / row_bytes) / (size_t)kUfbRowTile * (size_t)kUfbRowTile - 1);
  std::vector<tbrplan::BookRun> runs;
  std::vector<size_t> off;
  tbrplan::book_batches(entries, cap, runs, off);
  std::vector<tbrplan::MaskRun> mr;
  std::vector<tbrplan::MaskCol> mc;
  std::vector<uint32_t> crow_c, home_r, blen;
  std::vector<uint8_t> pass;
  std::vector<UfbEvent> events;
  const bool self_pass = cut.passes(cur_len);
  for (size_t bi = 0; bi + 1 < off.size(); bi++) {
    const tbrplan::BookRun *br = runs.data() + off[bi];
    const size_t n_runs = off[bi + 1] - off[bi];
    u.tbr_book_batches++;
    u.batches++;
    const double t0 = now_ms();
    // ---- the lengths the entries are booked under, which of them pass
    blen.clear();
    pass.clear();
    uint32_t n_take = 0;
    for (size_t r = 0; r < n_runs; r++)
      for (uint64_t en = br[r].begin; en < br[r].end; en++) {
        const bool self = en == 0;
        blen.push_back(self ? cur_len : cost[at[br[r].visit] + (size_t)en]);
        pass.push_back(self ? 0 : (uint8_t)cut.passes(blen.back()));      // (the current tree is offered from R_T on the host)
        n_take += pass.back();
      }
    const uint32_t n_c = (uint32_t)blen.size(), n_idx = 1u + n_c + (uint32_t)n_runs;
    events.clear();
    if (n_take) {
      // ---- mask rows, product, extraction
      const uint32_t rows = tbrplan::mask_rows(br, n_runs, ncols.data(), pass.data(), mr, mc, crow_c, home_r);
      const int rows_p = round_up((int)rows, kUfbRowTile);
      std::vector<uint32_t> home(n_runs), part((size_t)n_idx, 0xFFFFFFFFu), crow((size_t)n_idx, 0xFFFFFFFFu);
      uint32_t c = 0;
      for (size_t r = 0; r < n_runs; r++) {
        home[r] = 1u + n_c + (uint32_t)r;
        crow[home[r]] = home_r[r];
        for (uint64_t en = br[r].begin; en < br[r].end; en++, c++) { part[1 + c] = (uint32_t)r; crow[1 + c] = crow_c[c]; }
      }
      auto product = [&](int rp, const uint32_t *) -> int {
        UCHK(b.masks.reserve((size_t)rp * Wp));
        UCHK(b.mruns.reserve(mr.size()));
        UCHK(b.mcols.reserve(mc.size()));
        UCHK(u.C.reserve((size_t)rp * (size_t)u.Bp));
        UCHK(hipMemcpyAsync(b.mruns.p, mr.data(), mr.size() * sizeof(tbrplan::MaskRun), hipMemcpyHostToDevice, st_));
        UCHK(hipMemcpyAsync(b.mcols.p, mc.data(), mc.size() * sizeof(tbrplan::MaskCol), hipMemcpyHostToDevice, st_));
        // (the padding rows are multiplied along with the others: zero, as ufb_current_tree_reps keeps its own)
        if ((size_t)rp > rows) UCHK(hipMemsetAsync(b.masks.p + (size_t)rows * Wp, 0, ((size_t)rp - rows) * Wp * sizeof(uint32_t), st_));
        if (timing_) UCHK(hipEventRecord(ev0_, st_));
        UCHK(launch_tbr_masks(st_, g_, vec_rows(), b.store.p, b.visits.p, b.mruns.p, mr.size(), b.mcols.p, b.masks.p));
        if (timing_) UCHK(hipEventRecord(ev1_, st_));
        int rc = ufb_mask_product(b.masks.p, rp, u.C.p, kUfbOverwrite);
        if (timing_) UCHK(hipEventRecord(ev2_, st_));
        return rc;
      };
      int rc = nni_extract_events(n_idx, home, part, crow, pass, nullptr, rows_p, false, product, events);      // (waits: mr, mc outlive their copies)
      if (rc) return rc;
      if (timing_) {
        float m0 = 0.f, m1 = 0.f;
        if (hipEventElapsedTime(&m0, ev0_, ev1_) == hipSuccess && hipEventElapsedTime(&m1, ev1_, ev2_) == hipSuccess) {
          tbr_masks_ns_ += (uint64_t)((double)m0 * 1e6);
          tbr_product_ns_ += (uint64_t)((double)m1 * 1e6);
          u.gemm_ms += m1;
          tbr_extract_ns_ += (uint64_t)(std::max(0.0, now_ms() - t0 - (double)m0 - (double)m1) * 1e6);
        }
      }
    }
    const double t1 = now_ms();
    u.t_dev += t1 - t0;
    // ---- host replay, in booking order
    TbrReplay replay(*this, vis, br, n_runs);
    size_t ep = 0;
    uint32_t c = 0;
    for (size_t r = 0; r < n_runs; r++)
      for (uint64_t en = br[r].begin; en < br[r].end; en++, c++) {
        if (en == 0) {
          replay.book(cur_len, self_pass, 0xFFFFFFFFu, [&](auto offer) {
            for (int c2 = 0; c2 < u.Bl; c2++) offer((uint32_t)u.ids[(size_t)c2], (uint32_t)u.h_rt.p[c2]);
          });
          continue;
        }
        const uint32_t idx = 1u + c;
        replay.book(blen[c], pass[c] != 0, c, [&](auto offer) {
          while (ep < events.size() && events[ep].idx < idx) ep++;
          for (; ep < events.size() && events[ep].idx == idx; ep++) offer(events[ep].b, events[ep].s);
        });
      }
    replay.flush();
    u.t_replay += now_ms() - t1;
  }
  return MPF_OK;
}

// ---------------------------------------------------------------- ... on the weighted engine (-cost m -bb)
//
// The same entries in the same order under the same lengths: cost[i][j] is the full weighted length k_tbr_costs<PlaceMinPlus> returns.
// _pattern_pars of the tree of entry [i][j] is, per pattern, min_x(RF_i[x] + m(RG_j)[x]) -- the terms whose weighted sum cost[i][j]
// is --, which k_tbr_snk_vals writes as a 16-bit row per listed entry.  The chain is nni_book_step_snk's: K = bits of the largest
// value, k_vals_planes, K runs of k_bitgemm per weight plane.  A tree's score under sample b is its OWN product row: the home row of
// a run is its visit's [0][0] row, which under a symmetric matrix is the current tree's row at every cut edge, so that R_T - C[home]
// + C[c] = C[c].  No ufb_current_tree_reps pass, no join mask.  R_T itself is the product of the current tree's own row
// (launch_sankoff_pattern in tree_length's operand order), made once per sweep in front of the first batch: the current tree's
// bookings are offered from it on the host even where no candidate of a batch passes the cut-off.  Batches, pass flags, index space,
// extraction and replay are tbr_book_chunk's; the automatic batch cap is tbrplan::book_cap.
int Engine::tbr_snk_vals_check(const std::string &what)
{
  if (tbr_snk_vals_fit(g_, n_)) return MPF_OK;
  set_error(what + ": not served in the 32-bit store where a per-pattern length may exceed 16 bits (taxa x highest cost >= 65536)");
  return MPF_E_UNSUPPORTED;
}

int Engine::tbr_book_chunk_snk(const tbrplan::Visit *vis, size_t nv, const uint32_t *cost, uint32_t cur_len)
{
  UfbState &u = *ufb_;
  TbrBuffers &b = *tbr_buf_;
  const size_t npat = (size_t)g_.Wp;                 // (weighted: g_.Wp counts patterns)
  std::vector<size_t> entries(nv), at(nv);
  std::vector<uint32_t> ncols(nv);
  size_t total = 0;
  for (size_t k = 0; k < nv; k++) {
    at[k] = total;
    entries[k] = vis[k].rows() * vis[k].cols();
    ncols[k] = (uint32_t)vis[k].cols();
    total += entries[k];
  }
  u.tbr_booked += (uint64_t)total;
  const UfbCutoff cut = ufb_cutoff(u.logl_cutoff);     // iqtree.cpp:3343: booked iff  -len > logl_cutoff - 1e-4
  if (cut.none_pass) return MPF_OK;
  UCHK(b.vmax.reserve(4));
  UCHK(b.h_vmax.reserve(4));
  if (!u.rt_valid) {
    // R_T from the current tree's own row (as nni_eval fills row 2 nb); the pass is not counted among the products
    const uint64_t counted = u.gemm_rows;
    UCHK(b.vals.reserve(npat));
    UCHK(hipMemsetAsync(b.vmax.p, 0, sizeof(uint32_t), st_));
    UCHK(launch_sankoff_pattern(st_, g_, vec_rows(), slot(back_[start_]), slot(start_), b.vals.p, b.vmax.p));      // (left = far end, right = start: as tree_length)
    UCHK(hipMemcpyAsync(b.h_vmax.p, b.vmax.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    UCHK(hipStreamSynchronize(st_));
    UfbPlanes P;
    { int rc = ufb_vals_planes(b.vals.p, 1u, b.h_vmax.p[0], P); if (rc) return rc; }
    { int rc = ufb_weighted_product(P, P.rows_p, nullptr, 0u); if (rc) return rc; }
    u.gemm_rows = counted;
    u.rt_valid = true;
  }
  UCHK(u.h_rt.reserve((size_t)u.Bp));
  UCHK(hipMemcpyAsync(u.h_rt.p, u.rt.p, (size_t)(u.Bl + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  UCHK(hipStreamSynchronize(st_));
  u.rt_orig = (uint32_t)u.h_rt.p[u.Bl];
  // a batch's 16-bit rows, its K bit planes and its product each within 256 MiB (tbrplan::book_cap; K bounded by the values' bound)
  const size_t cap = tbr_book_rows_ > 0 ? (size_t)tbr_book_rows_
                                        : tbrplan::book_cap(npat, (size_t)u.Wp_s, (size_t)u.Bp, tbrplan::value_bits((uint64_t)n_ * (uint64_t)g_.highest_cost),
                                                            (size_t)kUfbRowTile);
  std::vector<tbrplan::BookRun> runs;
  std::vector<size_t> off;
  tbrplan::book_batches(entries, cap, runs, off);
  std::vector<tbrplan::MaskRun> mr;
  std::vector<tbrplan::MaskCol> mc;
  std::vector<uint32_t> crow_c, home_r, blen;
  std::vector<uint8_t> pass;
  std::vector<UfbEvent> events;
  const bool self_pass = cut.passes(cur_len);
  for (size_t bi = 0; bi + 1 < off.size(); bi++) {
    const tbrplan::BookRun *br = runs.data() + off[bi];
    const size_t n_runs = off[bi + 1] - off[bi];
    u.tbr_book_batches++;
    u.batches++;
    const double t0 = now_ms();
    // ---- the lengths the entries are booked under, which of them pass
    blen.clear();
    pass.clear();
    uint32_t n_take = 0;
    for (size_t r = 0; r < n_runs; r++)
      for (uint64_t en = br[r].begin; en < br[r].end; en++) {
        const bool self = en == 0;
        blen.push_back(self ? cur_len : cost[at[br[r].visit] + (size_t)en]);
        pass.push_back(self ? 0 : (uint8_t)cut.passes(blen.back()));      // (the current tree is offered from R_T on the host)
        n_take += pass.back();
      }
    const uint32_t n_c = (uint32_t)blen.size(), n_idx = 1u + n_c + (uint32_t)n_runs;
    events.clear();
    if (n_take) {
      // ---- 16-bit rows, bit planes, product, extraction
      const uint32_t rows = tbrplan::mask_rows(br, n_runs, ncols.data(), pass.data(), mr, mc, crow_c, home_r);
      const int rows_p = round_up((int)rows, kUfbRowTile);
      std::vector<uint32_t> home(n_runs), part((size_t)n_idx, 0xFFFFFFFFu), crow((size_t)n_idx, 0xFFFFFFFFu);
      uint32_t c = 0, rt_row = tbrplan::kNoRow;
      for (size_t r = 0; r < n_runs; r++) {
        home[r] = 1u + n_c + (uint32_t)r;
        crow[home[r]] = home_r[r];
        if (rt_row == tbrplan::kNoRow) rt_row = home_r[r];      // (any home row: every one of them is the current tree's)
        for (uint64_t en = br[r].begin; en < br[r].end; en++, c++) { part[1 + c] = (uint32_t)r; crow[1 + c] = crow_c[c]; }
      }
      bool timed = false;
      auto product = [&](int rp, const uint32_t *) -> int {
        UCHK(b.vals.reserve((size_t)rows * npat));
        UCHK(b.mruns.reserve(mr.size()));
        UCHK(b.mcols.reserve(mc.size()));
        UCHK(hipMemcpyAsync(b.mruns.p, mr.data(), mr.size() * sizeof(tbrplan::MaskRun), hipMemcpyHostToDevice, st_));
        UCHK(hipMemcpyAsync(b.mcols.p, mc.data(), mc.size() * sizeof(tbrplan::MaskCol), hipMemcpyHostToDevice, st_));
        UCHK(hipMemsetAsync(b.vmax.p, 0, sizeof(uint32_t), st_));
        if (timing_) UCHK(hipEventRecord(ev0_, st_));
        UCHK(launch_tbr_snk_vals(st_, g_, n_, vec_rows(), b.store.p, b.visits.p, b.mruns.p, mr.size(), b.mcols.p, b.vals.p, b.vmax.p));
        UCHK(hipMemcpyAsync(b.h_vmax.p, b.vmax.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        UCHK(hipStreamSynchronize(st_));               // K follows from the largest value written
        UfbPlanes P;
        { int rc = ufb_vals_planes(b.vals.p, rows, b.h_vmax.p[0], P); if (rc) return rc; }      // (the padding rows of every plane are zero)
        if (timing_) UCHK(hipEventRecord(ev1_, st_));
        timed = timing_;
        return ufb_weighted_product(P, rp, nullptr, rt_row);       // (R_T again from a home row: the values it had; ev2_ .. ev3_)
      };
      int rc = nni_extract_events(n_idx, home, part, crow, pass, nullptr, rows_p, false, product, events);      // (waits: mr, mc outlive their copies)
      if (rc) return rc;
      if (timed) {
        float m0 = 0.f, m1 = 0.f;
        if (hipEventElapsedTime(&m0, ev0_, ev1_) == hipSuccess && hipEventElapsedTime(&m1, ev2_, ev3_) == hipSuccess) {
          tbr_masks_ns_ += (uint64_t)((double)m0 * 1e6);      // (here: the vals kernel and the plane slicing)
          tbr_product_ns_ += (uint64_t)((double)m1 * 1e6);
          u.gemm_ms += m1;
          tbr_extract_ns_ += (uint64_t)(std::max(0.0, now_ms() - t0 - (double)m0 - (double)m1) * 1e6);
        }
      }
    }
    const double t1 = now_ms();
    u.t_dev += t1 - t0;
    // ---- host replay, in booking order
    TbrReplay replay(*this, vis, br, n_runs);
    size_t ep = 0;
    uint32_t c = 0;
    for (size_t r = 0; r < n_runs; r++)
      for (uint64_t en = br[r].begin; en < br[r].end; en++, c++) {
        if (en == 0) {
          replay.book(cur_len, self_pass, 0xFFFFFFFFu, [&](auto offer) {
            for (int c2 = 0; c2 < u.Bl; c2++) offer((uint32_t)u.ids[(size_t)c2], (uint32_t)u.h_rt.p[c2]);
          });
          continue;
        }
        const uint32_t idx = 1u + c;
        replay.book(blen[c], pass[c] != 0, c, [&](auto offer) {
          while (ep < events.size() && events[ep].idx < idx) ep++;
          for (; ep < events.size() && events[ep].idx == idx; ep++) offer(events[ep].b, events[ep].s);
        });
      }
    replay.flush();
    u.t_replay += now_ms() - t1;
  }
  return MPF_OK;
}

// what the two tracked entries ask of the engine and of the tracker
int Engine::tbr_tracked_check(const char *what, int maxtrav)
{
  const std::string w(what);
  if (!ufb_) { set_error("no UFBoot tracker attached"); return MPF_E_STATE; }
  if (!have_tree_) { set_error("no tree set"); return MPF_E_STATE; }
  if (sankoff_ && !(tbr_weighted_ && tbr_weighted_tracked_)) { set_error(w + ": the tracked TBR sweep is not served on the weighted (-cost) engine (its mask rows are Fitch joins)"); return MPF_E_UNSUPPORTED; }
  const UfbState &u = *ufb_;
  if (u.exchange || u.Bl != u.B) { set_error(w + ": not served with a sample-sharded tracker"); return MPF_E_UNSUPPORTED; }
  if (u.store_trees) { set_error(w + ": -storetrees is not served"); return MPF_E_UNSUPPORTED; }
  if (u.topboot) { set_error(w + ": -mulhits -topboot is not served"); return MPF_E_UNSUPPORTED; }
  if (u.distinct) { set_error(w + ": -distinct_iter_top_boot is not served"); return MPF_E_UNSUPPORTED; }
  if (u.ratchet) { set_error(w + ": not served on re-weighted (ratchet) patterns with ratchet booking on"); return MPF_E_UNSUPPORTED; }
  int rc = tbr_check(what, maxtrav, true);            // (a cost matrix that is not symmetric is refused here)
  if (rc) return rc;
  return sankoff_ ? tbr_snk_vals_check(w) : MPF_OK;
}

int Engine::ufboot_tbr_sweep(int maxtrav, uint32_t *best_cost, int32_t *best_f, int32_t *best_g, uint64_t *n_pairs)
{
  int rc = tbr_tracked_check("mpf_ufboot_tbr_sweep", maxtrav);
  if (rc) return rc;
  // (suspended: other weights than the attach-time ones under -no_hclimb1_bb, or an attach-time pattern without a site --
  //  saveCurrentTree is not called, iqtree.cpp:3280: the plain sweep)
  const bool tracked = !ufb_->suspended;
  uint32_t len = 0;
  if (tracked) {
    rc = score_tree(&len);
    if (rc) return rc;
    ufb_->rt_valid = false;
  }
  node_rectifier();
  std::vector<tbrplan::Visit> vis;
  std::vector<TbrBest> best;
  const size_t count = 2 * (size_t)n_ - 2;
  const TbrChunkFn book = [&](size_t first, size_t nv, const uint32_t *cost) { return tbr_book_chunk(vis.data() + first, nv, cost, len); };
  rc = tbr_run(nodep_.data() + 1, count, maxtrav, vis, nullptr, &best, n_pairs, tracked ? &book : nullptr);
  ufb_->rt_valid = false;
  if (rc) return rc;
  for (size_t i = 0; i < count; i++) {
    const TbrBest &t = best[i];
    const tbrplan::Visit &v = vis[i];
    if (v.rows() * v.cols() <= 1) { best_cost[i] = 0xFFFFFFFFu; best_f[i] = best_g[i] = -1; continue; }
    if (t.row >= v.rows() || t.col >= v.cols()) { set_error("TBR: the device reported no best pair"); return MPF_E_STATE; }
    best_cost[i] = t.cost;
    best_f[i] = t.row ? v.F.rec[t.row - 1] : -1;
    best_g[i] = t.col ? v.G.rec[t.col - 1] : -1;
  }
  return MPF_OK;
}

int Engine::ufboot_optimize_tbr(int maxtrav, int max_moves, uint32_t *score, int32_t *n_moves)
{
  int rc = tbr_tracked_check("mpf_ufboot_optimize_tbr", maxtrav);
  if (rc) return rc;
  const bool tracked = !ufb_->suspended;
  ufb_->rt_valid = false;
  rc = tbr_climb(maxtrav, max_moves, tracked, score, n_moves);
  ufb_->rt_valid = false;
  return rc;
}

// DIAGNOSTIC: every entry's mask row of one visit, as k_tbr_masks writes it, read back per original pattern
int Engine::tbr_pattern_terms(int rec, int maxtrav, std::vector<int32_t> &f, std::vector<int32_t> &g, std::vector<uint8_t> *terms)
{
  if (sankoff_) { set_error("mpf_tbr_pattern_terms: Fitch engines only (a mask row is a Fitch join)"); return MPF_E_UNSUPPORTED; }
  int rc = tbr_check("mpf_tbr_pattern_terms", maxtrav, true);
  if (rc) return rc;
  if (rec < 3 || rec >= 3 * (2 * n_ - 1) || back_[rec] < 0) { set_error("mpf_tbr_pattern_terms: bad record"); return MPF_E_INVALID; }
  std::vector<tbrplan::Visit> vis(1);
  if (!terms) {
    tbrplan::visit(n_, back_.data(), rec, maxtrav, vis[0]);
    f = vis[0].F.rec;
    g = vis[0].G.rec;
    return MPF_OK;
  }
  const size_t Wp = (size_t)g_.Wp;
  const TbrChunkFn rows_back = [&](size_t, size_t, const uint32_t *) -> int {
    TbrBuffers &b = *tbr_buf_;
    const size_t nf = vis[0].rows(), ng = vis[0].cols(), rows = nf * ng;
    std::vector<tbrplan::MaskRun> mr;
    std::vector<tbrplan::MaskCol> mc;
    for (size_t i = 0; i < nf; i++)
      for (size_t j = 0; j < ng; j++) {
        if (j % tbrplan::kMaskRunCols == 0) mr.push_back(tbrplan::MaskRun{0u, (uint32_t)i, (uint32_t)mc.size(), (uint32_t)mc.size()});
        mc.push_back(tbrplan::MaskCol{(uint32_t)j, (uint32_t)(i * ng + j)});
        mr.back().end = (uint32_t)mc.size();
      }
    HIPCHK(b.masks.reserve(rows * Wp));
    HIPCHK(b.mruns.reserve(mr.size()));
    HIPCHK(b.mcols.reserve(mc.size()));
    HIPCHK(hipMemcpyAsync(b.mruns.p, mr.data(), mr.size() * sizeof(tbrplan::MaskRun), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemcpyAsync(b.mcols.p, mc.data(), mc.size() * sizeof(tbrplan::MaskCol), hipMemcpyHostToDevice, st_));
    HIPCHK(launch_tbr_masks(st_, g_, vec_rows(), b.store.p, b.visits.p, b.mruns.p, mr.size(), b.mcols.p, b.masks.p));
    std::vector<uint32_t> h(rows * Wp);
    HIPCHK(hipMemcpyAsync(h.data(), b.masks.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    terms->assign(rows * (size_t)P_, 0);
    for (size_t r = 0; r < rows; r++)
      for (int p = 0; p < P_; p++) {
        const int site = first_site_[(size_t)p];
        if (site < 0 || (size_t)site >= 32 * Wp) continue;      // (weight 0 behind the last site of a full row: k_pattern_sum)
        (*terms)[r * (size_t)P_ + (size_t)p] = (uint8_t)((h[r * Wp + (size_t)(site >> 5)] >> (site & 31)) & 1u);
      }
    return MPF_OK;
  };
  const int32_t r = rec;
  rc = tbr_run(&r, 1, maxtrav, vis, nullptr, nullptr, nullptr, &rows_back);
  if (rc) return rc;
  f = vis[0].F.rec;
  g = vis[0].G.rec;
  return MPF_OK;
}

// DIAGNOSTIC, the weighted counterpart: every entry's row of per-pattern lengths of one visit, as k_tbr_snk_vals writes it, read back
// per original pattern
int Engine::tbr_pattern_lengths(int rec, int maxtrav, std::vector<int32_t> &f, std::vector<int32_t> &g, std::vector<uint16_t> *rows_out)
{
  if (!sankoff_) { set_error("mpf_tbr_pattern_lengths: weighted engines only (a Fitch engine has mpf_tbr_pattern_terms)"); return MPF_E_UNSUPPORTED; }
  if (!tbr_weighted_ || !tbr_weighted_tracked_) {
    set_error("mpf_tbr_pattern_lengths: the tracked TBR sweep is not served on the weighted (-cost) engine (its mask rows are Fitch joins)");
    return MPF_E_UNSUPPORTED;
  }
  int rc = tbr_check("mpf_tbr_pattern_lengths", maxtrav, true);
  if (rc) return rc;
  rc = tbr_snk_vals_check("mpf_tbr_pattern_lengths");
  if (rc) return rc;
  if (rec < 3 || rec >= 3 * (2 * n_ - 1) || back_[rec] < 0) { set_error("mpf_tbr_pattern_lengths: bad record"); return MPF_E_INVALID; }
  std::vector<tbrplan::Visit> vis(1);
  if (!rows_out) {
    tbrplan::visit(n_, back_.data(), rec, maxtrav, vis[0]);
    f = vis[0].F.rec;
    g = vis[0].G.rec;
    return MPF_OK;
  }
  const size_t npat = (size_t)g_.Wp;
  const TbrChunkFn rows_back = [&](size_t, size_t, const uint32_t *) -> int {
    TbrBuffers &b = *tbr_buf_;
    const size_t nf = vis[0].rows(), ng = vis[0].cols(), rows = nf * ng;
    std::vector<tbrplan::MaskRun> mr;
    std::vector<tbrplan::MaskCol> mc;
    for (size_t i = 0; i < nf; i++)
      for (size_t j = 0; j < ng; j++) {
        if (j % tbrplan::kMaskRunCols == 0) mr.push_back(tbrplan::MaskRun{0u, (uint32_t)i, (uint32_t)mc.size(), (uint32_t)mc.size()});
        mc.push_back(tbrplan::MaskCol{(uint32_t)j, (uint32_t)(i * ng + j)});
        mr.back().end = (uint32_t)mc.size();
      }
    HIPCHK(b.vals.reserve(rows * npat));
    HIPCHK(b.vmax.reserve(4));
    HIPCHK(b.mruns.reserve(mr.size()));
    HIPCHK(b.mcols.reserve(mc.size()));
    HIPCHK(hipMemcpyAsync(b.mruns.p, mr.data(), mr.size() * sizeof(tbrplan::MaskRun), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemcpyAsync(b.mcols.p, mc.data(), mc.size() * sizeof(tbrplan::MaskCol), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemsetAsync(b.vmax.p, 0, sizeof(uint32_t), st_));
    HIPCHK(launch_tbr_snk_vals(st_, g_, n_, vec_rows(), b.store.p, b.visits.p, b.mruns.p, mr.size(), b.mcols.p, b.vals.p, b.vmax.p));
    std::vector<uint16_t> h(rows * npat);
    HIPCHK(hipMemcpyAsync(h.data(), b.vals.p, h.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    rows_out->assign(rows * (size_t)P_, 0);
    for (int p = 0; p < P_; p++) {
      const int j = first_site_[(size_t)p];          // (weighted engine: the pattern's place among the kept ones)
      if (j < 0 || (size_t)j >= npat) continue;
      for (size_t r = 0; r < rows; r++) (*rows_out)[r * (size_t)P_ + (size_t)p] = h[r * npat + (size_t)j];
    }
    return MPF_OK;
  };
  const int32_t r = rec;
  rc = tbr_run(&r, 1, maxtrav, vis, nullptr, nullptr, nullptr, &rows_back);
  if (rc) return rc;
  f = vis[0].F.rec;
  g = vis[0].G.rec;
  return MPF_OK;
}

}  // namespace mpf
