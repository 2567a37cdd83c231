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
// Not served: a cost matrix that is not symmetric, an engine with a UFBoot tracker attached (nothing would be booked), random ties,
// a device-resident climb.
#include <string>

#include "../csrc/engine.hpp"
#include "../csrc/tbr.hpp"

namespace mpf {

struct TbrBuffers {
  DevBuf<uint32_t> store, deep, out, best;
  DevBuf<tbrplan::Op> ops;
  DevBuf<TbrSide> sides;
  DevBuf<TbrVisit> visits;
  DevBuf<tbrplan::Item> items[2];                  // narrow | wide
  PinBuf<uint32_t> h_best, h_out;
  std::vector<tbrplan::Op> v_ops;
  std::vector<TbrSide> v_sides;
  std::vector<TbrVisit> v_visits;
  std::vector<tbrplan::Item> v_items[2];
};

int Engine::tbr_check(const char *what, int maxtrav)
{
  if (sankoff_ && !tbr_weighted_) {
    set_error(std::string(what) + ": TBR is not served on the weighted (-cost) engine (its cost is a min-plus product rooted at the new edge)");
    return MPF_E_UNSUPPORTED;
  }
  if (sankoff_ && g_.costT) {
    set_error(std::string(what) + ": TBR is not served with a cost matrix that is not symmetric (the length depends on the evaluation edge)");
    return MPF_E_UNSUPPORTED;
  }
  if (ufb_) {
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
                    std::vector<TbrBest> *best, uint64_t *n_pairs)
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
    if (matrix) HIPCHK(b.h_out.reserve(at));
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
    if (matrix && at > 1) HIPCHK(hipMemcpyAsync(b.h_out.p, b.out.p, at * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    HIPCHK(hipStreamSynchronize(st_));
    float ms = 0.f;
    if (timing_ && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) tbr_kernel_ns_ += (uint64_t)((double)ms * 1e6);
    if (best)
      for (size_t k = 0; k < nv; k++) (*best)[ch.first + k] = TbrBest{b.h_best.p[3 * k], b.h_best.p[3 * k + 1], b.h_best.p[3 * k + 2]};
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
    rc = tbr_run(nodep_.data() + 1, count, maxtrav, vis, nullptr, &best, nullptr);
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
    rc = apply_tbr(mv.rec, mv.f_rec, mv.g_rec, &got);
    if (rc) return rc;
    if (got != mv.score) { set_error("TBR: the edited tree does not have the length its matrix entry promised"); return MPF_E_STATE; }
    tbr_moves_.push_back(mv);
    len = got;
  }
  if (score) *score = len;
  if (n_moves) *n_moves = (int32_t)tbr_moves_.size();
  return MPF_OK;
}

}  // namespace mpf
