// ufboot_snk.cpp -- the tracked climb on the weighted (Sankoff, -cost) engine
#include "ufboot_common.hpp"

namespace mpf {

// The same loop on the weighted (Sankoff) engine.  pllComputePatternParsimony dispatches to
// pllComputeSankoffPatternParsimony there (sprparsimony.cpp:3341-3355): the per-pattern lengths of the tentative tree are the
// minima the evaluate has just taken.  The scan writes them for every insertion test (k_snk_scan, 16 bits each), k_vals_planes
// slices them into bit planes and REPS = sum_k 2^k (plane k x weights) on the matrix cores; the current tree's own row is
// multiplied along with every batch and serves as the "home" row of the event formula, so that a candidate's score is its own
// product row and the current tree's slots score R_T.  Scans are host-planned (as every weighted scan).  Shared with the other
// tracked loops (host/ufboot_common.hpp): the replay of a prune-node visit -- cut-off filter, ratchet gate, update rules, the two
// SPR rules, in the reference's order -- and the exchange of a sharded run; this loop's own: the batch's device work, a plan's
// candidate list, and a booked tree's length on the original alignment straight from its product row.
int Engine::spr_sweeps_ufboot_snk(int mintrav, int maxtrav, uint32_t randomMP, uint32_t *final_score)
{
  UfbState &u = *ufb_;
  if (u.exchange) {
    // sample-sharded run: every rank must cut the climb into the same batches -- start from a fixed batch policy state
    gap_est_ = -1.0;
    since_move_ = 0;
  }
  uint32_t exchange_tag = 0;
  uint32_t startMP;
  unsigned iter_hits = 1;
  const int total = 2 * n_ - 2;
  const uint32_t npat = (uint32_t)g_.Wp;
  std::vector<ScanPlan> plans;
  const uint32_t *out = nullptr;
  int batch = first_batch();
  std::vector<UfbEvent> events, ev_tmp;
  std::vector<uint32_t> ev_count, small;
  std::vector<uint2> hinfo;
  std::vector<int32_t> lcol;
  const bool ratchet = u.ratchet;
  const bool store_trees = u.store_trees;          // -storetrees (iqtree.cpp:3302-3346)
  // (an asymmetric matrix gives the CURRENT tree another length and another row at every prune node's visit -- it is evaluated at
  //  that node's edge, evaluateParsimony(p) of :2285 --: the scan writes both to the visit's slot, scan_batch)
  const bool asym = asym_;
  const bool host_self = !u.exchange && !asym;     // (sample-sharded: R_T lives in pieces on the ranks, the current tree's bookings come as device events)
  const int oc = u.Bl;
  if (ratchet) u.gate_closed = false;
  bool stale_init = false;                         // ratchet: _pattern_pars of the climb's start tree, known after the first product
  // (no deferred mode on this engine; asym: the current tree's bookings have the visit's slot as their cost and their row)
  struct Visit : UfbVisit {
    const std::vector<int32_t> *lcol = nullptr;
    bool next(const ScanPlan &pl, Cursor &at, Cand &cd) const
    {
      if (at.c >= pl.cands.size()) return false;
      const uint32_t idx = pl.cands[at.c].out;
      cd = Cand{at.c++, idx, out[idx], 0u};
      return true;
    }
    uint32_t stale_len(uint32_t idx, uint32_t) const { return (uint32_t)(*lcol)[(size_t)idx]; }
  } V;
  V.e = this; V.events = &events; V.lcol = &lcol;
  V.ratchet = ratchet; V.store_trees = store_trees; V.host_self = host_self; V.self_row = asym;
  do {
    startMP = randomMP;
    node_rectifier();
    int i = 1;
    while (i <= total) {
      const int hi = std::min(total, i + batch - 1);
      const int np = hi - i + 1;
      UCHK(u.vmax.reserve(4));
      UCHK(hipMemsetAsync(u.vmax.p, 0, sizeof(uint32_t), st_));      // (a batch without any insertion test launches no scan)
      scan_vals_ = true;
      int rc = scan_batch(plans, nodep_.data() + i, np, mintrav, maxtrav, &out);
      scan_vals_ = false;
      if (rc) return rc;
      u.batches++;
      const uint32_t n_idx = vals_rows_;           // output indices: a slot for the current tree in front of every prune node's candidates
      const uint32_t R = n_idx;                    // the current tree's row of the product
      int jstar = np - 1;
      for (int j = 0; j < np; j++) {
        const ScanPlan &pl = plans[(size_t)j];
        uint32_t m = UINT32_MAX;
        for (const Candidate &cd : pl.cands) m = std::min(m, out[cd.out]);
        if (m < randomMP) { jstar = j; break; }
      }
      const UfbCutoff cut = ufb_cutoff(u.logl_cutoff);
      const bool skip_product = store_trees ? false : ratchet ? (u.gate_closed || cut.none_pass) : cut.none_pass;
      bool have_C = false;
      events.clear();
      if (!skip_product) {
        // ---- the current tree's row, the bit planes, the product
        UCHK(u.vals.reserve(((size_t)n_idx + 1) * npat));
        UCHK(u.h_vmax.reserve(4));
        if (asym) UCHK(launch_sankoff_pattern(st_, g_, vec_rows(), slot(back_[start_]), slot(start_), u.vals.p + (size_t)R * npat, u.vmax.p));     // (left = far end, as tree_length)
        else UCHK(launch_sankoff_pattern(st_, g_, vec_rows(), slot(start_), slot(back_[start_]), u.vals.p + (size_t)R * npat, u.vmax.p));
        UCHK(hipMemcpyAsync(u.h_vmax.p, u.vmax.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        UCHK(hipStreamSynchronize(st_));
        const uint32_t rows = n_idx + 1;
        UfbPlanes P;
        { int rc2 = ufb_vals_planes(u.vals.p, rows, u.h_vmax.p[0], P); if (rc2) return rc2; }
        const int rows_p = P.rows_p;
        { int rc2 = ufb_weighted_product(P, rows_p, nullptr, R); if (rc2) return rc2; }
        UCHK(u.h_rt.reserve((size_t)u.Bp));
        UCHK(hipMemcpyAsync(u.h_rt.p, u.rt.p, (size_t)u.Bl * sizeof(int32_t), hipMemcpyDeviceToHost, st_));    // synchronised below
        have_C = true;
        // ---- per output index: (row, part) for candidates of plans [0, jstar], the current tree's slots, everything else off
        uint32_t n_parts = 0;
        hinfo.assign((size_t)n_idx, make_uint2(0u, 0xFFFFFFFFu));
        const bool self_pass = ratchet || store_trees || cut.passes(randomMP);
        for (int j = 0; j <= jstar; j++) {
          const ScanPlan &pl = plans[(size_t)j];
          // (asym: the visit's slot is a row of its own -- it takes part like a candidate, its cost the length at that edge)
          if (pl.self_idx >= 0) hinfo[(size_t)pl.self_idx] = asym ? make_uint2((uint32_t)pl.self_idx, (uint32_t)j)
                                                                   : make_uint2(0u, (self_pass && !host_self) ? 0xFFFFFFFEu : 0xFFFFFFFFu);
          for (const Candidate &cd : pl.cands) hinfo[cd.out] = make_uint2(cd.out, (uint32_t)j);
          n_parts = (uint32_t)j + 1u;
        }
        // staging: thr[n_parts] | home[n_parts] | best[Bp]
        const size_t o_cnt = (size_t)2 * n_parts + (size_t)u.Bp;   // the event counter: a zero word of this upload
        small.assign(o_cnt + 1, 0u);
        for (uint32_t d = 0; d < n_parts; d++) {
          small[d] = (ratchet || store_trees) ? UINT32_MAX : cut.part_threshold(0u);            // max cost + 1 (costs are full lengths here)
          small[n_parts + d] = R;
        }
        for (int c2 = 0; c2 < u.Bl; c2++) small[(size_t)2 * n_parts + (size_t)c2] = ufb_event_bound((uint32_t)u.ids[(size_t)c2]);
        UCHK(u.h_small.reserve(small.size() + 4));
        std::memcpy(u.h_small.p, small.data(), small.size() * sizeof(uint32_t));
        UCHK(u.thr.reserve(small.size() + 4));
        UCHK(u.info.reserve((size_t)std::max<uint32_t>(n_idx, 1u)));
        UCHK(hipMemcpyAsync(u.thr.p, u.h_small.p, small.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
        if (n_idx) UCHK(hipMemcpyAsync(u.info.p, hinfo.data(), (size_t)n_idx * sizeof(uint2), hipMemcpyHostToDevice, st_));
        const uint32_t *d_thr = u.thr.p, *d_home = u.thr.p + n_parts, *d_best = u.thr.p + 2 * n_parts;
        if (ratchet) {
          UCHK(u.d_col.reserve((size_t)rows_p));
          UCHK(u.h_col.reserve((size_t)rows_p));
          UCHK(launch_ufb_column(st_, u.C.p, u.Bp, oc, rows, u.d_col.p));
          UCHK(hipMemcpyAsync(u.h_col.p, u.d_col.p, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
        }
        uint32_t n_ev = 0;
        const UfbExtract x{u.info.p, d_out(), d_thr, d_home, nullptr, d_best, u.thr.p + o_cnt, n_idx, (u.topboot || u.distinct || store_trees) ? 1 : 0};
        if (n_idx) { int rc2 = ufb_extract_events(x, n_ev); if (rc2) return rc2; }
        else UCHK(hipStreamSynchronize(st_));
        if (timing_) {
          float ms = 0;
          if (hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) u.gemm_ms += ms;
        }
        events.assign(u.h_ev.p, u.h_ev.p + n_ev);
        for (UfbEvent &ev : events) ev.b = (uint32_t)u.ids[(size_t)ev.b];
        if (u.exchange) { int rc2 = ufb_gather_events(events, exchange_tag++); if (rc2) return rc2; }
        sort_events(events, ev_tmp, ev_count, std::max<uint32_t>(n_idx, 1u), (uint32_t)u.B);
        u.events += n_ev;
        if (ratchet) {
          lcol.assign(u.h_col.p, u.h_col.p + rows);
          u.rt_orig = (uint32_t)lcol[(size_t)R];
          if (!stale_init) { u.stale_len = u.rt_orig; stale_init = true; }       // what the IQ-TREE kernel left for the start tree
        }
      }
      // ---- host replay in the reference's order
      V.out = out; V.h_rt = u.h_rt.p; V.ep = 0;
      V.cut = cut; V.product_self = V.product_cand = have_C;
      bool moved = false;
      int j = i;
      for (; j <= hi && !moved; j++) {
        { int rc2 = ufb_replay_visit(plans[(size_t)(j - i)], V, randomMP, iter_hits); if (rc2) return rc2; }
        if (V.accept) {
          moves_.push_back(Move{remove_rec_, insert_rec_, best_});
          apply_move(remove_rec_, insert_rec_);
          randomMP = best_;
          moved = true;
        }
      }
      batch = next_batch(batch, moved, j - i, total);
      i = j;
    }
  } while (randomMP < startMP);
  climb_finished(total);
  u.rt_valid = false;
  { int rc = ufb_close_exchange(); if (rc) return rc; }
  if (final_score) *final_score = randomMP;
  return MPF_OK;
}

}  // namespace mpf
