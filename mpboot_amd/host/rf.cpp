// rf.cpp -- Robinson-Foulds distances between trees on the device split table.
//
// The reference: MTreeSet::computeRFDist (mtreeset.cpp:484-546 for one set -- all pairs, or adjacent pairs at :535 --, :549-660 for
// two sets), printed by pda.cpp:1399-1539 for -rf_all, -rf <treefile2> and -rf_adj.  It turns every tree into Split objects through
// its Newick string and looks every split of one tree up in a hash of the other's, pair by pair.
//
// Here ONE split pass runs over all trees of the call (split_pass of host/splits.cpp: keys -> insert -> count, every tree weight 1,
// the second set behind the first), which gives every inner branch an exact identity: the table slot of its split.  The slots that at
// least two trees hold become the columns of a trees x columns bit matrix, shared(i, j) is the popcount of row i AND row j, and
// RF(i, j) = 2 (n - 3) - 2 shared(i, j) (k_rf_columns, k_rf_rows, k_rf_shared / k_rf_pairs, k_rf_finish of splits.hip); with trees
// given as neighbour lists in the call, which may have fewer splits, c_i + c_j - 2 shared(i, j) from the trees' split counts.  The matrix is
// built and multiplied in chunks of columns within kRfBudgetBytes.  The clusters of the overflow list (true key collisions) are
// grouped by whole-set comparison on the host (splitsets::overflow_columns) and get columns of their own, so the result is exact.
#include <string>

#include "split_sets.hpp"
#include "ufboot_common.hpp"

namespace mpf {

namespace {
int bad(const std::string &what) { set_error("rf distances: " + what); return MPF_E_INVALID; }
}  // namespace

int Engine::rf_distances(int mode, int n_trees, const int32_t *backs, int n_trees2, const int32_t *backs2, int64_t cap, int32_t *rf)
{
  splitsets::TreeSet a, b;
  a.n_records = n_trees;
  a.backs = backs;
  b.n_records = n_trees2;
  b.backs = backs2;
  return rf_distances(mode, a, b, cap, rf);
}

int Engine::rf_distances(int mode, const splitsets::TreeSet &s1, const splitsets::TreeSet &s2, int64_t cap, int32_t *rf)
{
  using namespace splitsets;
  const int n = n_, C = n - 3, words = words_of(n);
  rf_columns_ = rf_chunks_ = rf_launches_ = rf_rows_ns_ = rf_shared_ns_ = 0;
  split_overflow_ = 0;
  if (mode != RF_ALL_PAIRS && mode != RF_ADJACENT && mode != RF_TWO_SETS) return bad("unknown mode " + std::to_string(mode));
  if (s1.size() < 1 || s1.n_records < 0 || s1.n_lists < 0 || !s1.pointers_ok()) return bad("no trees");
  const bool two = mode == RF_TWO_SETS;
  if (two && (s2.size() < 1 || s2.n_records < 0 || s2.n_lists < 0 || !s2.pointers_ok())) return bad("two sets: no second set");
  if (!two && (s2.n_records != 0 || s2.backs || s2.n_lists != 0 || s2.n_inner || s2.first || s2.nbr))
    return bad("a second set is given, but the mode is not MPF_RF_TWO_SETS");
  const int N1 = s1.size(), N2 = two ? s2.size() : 0;
  const int64_t entries = mode == RF_ALL_PAIRS ? (int64_t)N1 * N1 : mode == RF_ADJACENT ? (int64_t)N1 - 1 : (int64_t)N1 * N2;
  if (entries > INT32_MAX) { set_error("rf distances: the result would have more than 2^31 - 1 entries"); return MPF_E_UNSUPPORTED; }
  if (cap < entries) return bad("cap " + std::to_string(cap) + " is smaller than the " + std::to_string(entries) + " entries of the result");
  if (entries && !rf) return bad("null output");
  if (n > kSplitMaxTaxa) {
    set_error("rf distances: more than " + std::to_string(kSplitMaxTaxa) + " taxa (a tree's records and its walk's stack must fit 64 KiB of LDS)");
    return MPF_E_UNSUPPORTED;
  }
  // the checks of mpf_set_tree (records) or of the polytomy hand-over (lists) on every tree
  std::vector<TreeRef> &trees = split_trees_;
  std::vector<int32_t> &hw = split_hw_;
  trees.clear();
  auto tree_name = [&](size_t i) {
    const TreeSet &s = i < (size_t)N1 ? s1 : s2;
    const size_t k = i < (size_t)N1 ? i : i - (size_t)N1;
    return std::string(i < (size_t)N1 ? "" : "second set, ") + (k < (size_t)s.n_records ? "tree " + std::to_string(k) : "list tree " + std::to_string(k - (size_t)s.n_records));
  };
  std::string why;
  for (int set = 0; set < (two ? 2 : 1); set++) {
    const size_t at = trees.size();
    const int stop = set_refs(n, set ? s2 : s1, trees);
    for (size_t t = at; t < trees.size(); t++) {
      if (trees[t].is_list()) {
        if (!lists_ok(n, trees[t].n_inner, trees[t].first, trees[t].nbr, &why)) return bad(tree_name(t) + ": " + why);
      } else if (!links_ok(trees[t].back, n))
        return bad(tree_name(t) + ": inconsistent back links (a complete tree on n_taxa taxa is needed)");
    }
    if (stop >= 0)
      return bad(std::string(set ? "second set, " : "") + "list tree " + std::to_string(stop) + ": n_inner or first[] are not those of a tree on n_taxa taxa");
  }
  hw.assign(trees.size(), 1);
  if (C < 1) {                                     // three taxa: one tree shape, no inner branch
    std::fill(rf, rf + entries, 0);
    return MPF_OK;
  }
  SplitPass ps;
  int rc = split_pass("rf distances", trees, hw, tree_name, false, true, ps);
  if (rc) return rc;
  rf_launches_ = 4 + ps.key_launches;              // keys (one launch for record-format trees alone), insert, count, compact, columns
  SplitBufs &b = split_;
  // true key collisions: the overflow clusters grouped as sets; a group of two or more is a column behind the device's
  std::vector<uint32_t> patch;
  int64_t columns = ps.rf_columns;
  if (ps.n_ovf) {
    rc = split_fetch_sets(ps.D, ps.n_ovf);
    if (rc) return rc;
    rf_launches_++;
    const std::vector<uint32_t> sets(b.h_bits.p, b.h_bits.p + (size_t)ps.n_ovf * (size_t)words);
    std::vector<int64_t> col;
    const int64_t extra = overflow_columns(sets, ps.n_ovf, words, columns, col);
    for (uint32_t k = 0; k < ps.n_ovf; k++)
      if (col[k] >= 0) { patch.push_back(b.h_ids.p[ps.D + k]); patch.push_back((uint32_t)col[k]); }
    columns += extra;
  }
  rf_columns_ = (uint64_t)columns;
  if (!entries) return MPF_OK;                     // adjacent pairs of one tree
  const uint32_t row2 = (uint32_t)(rf_tiles((uint64_t)N1) * kRfTile);
  const uint64_t rows = row2 + (two ? rf_tiles((uint64_t)N2) * kRfTile : 0);
  const std::vector<RfChunk> plan = rf_chunk_plan(columns, (int64_t)rows, rf_chunk_columns_, (int64_t)kRfBudgetBytes, kRfKStep);
  rf_chunks_ = plan.size();
  HIPCHK(rf_out_.reserve((size_t)entries));
  if (plan.empty()) HIPCHK(hipMemsetAsync(rf_out_.p, 0, (size_t)entries * sizeof(int32_t), st_));
  else {
    const size_t max_words = (size_t)rf_round_up((plan[0].c1 - plan[0].c0 + 31) / 32, kRfKStep);
    HIPCHK(rf_bits_.reserve((size_t)rows * max_words));
  }
  const uint32_t n_patch = (uint32_t)(patch.size() / 2);
  if (n_patch) {
    HIPCHK(rf_patch_.reserve(patch.size()));
    HIPCHK(hipMemcpyAsync(rf_patch_.p, patch.data(), patch.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
  }
  for (size_t ci = 0; ci < plan.size(); ci++) {
    const uint32_t c0 = (uint32_t)plan[ci].c0, c1 = (uint32_t)plan[ci].c1;
    const uint32_t row_words = (uint32_t)rf_round_up((c1 - c0 + 31) / 32, kRfKStep);
    HIPCHK(hipMemsetAsync(rf_bits_.p, 0, (size_t)rows * row_words * sizeof(uint32_t), st_));
    if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
    HIPCHK(launch_rf_rows(st_, b.slot_of.p, ps.M, n, b.col_of_slot.p, c0, c1, (uint32_t)N1, row2, row_words, rf_bits_.p));
    HIPCHK(launch_rf_patch(st_, rf_patch_.p, n_patch, n, c0, c1, (uint32_t)N1, row2, row_words, rf_bits_.p));
    if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
    if (mode == RF_ADJACENT) HIPCHK(launch_rf_pairs(st_, rf_bits_.p, row_words, (uint32_t)(N1 - 1), ci > 0, rf_out_.p));
    else HIPCHK(launch_rf_shared(st_, rf_bits_.p, 0, two ? row2 : 0, row_words, !two, (uint32_t)N1, (uint32_t)(two ? N2 : N1), ci > 0, rf_out_.p));
    rf_launches_ += 2 + (n_patch ? 1 : 0);
    if (timing_) {
      HIPCHK(hipEventRecord(ev2_, st_));
      HIPCHK(hipStreamSynchronize(st_));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) rf_rows_ns_ += (uint64_t)((double)ms * 1e6);
      if (hipEventElapsedTime(&ms, ev1_, ev2_) == hipSuccess) rf_shared_ns_ += (uint64_t)((double)ms * 1e6);
    }
  }
  HIPCHK(launch_rf_finish(st_, rf_out_.p, (unsigned long long)entries, n, mode == RF_ALL_PAIRS ? (uint32_t)N1 : 0u, ps.n_splits, (uint32_t)N1,
                          (uint32_t)N2));
  rf_launches_++;
  HIPCHK(hipMemcpyAsync(rf, rf_out_.p, (size_t)entries * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  return MPF_OK;
}

}  // namespace mpf
