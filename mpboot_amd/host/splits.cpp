// splits.cpp -- the summary of a -bb run: split supports on a tree and the bootstrap consensus tree.
//
// The reference: IQTree::summarizeBootstrap (iqtree.cpp:4020-4165) weights the booked trees by the samples that point to them,
// MTreeSet::convertSplits (mtreeset.cpp:288-470) turns every tree into Split objects through its Newick string and counts them in
// a hash map, computeConsensusTree (phyloanalysis.cpp:2488-2600) drops the splits at or below the threshold and keeps a maximal
// compatible set (SplitGraph::findMaxCompatibleSplits, splitgraph.cpp:615-648), and the supports go onto the best tree's branches.
//
// Here the trees stay in the engine's record format.  The device makes every tree's clusters and counts them exactly (splits.hip:
// keys -> insert -> count -> compact); the host checks the trees, resolves the overflow list of true key collisions through whole-set
// comparison, puts the distinct splits in the contract order and runs the consensus rule on the kept sets (host/split_sets.hpp,
// which holds everything that needs no device and is tested stand-alone under a sanitizer).
#include <functional>
#include <string>

#include "split_sets.hpp"
#include "ufboot_common.hpp"

namespace mpf {

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e__) + " (" + __FILE__ + ":" +      \
                std::to_string(__LINE__) + ")");                                                  \
      return MPF_E_HIP;                                                                           \
    }                                                                                             \
  } while (0)

namespace {
int bad(const std::string &what) { set_error("split summary: " + what); return MPF_E_INVALID; }
}  // namespace

// The front half of every call on a tree set: the trees (already checked link by link by the caller) are staged, walked
// (k_split_keys; a tree whose records do not form one tree ends the call, named by `name`), and their clusters inserted and counted
// (k_split_insert, k_split_count, k_split_compact); the counters and the overflow list of true key collisions come back.
// hw[i]: the weight of trees[i].  gather_last: the counts of the last tree's clusters go to split_.h_tsup (a target tree).
// rf: k_rf_columns numbers the slots that at least two trees hold (p.rf_columns).  Afterwards split_.h_entries holds the p.D used
// slots and split_.h_ids[p.D .. p.D + p.n_ovf) the overflow clusters, sorted
int Engine::split_pass(const char *what, const std::vector<const int32_t *> &trees, const std::vector<int32_t> &hw,
                       const std::function<std::string(size_t)> &name, bool gather_last, bool rf, SplitPass &p)
{
  const int n = n_, C = n - 3;
  const size_t len = 3 * (size_t)(2 * n - 1);
  const size_t T = trees.size();
  if ((uint64_t)T * (uint64_t)C > (1ull << 27)) { set_error(std::string(what) + ": more than 2^27 clusters in one call"); return MPF_E_UNSUPPORTED; }
  const uint32_t M = (uint32_t)(T * (size_t)C);
  uint32_t tsize = 64;
  while ((uint64_t)tsize < 2ull * M) tsize <<= 1;
  SplitBufs &b = split_;
  HIPCHK(b.h_backs.reserve(T * len));
  for (size_t i = 0; i < T; i++) std::memcpy(b.h_backs.p + i * len, trees[i], len * sizeof(int32_t));
  HIPCHK(b.backs.reserve(T * len));
  HIPCHK(b.pos.reserve(T * (size_t)n));
  HIPCHK(b.order.reserve(T * (size_t)(n - 1)));
  HIPCHK(b.cl.reserve(M));
  HIPCHK(b.flags.reserve(T));
  HIPCHK(b.h_flags.reserve(T + 4));
  HIPCHK(b.w.reserve(T));
  HIPCHK(b.table.reserve(3 * (size_t)tsize));
  HIPCHK(b.slot_of.reserve(M));
  HIPCHK(b.ovf.reserve(M));
  HIPCHK(b.counters.reserve(4));
  HIPCHK(b.entries.reserve(M));
  if (rf) HIPCHK(b.col_of_slot.reserve(tsize));
  unsigned long long *tkey = b.table.p, *trep = tkey + tsize, *tcount = trep + tsize;
  HIPCHK(hipMemcpyAsync(b.backs.p, b.h_backs.p, T * len * sizeof(int32_t), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemcpyAsync(b.w.p, hw.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(tkey, 0xFF, 2 * (size_t)tsize * sizeof(unsigned long long), st_));      // keys and representatives: empty
  HIPCHK(hipMemsetAsync(tcount, 0, (size_t)tsize * sizeof(unsigned long long), st_));
  HIPCHK(hipMemsetAsync(b.counters.p, 0, 4 * sizeof(uint32_t), st_));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  HIPCHK(launch_split_keys(st_, b.backs.p, (int)T, n, split_key_bits_, b.pos.p, b.order.p, b.cl.p, b.flags.p));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  HIPCHK(hipMemcpyAsync(b.h_flags.p, b.flags.p, T * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  // the later kernels index through what the walk wrote: they start only behind a walk that ended well on every tree
  HIPCHK(hipStreamSynchronize(st_));
  for (size_t i = 0; i < T; i++)
    if (b.h_flags.p[i]) { set_error(std::string(what) + ": " + name(i) + ": the records do not form one tree"); return MPF_E_INVALID; }
  if (timing_) HIPCHK(hipEventRecord(ev2_, st_));
  HIPCHK(launch_split_insert(st_, b.cl.p, M, tkey, trep, tsize, b.slot_of.p));
  HIPCHK(launch_split_count(st_, b.cl.p, M, n, b.pos.p, b.order.p, trep, b.slot_of.p, b.w.p, tcount, b.ovf.p, b.counters.p));
  HIPCHK(launch_split_compact(st_, trep, tcount, tsize, b.entries.p, b.counters.p));
  if (gather_last) {
    HIPCHK(b.tsup.reserve((size_t)C));
    HIPCHK(b.h_tsup.reserve((size_t)C));
    HIPCHK(launch_split_gather(st_, b.slot_of.p, M - (uint32_t)C, (uint32_t)C, tcount, b.tsup.p));
    HIPCHK(hipMemcpyAsync(b.h_tsup.p, b.tsup.p, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost, st_));
  }
  if (timing_) HIPCHK(hipEventRecord(ev3_, st_));
  if (rf) HIPCHK(launch_rf_columns(st_, trep, tcount, tsize, b.col_of_slot.p, b.counters.p));
  HIPCHK(hipMemcpyAsync(b.h_flags.p, b.counters.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  float ms = 0.f;
  if (timing_ && hipEventElapsedTime(&ms, ev0_, ev1_) == hipSuccess) split_keys_ns_ += (uint64_t)((double)ms * 1e6);
  if (timing_ && hipEventElapsedTime(&ms, ev2_, ev3_) == hipSuccess) split_count_ns_ += (uint64_t)((double)ms * 1e6);
  split_launches_++;
  const uint32_t n_ovf = (uint32_t)b.h_flags.p[0], D = (uint32_t)b.h_flags.p[1], cols = (uint32_t)b.h_flags.p[2];
  if (n_ovf > M || D > M || cols > D) { set_error(std::string(what) + ": inconsistent counters"); return MPF_E_STATE; }
  split_overflow_ = n_ovf;
  HIPCHK(b.h_entries.reserve(D + 1));
  HIPCHK(hipMemcpyAsync(b.h_entries.p, b.entries.p, (size_t)D * sizeof(SplitEntry), hipMemcpyDeviceToHost, st_));
  HIPCHK(b.h_ids.reserve((size_t)D + n_ovf + 1));
  if (n_ovf) HIPCHK(hipMemcpyAsync(b.h_ids.p + D, b.ovf.p, (size_t)n_ovf * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  // in cluster order, so that nothing depends on the order the device appended them in
  std::sort(b.h_ids.p + D, b.h_ids.p + D + n_ovf);
  for (uint32_t k = 0; k < n_ovf; k++)
    if (b.h_ids.p[D + k] >= M) { set_error(std::string(what) + ": overflow entry out of range"); return MPF_E_STATE; }
  p = SplitPass{T, M, tsize, n_ovf, D, cols, trep, tcount};
  return MPF_OK;
}

// the sets of the clusters split_.h_ids[first .. first + m), made on the device, into split_.h_bits
int Engine::split_fetch_sets(size_t first, size_t m)
{
  SplitBufs &b = split_;
  const int words = splitsets::words_of(n_);
  HIPCHK(b.ids.reserve(m));
  HIPCHK(b.bits.reserve(m * (size_t)words));
  HIPCHK(b.h_bits.reserve(m * (size_t)words));
  HIPCHK(hipMemcpyAsync(b.ids.p, b.h_ids.p + first, m * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  HIPCHK(launch_split_bits(st_, b.cl.p, b.ids.p, (uint32_t)m, n_, b.pos.p, b.bits.p));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  HIPCHK(hipMemcpyAsync(b.h_bits.p, b.bits.p, m * (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  float t = 0.f;
  if (timing_ && hipEventElapsedTime(&t, ev0_, ev1_) == hipSuccess) split_bits_ns_ += (uint64_t)((double)t * 1e6);
  return MPF_OK;
}

// One pass over the trees.  r.table: the distinct splits with count > max(0, threshold * total) and, if want_sets, their sets -- in
// no particular order.  target (may be null): one more tree of weight 0 whose clusters' counts come back in r.target_support,
// indexed as splitsets::walk_clusters numbers them (r.target)
int Engine::split_run(int n_trees, const int32_t *backs, const int32_t *weights, const int32_t *target, bool want_sets, double threshold, SplitRun &r)
{
  const int n = n_, C = n - 3, words = splitsets::words_of(n);
  const size_t len = 3 * (size_t)(2 * n - 1);
  splitsets::SplitTable &tab = r.table;
  tab.n = n;
  tab.words = words;
  tab.total = 0;
  tab.bits.clear();
  tab.count.clear();
  r.target_support.clear();
  split_overflow_ = 0;
  if (n_trees < 1 || !backs) return bad("no trees");
  if (n > kSplitMaxTaxa) {
    set_error("split summary: more than " + std::to_string(kSplitMaxTaxa) + " taxa (a tree's records and its walk's stack must fit 64 KiB of LDS)");
    return MPF_E_UNSUPPORTED;
  }
  // the checks of mpf_set_tree on every tree; trees of weight 0 are left out here
  std::vector<int32_t> &hw = split_hw_;
  std::vector<int32_t> &pick = split_pick_;
  std::vector<const int32_t *> &trees = split_trees_;
  hw.clear();
  pick.clear();
  trees.clear();
  for (int t = 0; t < n_trees; t++) {
    const int32_t w = weights ? weights[t] : 1;
    if (w < 0) return bad("tree " + std::to_string(t) + " has a negative weight");
    if (!splitsets::links_ok(backs + (size_t)t * len, n)) return bad("tree " + std::to_string(t) + ": inconsistent back links (a complete tree on n_taxa taxa is needed)");
    if (!w) continue;
    tab.total += w;
    hw.push_back(w);
    pick.push_back(t);
    trees.push_back(backs + (size_t)t * len);
  }
  if (target) {
    if (!splitsets::links_ok(target, n)) return bad("target tree: inconsistent back links (a complete tree on n_taxa taxa is needed)");
    if (!splitsets::walk_clusters(target, n, r.target)) return bad("target tree: the records do not form one tree");
    r.target_support.assign((size_t)std::max(C, 0), 0);
    hw.push_back(0);
    trees.push_back(target);
  }
  if (C < 1 || hw.empty()) return MPF_OK;
  SplitPass ps;
  int rc = split_pass("split summary", trees, hw,
                      [&](size_t i) { return i < pick.size() ? "tree " + std::to_string(pick[i]) : std::string("target tree"); }, target != nullptr,
                      false, ps);
  if (rc) return rc;
  SplitBufs &b = split_;
  const uint32_t M = ps.M, n_ovf = ps.n_ovf, D = ps.D;
  const SplitEntry *ent = b.h_entries.p;
  const double cut = threshold * (double)tab.total;
  auto passes = [&](int64_t c) { return c > 0 && (double)c > cut; };
  if (!n_ovf) {
    // no collision: every slot is one split and its count is final
    if (target)
      for (int ci = 0; ci < C; ci++) r.target_support[(size_t)ci] = b.h_tsup.p[ci];
    size_t m = 0;
    for (uint32_t i = 0; i < D; i++)
      if (passes((int64_t)ent[i].count)) { b.h_ids.p[m++] = ent[i].rep; tab.count.push_back((int64_t)ent[i].count); }
    if (want_sets && m) {
      rc = split_fetch_sets(0, m);
      if (rc) return rc;
      tab.bits.assign(b.h_bits.p, b.h_bits.p + m * (size_t)words);
    }
    return MPF_OK;
  }
  // true key collisions (in practice only under the test option split_key_bits): the sets of every representative and of every
  // cluster on the overflow list, then the overflow clusters one by one through an exact index -- in cluster order, so that the
  // result does not depend on the order the device appended them in
  for (uint32_t i = 0; i < D; i++) b.h_ids.p[i] = ent[i].rep;
  rc = split_fetch_sets(0, (size_t)D + n_ovf);
  if (rc) return rc;
  std::vector<uint32_t> rows(b.h_bits.p, b.h_bits.p + (size_t)D * (size_t)words);
  std::vector<int64_t> cnt((size_t)D);
  splitsets::SetIndex idx(words);
  idx.reserve((size_t)D + n_ovf);
  for (uint32_t i = 0; i < D; i++) { cnt[i] = (int64_t)ent[i].count; idx.insert(rows.data() + (size_t)i * (size_t)words, i); }
  const uint32_t target_first = target ? M - (uint32_t)C : M;
  std::vector<int64_t> target_row((size_t)std::max(C, 0), -1);
  for (uint32_t k = 0; k < n_ovf; k++) {
    const uint32_t g = b.h_ids.p[D + k];
    const uint32_t *w = b.h_bits.p + ((size_t)D + k) * (size_t)words;
    int64_t row = idx.find(rows, w);
    if (row < 0) {
      row = (int64_t)cnt.size();
      rows.insert(rows.end(), w, w + words);
      cnt.push_back(0);
      idx.insert(w, row);
    }
    cnt[(size_t)row] += hw[g / (uint32_t)C];
    if (g >= target_first) target_row[g - target_first] = row;
  }
  if (target)
    for (int ci = 0; ci < C; ci++)
      r.target_support[(size_t)ci] = target_row[(size_t)ci] >= 0 ? cnt[(size_t)target_row[(size_t)ci]] : (int64_t)b.h_tsup.p[ci];
  for (size_t i = 0; i < cnt.size(); i++)
    if (passes(cnt[i])) {
      tab.count.push_back(cnt[i]);
      if (want_sets) tab.bits.insert(tab.bits.end(), rows.begin() + (long)(i * (size_t)words), rows.begin() + (long)((i + 1) * (size_t)words));
    }
  return MPF_OK;
}

// MTreeSet::convertSplits: the distinct splits of the trees with their summed weights, in the contract order
int Engine::split_counts(int n_trees, const int32_t *backs, const int32_t *weights, splitsets::SplitTable &out)
{
  SplitRun &r = split_run_;
  int rc = split_run(n_trees, backs, weights, nullptr, true, -1.0, r);
  if (rc) return rc;
  splitsets::apply_order(r.table, splitsets::order_splits(r.table));
  out = r.table;
  return MPF_OK;
}

// the supports of the branches of `target`, in the walk order of branch_substitutions from tip 1 (fixNegativeBranch's walk)
int Engine::split_support(int n_trees, const int32_t *backs, const int32_t *weights, const int32_t *target, std::vector<NniBranch> &br,
                          std::vector<int64_t> &support, int64_t *total)
{
  if (!target) return bad("null target tree");
  SplitRun &r = split_run_;
  int rc = split_run(n_trees, backs, weights, target, false, -1.0, r);
  if (rc) return rc;
  std::vector<int32_t> cluster_of((size_t)2 * n_, -1);
  for (size_t ci = 0; ci < r.target.node.size(); ci++) cluster_of[(size_t)r.target.node[ci]] = (int32_t)ci;
  br.clear();
  struct F { int node, dad; };
  std::vector<F> st{F{1, 0}};
  while (!st.empty()) {                            // Engine::branch_order on the target's records
    const F f = st.back();
    st.pop_back();
    if (f.dad) br.push_back(NniBranch{f.dad, f.node});
    for (int s = (f.node > n_ ? 2 : 0); s >= 0; s--) {
      const int nb = target[3 * f.node + s] / 3;
      if (nb != f.dad) st.push_back(F{nb, f.node});
    }
  }
  support.assign(br.size(), -1);
  for (size_t i = 0; i < br.size(); i++) {
    const int32_t ci = br[i].node2 > n_ ? cluster_of[(size_t)br[i].node2] : -1;
    if (ci >= 0) support[i] = r.target_support[(size_t)ci];
  }
  if (total) *total = r.table.total;
  return MPF_OK;
}

// computeConsensusTree: threshold filter, contract order, greedy maximal compatible set, neighbour lists
int Engine::consensus_tree(int n_trees, const int32_t *backs, const int32_t *weights, double threshold, splitsets::ListTree &out, int64_t *total)
{
  if (!(threshold >= 0.0 && threshold <= 1.0)) return bad("threshold must be in 0 .. 1");
  SplitRun &r = split_run_;
  int rc = split_run(n_trees, backs, weights, nullptr, true, threshold, r);
  if (rc) return rc;
  splitsets::apply_order(r.table, splitsets::order_splits(r.table));
  splitsets::build_lists(r.table, splitsets::greedy_compatible(r.table, threshold), out);
  if (total) *total = r.table.total;
  return MPF_OK;
}

// The weighted tree set of IQTree::summarizeBootstrap from the attached tracker.  rule 0: tree_weights[boot_trees[b]]++
// (iqtree.cpp:4036-4038); 1: -mulhits, += B / |boot_trees_parsimony[b]| for each tree of the sample (:4097-4115); 2: -mulhits
// -topboot, +1 per listed tree (:4117-4130); -1: the one the tracker's own options select, as the reference does (:4021-4027)
int Engine::ufboot_summary_trees(int rule, std::vector<int32_t> &backs, std::vector<int32_t> &weights, std::vector<int64_t> &index)
{
  if (!ufb_) { set_error("no UFBoot tracker attached"); return MPF_E_STATE; }
  ufb_drain_log();
  const UfbState &u = *ufb_;
  if (rule == -1) rule = u.mulhits ? (u.topboot ? 2 : 1) : 0;
  if (rule < 0 || rule > 2) return bad("rule must be -1, 0, 1 or 2");
  if ((rule == 1 && !u.mulhits) || (rule == 2 && !(u.mulhits && u.topboot))) {
    set_error("split summary: the tracker does not keep the lists of that rule");
    return MPF_E_STATE;
  }
  std::map<int64_t, int64_t> tally;
  for (int b = 0; b < u.B; b++) {
    if (rule == 0) { if (u.boot_trees[(size_t)b] >= 0) tally[u.boot_trees[(size_t)b]]++; }
    else if (rule == 1) {
      const auto &hs = u.hit_sets[(size_t)b];
      if (hs.empty()) continue;
      const int64_t scale = (int64_t)u.B / (int64_t)hs.size();
      for (int64_t t : hs) tally[t] += scale;
    } else
      for (const auto &e : u.top[(size_t)b]) tally[e.first]++;
  }
  const size_t len = 3 * (size_t)(2 * n_ - 1);
  backs.clear();
  weights.clear();
  index.clear();
  for (const auto &kv : tally) {
    auto it = u.store.find(kv.first);
    if (it == u.store.end()) { set_error("split summary: the tracker holds no topology for tree " + std::to_string(kv.first)); return MPF_E_STATE; }
    if (kv.second > INT32_MAX) return bad("a tree's weight does not fit 32 bits");
    backs.insert(backs.end(), it->second.begin(), it->second.begin() + (long)len);
    weights.push_back((int32_t)kv.second);
    index.push_back(kv.first);
  }
  if (index.empty()) { set_error("split summary: no sample points to a tree yet"); return MPF_E_STATE; }
  return MPF_OK;
}

}  // namespace mpf
