// splits.cpp -- the summary of a -bb run: split supports on a tree and the bootstrap consensus tree.
//
// The reference: IQTree::summarizeBootstrap (iqtree.cpp:4020-4165) weights the booked trees by the samples that point to them,
// MTreeSet::convertSplits (mtreeset.cpp:288-470) turns every tree into Split objects through its Newick string and counts them in
// a hash map, computeConsensusTree (phyloanalysis.cpp:2488-2600) drops the splits at or below the threshold and keeps a maximal
// compatible set (SplitGraph::findMaxCompatibleSplits, splitgraph.cpp:615-648), and the supports go onto the best tree's branches.
//
// Here the trees stay in the engine's record format, or come as CSR neighbour lists where an inner node has more than three
// neighbours (the consensus tree itself, user trees with polytomies: the hand-over of mpf_polytomy_*).  The device makes every tree's clusters and counts them exactly (splits.hip:
// keys -> insert -> count -> compact); the host checks the trees, resolves the overflow list of true key collisions through whole-set
// comparison, puts the distinct splits in the contract order and runs the consensus rule on the kept sets (host/split_sets.hpp,
// which holds everything that needs no device and is tested stand-alone under a sanitizer).
#include <functional>
#include <string>

#include "split_sets.hpp"
#include "ufboot_common.hpp"

namespace mpf {

namespace {
int bad(const std::string &what) { set_error("split summary: " + what); return MPF_E_INVALID; }
}  // namespace

// The front half of every call on a tree set: the trees (already checked link by link by the caller) are staged, walked
// (k_split_keys over every run of record-format trees, k_split_keys_lists over all list trees, into the same pos / order / cluster
// arrays; a tree whose records or lists do not form one tree ends the call, named by `name`), and their clusters inserted and counted
// (k_split_insert, k_split_count, k_split_compact); the counters and the overflow list of true key collisions come back.
// hw[i]: the weight of trees[i].  gather_last: the counts of the last tree's clusters go to split_.h_tsup (a target tree).
// rf: k_rf_columns numbers the slots that at least two trees hold (p.rf_columns).  Afterwards split_.h_entries holds the p.D used
// slots and split_.h_ids[p.D .. p.D + p.n_ovf) the overflow clusters, sorted
int Engine::split_pass(const char *what, const std::vector<splitsets::TreeRef> &trees, const std::vector<int32_t> &hw,
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
  size_t R = 0, L = 0, list_words = 0;
  for (const splitsets::TreeRef &t : trees) {
    if (!t.is_list()) { R++; continue; }
    L++;
    list_words += (size_t)t.n_inner + 1 + (size_t)t.first[t.n_inner];
  }
  HIPCHK(b.h_backs.reserve(R * len));
  HIPCHK(b.backs.reserve(R * len));
  constexpr size_t kDescWords = sizeof(SplitListDesc) / sizeof(int32_t);
  if (L) {
    // the list trees: their descriptors, then every tree's first[] and nbr[]
    HIPCHK(b.h_lists.reserve(L * kDescWords + list_words));
    HIPCHK(b.lists.reserve(L * kDescWords + list_words));
    HIPCHK(b.n_splits.reserve(T));
    HIPCHK(b.h_n_splits.reserve(T));
  }
  {
    SplitListDesc *desc = reinterpret_cast<SplitListDesc *>(b.h_lists.p);
    size_t r = 0, l = 0, at = L * kDescWords;
    for (size_t i = 0; i < T; i++) {
      const splitsets::TreeRef &t = trees[i];
      if (L) b.h_n_splits.p[i] = t.clusters(n);
      if (!t.is_list()) { std::memcpy(b.h_backs.p + r++ * len, t.back, len * sizeof(int32_t)); continue; }
      const int32_t E = t.first[t.n_inner];
      desc[l++] = SplitListDesc{(int32_t)i, t.n_inner, (int32_t)at, (int32_t)(at + (size_t)t.n_inner + 1), E,
                                splitsets::list_root(n, t.n_inner, t.first, t.nbr)};
      std::memcpy(b.h_lists.p + at, t.first, ((size_t)t.n_inner + 1) * sizeof(int32_t));
      std::memcpy(b.h_lists.p + at + (size_t)t.n_inner + 1, t.nbr, (size_t)E * sizeof(int32_t));
      at += (size_t)t.n_inner + 1 + (size_t)E;
    }
  }
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
  if (R) HIPCHK(hipMemcpyAsync(b.backs.p, b.h_backs.p, R * len * sizeof(int32_t), hipMemcpyHostToDevice, st_));
  if (L) {
    HIPCHK(hipMemcpyAsync(b.lists.p, b.h_lists.p, (L * kDescWords + list_words) * sizeof(int32_t), hipMemcpyHostToDevice, st_));
    HIPCHK(hipMemcpyAsync(b.n_splits.p, b.h_n_splits.p, T * sizeof(int32_t), hipMemcpyHostToDevice, st_));
  }
  HIPCHK(hipMemcpyAsync(b.w.p, hw.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(tkey, 0xFF, 2 * (size_t)tsize * sizeof(unsigned long long), st_));      // keys and representatives: empty
  HIPCHK(hipMemsetAsync(tcount, 0, (size_t)tsize * sizeof(unsigned long long), st_));
  HIPCHK(hipMemsetAsync(b.counters.p, 0, 4 * sizeof(uint32_t), st_));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  uint32_t key_launches = 0;
  for (size_t i = 0, r = 0; i < T;) {                // the record walk over every run of record-format trees
    if (trees[i].is_list()) { i++; continue; }
    size_t j = i;
    while (j < T && !trees[j].is_list()) j++;
    HIPCHK(launch_split_keys(st_, b.backs.p + r * len, (int)(j - i), n, split_key_bits_, b.pos.p + i * (size_t)n, b.order.p + i * (size_t)(n - 1),
                             b.cl.p + i * (size_t)C, b.flags.p + i));
    key_launches++;
    r += j - i;
    i = j;
  }
  if (L) {                                           // the list walk over all list trees, into the same arrays
    HIPCHK(launch_split_keys_lists(st_, reinterpret_cast<const SplitListDesc *>(b.lists.p), (int)L, b.lists.p, n, split_key_bits_, b.pos.p,
                                   b.order.p, b.cl.p, b.flags.p));
    key_launches++;
  }
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  HIPCHK(hipMemcpyAsync(b.h_flags.p, b.flags.p, T * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  // the later kernels index through what the walk wrote: they start only behind a walk that ended well on every tree
  HIPCHK(hipStreamSynchronize(st_));
  for (size_t i = 0; i < T; i++)
    if (b.h_flags.p[i]) {
      set_error(std::string(what) + ": " + name(i) + (trees[i].is_list() ? ": the lists do not form one tree" : ": the records do not form one tree"));
      return MPF_E_INVALID;
    }
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
  p = SplitPass{T, M, tsize, n_ovf, D, cols, trep, tcount, key_launches, L ? b.n_splits.p : nullptr};
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
// indexed as splitsets::walk_clusters / walk_clusters_lists number them (r.target)
int Engine::split_run(const splitsets::TreeSet &set, const int32_t *weights, const splitsets::TreeRef *target, bool want_sets, double threshold,
                      SplitRun &r)
{
  const int n = n_, C = n - 3, words = splitsets::words_of(n);
  splitsets::SplitTable &tab = r.table;
  tab.n = n;
  tab.words = words;
  tab.total = 0;
  tab.bits.clear();
  tab.count.clear();
  r.target_support.clear();
  split_overflow_ = 0;
  if (set.size() < 1 || set.n_records < 0 || set.n_lists < 0 || !set.pointers_ok()) return bad("no trees");
  if (n > kSplitMaxTaxa) {
    set_error("split summary: more than " + std::to_string(kSplitMaxTaxa) + " taxa (a tree's records and its walk's stack must fit 64 KiB of LDS)");
    return MPF_E_UNSUPPORTED;
  }
  // the checks of mpf_set_tree (records) or of the polytomy hand-over (lists) on every tree; trees of weight 0 are left out here
  std::vector<int32_t> &hw = split_hw_;
  std::vector<int32_t> &pick = split_pick_;
  std::vector<splitsets::TreeRef> &trees = split_trees_;
  std::vector<splitsets::TreeRef> &all = split_all_;
  hw.clear();
  pick.clear();
  trees.clear();
  all.clear();
  const int stop = splitsets::set_refs(n, set, all);
  auto tree_name = [&](size_t t) {
    return t < (size_t)set.n_records ? "tree " + std::to_string(t) : "list tree " + std::to_string(t - (size_t)set.n_records);
  };
  std::string why;
  for (size_t t = 0; t < all.size(); t++) {
    const int32_t w = weights ? weights[t] : 1;
    if (w < 0) return bad(tree_name(t) + " has a negative weight");
    if (all[t].is_list()) {
      if (!splitsets::lists_ok(n, all[t].n_inner, all[t].first, all[t].nbr, &why)) return bad(tree_name(t) + ": " + why);
    } else if (!splitsets::links_ok(all[t].back, n))
      return bad(tree_name(t) + ": inconsistent back links (a complete tree on n_taxa taxa is needed)");
    if (!w) continue;
    tab.total += w;
    hw.push_back(w);
    pick.push_back((int32_t)t);
    trees.push_back(all[t]);
  }
  if (stop >= 0) return bad("list tree " + std::to_string(stop) + ": n_inner or first[] are not those of a tree on n_taxa taxa");
  if (target) {
    if (target->is_list()) {
      if (!listtree::check(n, target->n_inner, target->first, target->nbr, 1, false, r.target_shape, &why)) return bad("target tree: " + why);
      if (!splitsets::walk_clusters_lists(n, target->n_inner, target->first, target->nbr, r.target)) return bad("target tree: the lists do not form one tree");
    } else {
      if (!splitsets::links_ok(target->back, n)) return bad("target tree: inconsistent back links (a complete tree on n_taxa taxa is needed)");
      if (!splitsets::walk_clusters(target->back, n, r.target)) return bad("target tree: the records do not form one tree");
    }
    r.target_support.assign((size_t)r.target.size(), 0);
    hw.push_back(0);
    trees.push_back(*target);
  }
  if (C < 1 || hw.empty()) return MPF_OK;
  SplitPass ps;
  int rc = split_pass("split summary", trees, hw,
                      [&](size_t i) { return i < pick.size() ? tree_name((size_t)pick[i]) : std::string("target tree"); }, target != nullptr,
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
      for (int ci = 0; ci < r.target.size(); ci++) r.target_support[(size_t)ci] = b.h_tsup.p[ci];
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
    for (int ci = 0; ci < r.target.size(); ci++)
      r.target_support[(size_t)ci] = target_row[(size_t)ci] >= 0 ? cnt[(size_t)target_row[(size_t)ci]] : (int64_t)b.h_tsup.p[ci];
  for (size_t i = 0; i < cnt.size(); i++)
    if (passes(cnt[i])) {
      tab.count.push_back(cnt[i]);
      if (want_sets) tab.bits.insert(tab.bits.end(), rows.begin() + (long)(i * (size_t)words), rows.begin() + (long)((i + 1) * (size_t)words));
    }
  return MPF_OK;
}

// MTreeSet::convertSplits: the distinct splits of the trees with their summed weights, in the contract order
int Engine::split_counts(const splitsets::TreeSet &set, const int32_t *weights, splitsets::SplitTable &out)
{
  SplitRun &r = split_run_;
  int rc = split_run(set, weights, nullptr, true, -1.0, r);
  if (rc) return rc;
  splitsets::apply_order(r.table, splitsets::order_splits(r.table));
  out = r.table;
  return MPF_OK;
}

// the supports of the branches of `target`: a record-format target in the walk order of branch_substitutions from tip 1
// (fixNegativeBranch's walk), a list target in that of polytomy_branch_substitutions from tip 1 (the same walk, neighbours in list
// order).  -1 on a leaf branch and -- a list target -- on the branch at tip 1
int Engine::split_support(const splitsets::TreeSet &set, const int32_t *weights, const splitsets::TreeRef &target, std::vector<NniBranch> &br,
                          std::vector<int64_t> &support, int64_t *total)
{
  if (target.is_list() && (!target.first || !target.nbr)) return bad("null target tree");
  SplitRun &r = split_run_;
  int rc = split_run(set, weights, &target, false, -1.0, r);
  if (rc) return rc;
  const int N = target.is_list() ? n_ + target.n_inner : 2 * n_ - 2;
  std::vector<int32_t> cluster_of((size_t)N + 1, -1);
  for (size_t ci = 0; ci < r.target.node.size(); ci++) cluster_of[(size_t)r.target.node[ci]] = (int32_t)ci;
  br.clear();
  struct F { int node, dad; };
  std::vector<F> st;
  if (target.is_list()) listtree::branches(r.target_shape, br);       // the walk from tip 1 that split_run's check of the target left
  else st.push_back(F{1, 0});
  while (!st.empty()) {                            // Engine::branch_order on the target's records
    const F f = st.back();
    st.pop_back();
    if (f.dad) br.push_back(NniBranch{f.dad, f.node});
    for (int s = (f.node > n_ ? 2 : 0); s >= 0; s--) {
      const int nb = target.back[3 * f.node + s] / 3;
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
int Engine::consensus_tree(const splitsets::TreeSet &set, const int32_t *weights, double threshold, splitsets::ListTree &out, int64_t *total)
{
  if (!(threshold >= 0.0 && threshold <= 1.0)) return bad("threshold must be in 0 .. 1");
  SplitRun &r = split_run_;
  int rc = split_run(set, weights, nullptr, true, threshold, r);
  if (rc) return rc;
  splitsets::apply_order(r.table, splitsets::order_splits(r.table));
  splitsets::build_lists(r.table, splitsets::greedy_compatible(r.table, threshold), out);
  if (total) *total = r.table.total;
  return MPF_OK;
}

// the same calls on record-format trees alone
namespace {
splitsets::TreeSet record_set(int n_trees, const int32_t *backs)
{
  splitsets::TreeSet s;
  s.n_records = n_trees;
  s.backs = backs;
  return s;
}
}  // namespace
int Engine::split_counts(int n_trees, const int32_t *backs, const int32_t *weights, splitsets::SplitTable &out)
{
  return split_counts(record_set(n_trees, backs), weights, out);
}
int Engine::split_support(int n_trees, const int32_t *backs, const int32_t *weights, const int32_t *target, std::vector<NniBranch> &br,
                          std::vector<int64_t> &support, int64_t *total)
{
  if (!target) return bad("null target tree");
  splitsets::TreeRef t;
  t.back = target;
  return split_support(record_set(n_trees, backs), weights, t, br, support, total);
}
int Engine::consensus_tree(int n_trees, const int32_t *backs, const int32_t *weights, double threshold, splitsets::ListTree &out, int64_t *total)
{
  return consensus_tree(record_set(n_trees, backs), weights, threshold, out, total);
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
