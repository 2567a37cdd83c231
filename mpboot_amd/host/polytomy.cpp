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
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
int bad(const std::string &what) { set_error("polytomy tree: " + what); return MPF_E_INVALID; }
}  // namespace

// (splitsets::lists_ok of host/split_sets.hpp restates these conditions device-free for the mpf_*_set calls: change both together.)
// The checks of the hand-over (include/mpfitch.h) and the rooted shape: parent and pre-order of every node from the root leaf,
// neighbours in list order (fixNegativeBranch's walk: FOR_NEIGHBOR_IT(node, dad, it))
int Engine::polytomy_check(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, PolyTree &t, bool absent_tips) const
{
  const int n = n_;
  if (!first || !nbr) return bad("null neighbour lists");
  if (n_inner < 1 || n_inner > n - 2) return bad("n_inner must be in 1 .. n_taxa - 2");
  if (root_taxon < 1 || root_taxon > n) return bad("root_taxon must be in 1 .. n_taxa");
  if (first[0] != 0) return bad("first[0] must be 0");
  const int N = n + n_inner;
  for (int i = 0; i < n_inner; i++)
    if (first[i + 1] - first[i] < 3) return bad("inner node " + std::to_string(n + 1 + i) + " has fewer than three neighbours");
  const int64_t E = first[n_inner];
  if (E > 3 * (int64_t)(n - 2)) return bad("more neighbour entries than a tree of n_taxa leaves can have");
  t.tip_nb.assign((size_t)n + 1, 0);
  std::vector<std::pair<int32_t, int32_t>> arcs;       // inner -> inner, for the symmetry check
  for (int i = 0; i < n_inner; i++)
    for (int k = first[i]; k < first[i + 1]; k++) {
      const int u = nbr[k], v = n + 1 + i;
      if (u < 1 || u > N) return bad("neighbour number out of range");
      if (u == v) return bad("a node is its own neighbour");
      if (u <= n) {
        if (t.tip_nb[(size_t)u]) return bad("tip " + std::to_string(u) + " occurs more than once");
        t.tip_nb[(size_t)u] = v;
      } else arcs.emplace_back(v, u);
    }
  int m = 0;                                             // tips that occur
  for (int u = 1; u <= n; u++) {
    if (t.tip_nb[(size_t)u]) m++;
    else if (!absent_tips) return bad("tip " + std::to_string(u) + " does not occur");
  }
  if (!t.tip_nb[(size_t)root_taxon]) return bad("root_taxon does not occur");
  std::sort(arcs.begin(), arcs.end());
  for (size_t i = 0; i < arcs.size(); i++) {
    if (i && arcs[i] == arcs[i - 1]) return bad("a neighbour is listed twice");
    if (!std::binary_search(arcs.begin(), arcs.end(), std::make_pair(arcs[i].second, arcs[i].first))) return bad("adjacency is not symmetric");
  }
  if ((int64_t)m + (int64_t)arcs.size() / 2 != (int64_t)(m + n_inner) - 1) return bad("not n_taxa + n_inner - 1 edges");
  // pre-order from the root leaf
  t.parent.assign((size_t)N + 1, -1);
  t.order.clear();
  t.order.reserve((size_t)N);
  std::vector<int32_t> st{root_taxon};
  t.parent[(size_t)root_taxon] = 0;
  {
    const int r0 = t.tip_nb[(size_t)root_taxon];
    t.order.push_back(root_taxon);
    t.parent[(size_t)r0] = root_taxon;
    st.assign(1, r0);
  }
  while (!st.empty()) {
    const int v = st.back();
    st.pop_back();
    t.order.push_back(v);
    if (v <= n) continue;
    const int i = v - n - 1;
    for (int k = first[i + 1] - 1; k >= first[i]; k--) {
      const int u = nbr[k];
      if (u == t.parent[(size_t)v]) continue;
      if (t.parent[(size_t)u] >= 0) return bad("the neighbour lists hold a cycle");
      t.parent[(size_t)u] = v;
      st.push_back(u);
    }
  }
  if ((int)t.order.size() != m + n_inner) return bad("the tree is not connected");
  return MPF_OK;
}

// items of the view launch: up views by height, the root edge (Fitch), down views by depth
int Engine::polytomy_views(int n_inner, const int32_t *first, const int32_t *nbr, int root_taxon, bool all_views, PolyTree &t, bool absent_tips)
{
  int rc = polytomy_check(n_inner, first, nbr, root_taxon, t, absent_tips);
  if (rc) return rc;
  const int n = n_, N = n + n_inner;
  // whatever the engine's own tree has under way is finished first; its vectors are about to be overwritten
  if (cnt_copy_pending_) {
    HIPCHK(hipMemcpyAsync(h_cnt(), d_cnt(), nslots_ * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    cnt_copy_pending_ = false;
  }
  HIPCHK(hipStreamSynchronize(st_));
  finish_views();
  invalidate_vectors();
  // slots: a tip keeps its own; the view of inner node i towards its k-th neighbour (list position first[i] + k) is n + first[i] + k
  // the parent's position in every inner node's list
  std::vector<int32_t> ppos((size_t)N + 1, -1), height((size_t)N + 1, 0), depth((size_t)N + 1, 0);
  for (int v = n + 1; v <= N; v++) {
    const int i = v - n - 1;
    for (int k = first[i]; k < first[i + 1]; k++)
      if (nbr[k] == t.parent[(size_t)v]) ppos[(size_t)v] = k;
    if (ppos[(size_t)v] < 0) return bad("inconsistent neighbour lists");
  }
  // slot of the view of neighbour u TOWARDS inner node v (an input of v): a tip's own vector, the up view of a child, the down
  // view of the parent -- the latter sits at the parent's entry for v, found through v's position in the parent's list
  std::vector<int32_t> cpos((size_t)N + 1, -1);         // position of inner node v in its parent's list
  for (int v = n + 1; v <= N; v++) {
    const int i = v - n - 1;
    for (int k = first[i]; k < first[i + 1]; k++) {
      const int u = nbr[k];
      if (u > n && t.parent[(size_t)u] == v) cpos[(size_t)u] = k;
    }
  }
  int maxh = 0, maxd = 0;
  for (size_t q = t.order.size(); q-- > 0;) {
    const int v = t.order[q];
    if (v == root_taxon) continue;
    const int p = t.parent[(size_t)v];
    if (p != root_taxon) height[(size_t)p] = std::max(height[(size_t)p], height[(size_t)v] + 1);
    maxh = std::max(maxh, height[(size_t)v]);
  }
  for (int v : t.order) {
    if (v <= n || t.parent[(size_t)v] == root_taxon) continue;
    depth[(size_t)v] = depth[(size_t)t.parent[(size_t)v]] + 1;
    maxd = std::max(maxd, depth[(size_t)v]);
  }
  const int r0 = t.tip_nb[(size_t)root_taxon];
  // levels: [0, maxh) up views by height - 1; maxh: the root edge; maxh + 1 + depth: down views
  const int n_lev = all_views ? maxh + 2 + maxd : maxh + 1;
  std::vector<int32_t> lev_cnt((size_t)n_lev + 1, 0);
  auto up_level = [&](int v) { return height[(size_t)v] - 1; };
  auto down_level = [&](int v) { return maxh + 1 + depth[(size_t)v]; };
  for (int v = n + 1; v <= N; v++) {
    lev_cnt[(size_t)up_level(v)]++;
    if (all_views) lev_cnt[(size_t)down_level(v)]++;
  }
  if (!sankoff_) lev_cnt[(size_t)maxh]++;
  t.lev_off.assign((size_t)n_lev + 1, 0);
  for (int l = 0; l < n_lev; l++) t.lev_off[(size_t)l + 1] = t.lev_off[(size_t)l] + lev_cnt[(size_t)l];
  const size_t n_items = (size_t)t.lev_off[(size_t)n_lev];
  t.items.assign(n_items, PolyItem{0, 0, 0, 0});
  t.outs.clear();
  t.inputs.clear();
  std::vector<int32_t> fill(t.lev_off.begin(), t.lev_off.end() - 1);
  t.n_rows = 0;
  t.up_slot.assign((size_t)N + 1, kNoSlot);
  for (int v = 1; v <= n; v++) t.up_slot[(size_t)v] = (uint32_t)(v - 1);
  for (int v = n + 1; v <= N; v++) t.up_slot[(size_t)v] = (uint32_t)(n + ppos[(size_t)v]);
  auto input_of = [&](int v, int k) -> uint32_t {       // the view of v's k-th neighbour towards v
    const int u = nbr[k];
    if (u <= n) return (uint32_t)(u - 1);
    if (u == t.parent[(size_t)v]) return (uint32_t)(n + cpos[(size_t)v]);
    return t.up_slot[(size_t)u];
  };
  for (int v = n + 1; v <= N; v++) {
    const int i = v - n - 1;
    // up: the rule over the children, one output towards the parent; its step mask is a row of the tree's per-site count
    PolyItem up{(uint32_t)t.inputs.size(), 0, (uint32_t)t.outs.size(), 1};
    for (int k = first[i]; k < first[i + 1]; k++)
      if (k != ppos[(size_t)v]) t.inputs.push_back(input_of(v, k));
    up.n_in = (uint32_t)t.inputs.size() - up.in_begin;
    t.outs.push_back(PolyOut{t.up_slot[(size_t)v], kNoSlot, sankoff_ ? kNoSlot : (uint32_t)t.n_rows++, 0});
    t.items[(size_t)fill[(size_t)up_level(v)]++] = up;
    if (!all_views) continue;
    // down: accumulators over all d inputs, one output towards every child (the rule over the other d - 1 inputs)
    PolyItem dn{(uint32_t)t.inputs.size(), 0, (uint32_t)t.outs.size(), 0};
    for (int k = first[i]; k < first[i + 1]; k++) t.inputs.push_back(input_of(v, k));
    dn.n_in = (uint32_t)t.inputs.size() - dn.in_begin;
    for (int k = first[i]; k < first[i + 1]; k++)
      if (k != ppos[(size_t)v]) t.outs.push_back(PolyOut{(uint32_t)(n + k), input_of(v, k), kNoSlot, 0});
    dn.n_out = (uint32_t)t.outs.size() - dn.out_begin;
    t.items[(size_t)fill[(size_t)down_level(v)]++] = dn;
  }
  if (!sankoff_) {
    // computeParsimonyBranch(root->neighbors[0], root): the root leaf against the rest of the tree, a two-input node that stores
    // no vector
    PolyItem re{(uint32_t)t.inputs.size(), 2, (uint32_t)t.outs.size(), 1};
    t.inputs.push_back((uint32_t)(root_taxon - 1));
    t.inputs.push_back(t.up_slot[(size_t)r0]);
    t.outs.push_back(PolyOut{kNoSlot, kNoSlot, (uint32_t)t.n_rows++, 0});
    t.items[(size_t)fill[(size_t)maxh]++] = re;
  }
  // one upload: items | outs | inputs | level offsets
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_items = 0, o_outs = al(o_items + n_items * sizeof(PolyItem)), o_in = al(o_outs + t.outs.size() * sizeof(PolyOut)),
               o_lev = al(o_in + t.inputs.size() * sizeof(uint32_t)), bytes = al(o_lev + t.lev_off.size() * sizeof(int32_t));
  HIPCHK(h_poly_stage_.reserve(bytes));
  HIPCHK(d_poly_stage_.reserve(bytes));
  std::memcpy(h_poly_stage_.p + o_items, t.items.data(), n_items * sizeof(PolyItem));
  std::memcpy(h_poly_stage_.p + o_outs, t.outs.data(), t.outs.size() * sizeof(PolyOut));
  std::memcpy(h_poly_stage_.p + o_in, t.inputs.data(), t.inputs.size() * sizeof(uint32_t));
  std::memcpy(h_poly_stage_.p + o_lev, t.lev_off.data(), t.lev_off.size() * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(d_poly_stage_.p, h_poly_stage_.p, bytes, hipMemcpyHostToDevice, st_));
  if (!sankoff_) HIPCHK(d_poly_masks_.reserve((size_t)t.n_rows * (size_t)g_.Wp));
  if (timing_) HIPCHK(hipEventRecord(ev0_, st_));
  HIPCHK(launch_poly_views(st_, g_, vec_rows(), reinterpret_cast<const PolyItem *>(d_poly_stage_.p + o_items),
                           reinterpret_cast<const PolyOut *>(d_poly_stage_.p + o_outs), reinterpret_cast<const uint32_t *>(d_poly_stage_.p + o_in),
                           reinterpret_cast<const int32_t *>(d_poly_stage_.p + o_lev), n_lev, d_poly_masks_.p, poly_tile_));
  if (timing_) HIPCHK(hipEventRecord(ev1_, st_));
  poly_view_timed_ = timing_ != 0;
  poly_launches_++;
  poly_views_ += t.outs.size() - (sankoff_ ? 0 : 1);
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
  const uint32_t rest = t.up_slot[(size_t)t.tip_nb[(size_t)root_taxon]], leaf = (uint32_t)(root_taxon - 1);
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
    const size_t rows = (size_t)t.n_rows;
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
  br.clear();
  for (int v : t.order)
    if (v != root_taxon) br.push_back(NniBranch{t.parent[(size_t)v], v});
  const size_t nb = br.size();
  subst.assign(nb, 0u);
  HIPCHK(h_br_desc_.reserve(nb));
  HIPCHK(d_br_desc_.reserve(nb));
  HIPCHK(h_br_out_.reserve(nb));
  HIPCHK(d_br_out_.reserve(nb));
  // position of every inner child in its parent's list: the parent's down view towards it
  std::vector<uint32_t> down((size_t)n + (size_t)n_inner + 1, kNoSlot);
  for (int i = 0; i < n_inner; i++)
    for (int k = first[i]; k < first[i + 1]; k++)
      if (t.parent[(size_t)nbr[k]] == n + 1 + i) down[(size_t)nbr[k]] = (uint32_t)(n + k);
  for (size_t i = 0; i < nb; i++) {
    const int v1 = br[i].node1, v2 = br[i].node2;
    const uint32_t rest = v1 <= n ? (uint32_t)(v1 - 1) : down[(size_t)v2];       // the rest of the tree seen from node2
    const uint32_t sub = t.up_slot[(size_t)v2];                                  // the subtree at node2 (a leaf: its own vector)
    if (rest == kNoSlot || sub == kNoSlot) { set_error("polytomy tree: inconsistent walk"); return MPF_E_STATE; }
    // the orientation of Engine::branch_substitutions (parstree.cpp:439-541 and the leaf swap at :449-457)
    if (sankoff_ && v2 <= n) h_br_desc_.p[i] = BranchDesc{rest, sub};
    else h_br_desc_.p[i] = BranchDesc{sub, rest};
  }
  const int vw = brlen_vw_ > 0 ? brlen_vw_ : (brlen_vw_ == 0 ? 1 : g_.vw);       // (the row-major store only: no word-major copy of these views)
  HIPCHK(hipMemcpyAsync(d_br_desc_.p, h_br_desc_.p, nb * sizeof(BranchDesc), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(d_br_out_.p, 0, nb * sizeof(uint32_t), st_));
  if (timing_) HIPCHK(hipEventRecord(ev2_, st_));
  if (sankoff_) HIPCHK(launch_snk_branch_eval(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, force_big_ != 0));
  else HIPCHK(launch_branch_subst(st_, g_, vec_rows(), d_br_desc_.p, (int)nb, d_br_out_.p, vw, false));
  if (timing_) HIPCHK(hipEventRecord(ev3_, st_));
  HIPCHK(hipMemcpyAsync(h_br_out_.p, d_br_out_.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
  const size_t rows = (size_t)t.n_rows;
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
