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

#include "../csrc/engine.hpp"

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

int Engine::nni_check(int root_taxon) const
{
  // the weighted climb skips the rollback (iqtree.cpp:2258) and an attached tracker would have to book every NNI
  // (saveCurrentTree from getBestNNIForBran, phylotree.cpp:3937): neither is served
  if (sankoff_) { set_error("NNI climb: Fitch engines only (the -cost climb is not served)"); return MPF_E_UNSUPPORTED; }
  if (ufb_) { set_error("NNI climb: not served with a UFBoot tracker attached"); return MPF_E_UNSUPPORTED; }
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
int Engine::nni_eval(const std::vector<NniBranch> &br, std::vector<uint32_t> &len, std::vector<NniSwap> *moves)
{
  if (!views_valid_) { int rc = update_views(); if (rc) return rc; }
  const size_t nb = br.size();
  len.assign(2 * nb, 0u);
  if (moves) moves->assign(2 * nb, NniSwap{0, 0, 0, 0});
  if (!nb) return MPF_OK;
  HIPCHK(h_nni_desc_.reserve(nb));
  HIPCHK(d_nni_desc_.reserve(nb));
  HIPCHK(h_nni_out_.reserve(nb));
  HIPCHK(d_nni_out_.reserve(nb));
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
    base[i] = score(ra) + score(rb) + score(rc0) + score(rc1);
    if (moves) {
      (*moves)[2 * i] = NniSwap{v1, s1[0], v2, s2[0]};
      (*moves)[2 * i + 1] = NniSwap{v1, s1[0], v2, s2[1]};
    }
  }
  bool wm = nni_vw_ <= 0 && g_.S == 4 && g_.shoff && shadow_ok_;
  int vw = nni_vw_ > 0 ? nni_vw_ : (nni_vw_ == 0 ? 1 : g_.vw);
  HIPCHK(hipMemcpyAsync(d_nni_desc_.p, h_nni_desc_.p, nb * sizeof(NniDesc), hipMemcpyHostToDevice, st_));
  HIPCHK(hipMemsetAsync(d_nni_out_.p, 0, nb * sizeof(unsigned long long), st_));
  HIPCHK(launch_nni_eval(st_, g_, d_vec_, d_nni_desc_.p, (int)nb, d_nni_out_.p, vw, wm));
  HIPCHK(hipMemcpyAsync(h_nni_out_.p, d_nni_out_.p, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, st_));
  HIPCHK(hipStreamSynchronize(st_));
  for (size_t i = 0; i < nb; i++) {
    const unsigned long long o = h_nni_out_.p[i];
    len[2 * i] = base[i] + (uint32_t)(o & 0xFFFFFFFFull);
    len[2 * i + 1] = base[i] + (uint32_t)(o >> 32);
  }
  nni_launches_++;
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
  if (max_steps < 0) { set_error("NNI climb: max_steps must be >= 0"); return MPF_E_INVALID; }
  nni_log_.clear();
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
      rc = nni_eval(br, len, &mv);
      if (rc) return rc;
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
    if (cur <= chosen[0].len) {
      count += num_nnis;
      rollback = false;
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

}  // namespace mpf
