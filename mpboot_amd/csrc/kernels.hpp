// kernels.hpp -- launch interface of the gfx950 Fitch kernels (kernels.hip).
//
// Data layout in HBM: one "directional vector" per node record,
// stored at a compact slot index; a vector is S rows (one per state) of Wp 32-bit
// words, bit j of word i = "state k possible at site 32*i+j" -- the reference's
// parsVect row layout (sprparsimony.cpp:732-734, :2926-2927), site-major so that a
// wavefront reading one row touches 64*VW consecutive words (256 B .. 1 KiB).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>

#include "../host/list_tree.hpp"

namespace mpf {

// recompute dst = fitch(a, b); cnt[dst] += #sites with empty intersection   (K1, newview)
struct NvOp { uint32_t dst, a, b, pad; };

// popcount(~OR_k(a_k & b_k)) -> out[out]                                      (K2, evaluate)
struct EvOp { uint32_t a, b, out, pad; };

// one step of an SPR-scan program
//   kind 0  CHAIN : U[d] = fitch(U[d-1], vec[sib]); if test: out[out] += cost(fitch(U[d], vec[own]), S)
//   kind 1  ROOT  : U[0] = vec[own]
//   kind 2  JOIN  : out[out] += cost(fitch(vec[own], vec[sib]), S)            (stepwise addition)
struct ScanOp { uint32_t own, sib, meta, out; };   // meta = depth | test<<8 | kind<<16
struct ScanHdr { uint32_t op_begin, op_end, s_slot, pad /* bit 0: stepwise-addition program (the subtree s is the root side of every test) */; };

enum { SCAN_CHAIN = 0, SCAN_ROOT = 1, SCAN_JOIN = 2, SCAN_EVAL = 3 };   // EVAL (weighted kernels only): min_x(vec[sib][x] + m(S)[x]), the evaluate at a tip's edge

// device-walked scan: the kernel enumerates the neighbourhood of prune record x itself from the
// topology (back links) resident in HBM; candidate i of the scan lands in out[out_base + i] in the
// reference's DFS order, ncand[scan] = number of candidates
// All ids are compact vector slots ("cid"): tips 0..n-1, inner record 3v+s -> n + 3(v-n-1) + s.
// kids[cid] = cids of the two records behind an inner record (back[next], back[next next]).
struct WalkDesc { uint32_t s_cid, xa_cid, xb_cid, trav /* mintrav | maxtrav<<8 | side_mask<<16 | child_mask<<18 */,
                  out_base, pad0, pad1, pad2; };
constexpr int kWalkMaxDepth = 8;    // deepest device-walked scan (k_scan_walk); longer radii use the host-planned k_scan
constexpr int kMaxDepth = 12;   // deepest chain the register-resident scan kernel supports
// ... for 4- and 20-row tiles.  32-row tiles: 6 (thirteen of them do not fit a lane's 512 registers: k_scan<32, 1, 12> spilled);
// longer radii there take the HBM-scratch kernel like everything above kMaxDepth
constexpr int scan_reg_depth(int S, bool sankoff) { return sankoff ? (S != 4 ? 6 : kMaxDepth) : (S >= 32 ? 6 : kMaxDepth); }

struct Geometry {
  int S;        // states (4 | 20)
  int Wp;       // elements per row, multiple of 32 (Fitch: 32-site words; Sankoff: patterns)
  int vw;       // words per lane (1 | 2 | 4)
  int reduce;   // 0 = DPP wave reduction, 1 = ds_bpermute (__shfl) reduction
  int map;      // 0 = scan-major wave mapping, 1 = tiles pinned to XCD classes
  int big = 0;  // the vector store is 2 GiB or more: the scan kernel uses 64-bit addressing instead of one raw buffer
  int nv_pipe = 1;   // level-synchronous refresh, one word per lane: 1 = k_newview_wgq (operands requested a round ahead), 0 = k_newview_wgh
  // DNA, below 2 GiB: a second copy of every vector in WORD-major order (the four state words of a 32-site word side by side, 16 B)
  // `shoff` words behind the row-major store.  A CU loads 1 KB of it with ONE buffer_load_dwordx4 per wave at 124-146 GB/s, against
  // 75 GB/s for the four 256-byte row loads (tools/ubench/l1_rate: the load path inside the CU is what bounds the planned scan).
  // Written by k_pack_tips, k_newview_wgq and k_newview_chain; current for every valid vector while Engine::shadow_ok_ holds, and
  // then what the scans, the NNI / branch-length kernels and k_evaluate read.  The refresh kernels' word-major shapes also READ it
  // and leave the rows of what they write alone: the row-major store of the inner vectors is current only while Engine::rows_ok_
  // holds (launch_rows_from_wm brings it up to date on demand).  The tips are always current in both layouts.
  size_t shoff = 0;
  // radii above kMaxDepth (k_scan_deep): the scans' per-level up-vectors live in this scratch area (allocated on first use)
  uint32_t *deep_scratch = nullptr;
  size_t deep_scratch_words = 0;
  int nv_tile = 0;   // ... on tiles of 32 | 16 | 8 | 4 words (Wp / tile workgroups); 0 = chosen from Wp (newview_tile)
  // Sankoff (weighted parsimony) mode: vectors hold one 32-bit cost per state and pattern
  int sankoff = 0;
  const uint32_t *cost = nullptr;   // device, [S][S]
  const uint32_t *costT = nullptr;  // device, the transposed matrix; nullptr: the matrix is symmetric (see k_snk_scan)
  const uint32_t *pwgt = nullptr;   // device, [Wp] pattern weights (0 on padding)
  uint32_t highest_cost = 0;
  int snk16 = 0;                    // weighted mode: two 16-bit costs per lane (v_pk_add_u16 / v_pk_min_u16)
  size_t moff = 0;                  // words from a vector to its min-plus transform m(v) (second half of the vector array)
};

// The shapes in which launch_scan_prog / launch_scan_walk follow `word_major = true` and read the word-major copy; in every other
// shape they read rows whatever they are told.  The launchers and the engine (which must bring the rows up to date for a launch
// that reads them) both decide by these.
inline bool scan_prog_word_major(const Geometry &g) { return g.S == 4 && g.shoff != 0 && !g.big && g.vw == 1; }
inline bool scan_walk_word_major(const Geometry &g, int max_depth) { return g.S == 4 && g.shoff != 0 && !g.big && g.vw == 1 && max_depth <= kWalkMaxDepth; }

// ---------------------------------------------------------------- launch dispatch
// Each helper turns one runtime value into a compile-time constant (std::integral_constant, usable as a template argument) and
// calls f with it; f's result is returned.  A launch function names its kernel and arguments once, inside the innermost lambda.
template <int V> using int_c = std::integral_constant<int, V>;
template <bool V> using bool_c = std::integral_constant<bool, V>;

template <class F> decltype(auto) dispatch_bool(bool b, F &&f) { if (b) return f(bool_c<true>()); return f(bool_c<false>()); }
// state rows: 4 | 20 | 32 (anything else takes the 32-state kernels)
template <class F> decltype(auto) dispatch_states(int S, F &&f)
{
  if (S == 4) return f(int_c<4>());
  if (S == 20) return f(int_c<20>());
  return f(int_c<32>());
}
// (S, words per lane) of the Fitch kernels: several words per lane (2 | 4) for DNA only; 20 and 32 states run one
template <class F> decltype(auto) dispatch_sv(const Geometry &g, F &&f)
{
  if (g.S == 4) {
    if (g.vw == 1) return f(int_c<4>(), int_c<1>());
    if (g.vw == 2) return f(int_c<4>(), int_c<2>());
    return f(int_c<4>(), int_c<4>());
  }
  return dispatch_states(g.S, [&](auto S) { return f(S, int_c<1>()); });
}
// (S, two 16-bit costs per lane) of the weighted kernels
template <class F> decltype(auto) dispatch_snk(const Geometry &g, F &&f)
{
  return dispatch_states(g.S, [&](auto S) { return dispatch_bool(g.snk16 != 0, [&](auto PK) { return f(S, PK); }); });
}
// wave reduction: 0 = DPP, 1 = ds_bpermute
template <class F> decltype(auto) dispatch_reduce(const Geometry &g, F &&f) { if (g.reduce == 0) return f(int_c<0>()); return f(int_c<1>()); }
// depth class of a register-resident scan: 6, or DEEP for longer radii
template <int DEEP, class F> decltype(auto) dispatch_depth(int max_depth, F &&f) { if (max_depth <= 6) return f(int_c<6>()); return f(int_c<DEEP>()); }
// lane shape <KS, VW> of the climb and grow kernels (states per lane group, words per lane): DNA <1, vw> (vw 1 | 2 | 4 | 8), DNA in
// the word-major layout <4, 1> (a lane holds the four states of a word, 64-word tiles), 20 states <5, 1>, 32 states <8, 1>
template <class F> decltype(auto) dispatch_lane_shape(int S, int vw, bool word_major, F &&f)
{
  if (S == 4) {
    if (word_major) return f(int_c<4>(), int_c<1>());
    if (vw == 1) return f(int_c<1>(), int_c<1>());
    if (vw == 2) return f(int_c<1>(), int_c<2>());
    if (vw == 8) return f(int_c<1>(), int_c<8>());
    return f(int_c<1>(), int_c<4>());
  }
  if (S == 32) return f(int_c<8>(), int_c<1>());
  return f(int_c<5>(), int_c<1>());
}

// Opt-in of a kernel to dynamic LDS above 64 KiB: up to max_bytes of LDS per workgroup in all (the runtime refuses a dynamic
// maximum that leaves no room for the kernel's static LDS).  The attribute belongs to the process and the device, so it is set
// once per (kernel, device) for the whole process, before the kernel's first launch there (engines on several host threads share
// a device; engines of one process may sit on different GPUs)
template <auto Kernel> hipError_t lds_opt_in(int max_bytes)
{
  static std::atomic<bool> set[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool tracked = dev >= 0 && dev < 64;
  if (tracked && set[dev].load(std::memory_order_acquire)) return hipSuccess;
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(Kernel));
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes - (int)fa.sharedSizeBytes);
  if (e == hipSuccess && tracked) set[dev].store(true, std::memory_order_release);
  return e;
}

hipError_t launch_pack_tips(hipStream_t st, const Geometry &g, uint32_t *vec, const uint8_t *codes, int n_taxa,
                            int n_patterns, const int32_t *site2ptn, int n_sites, int datatype,
                            const uint32_t *tip_slots);
// cntp[tile][slot]: per-tile mutation counts of the recomputed vectors, folded by launch_cntsum into cnt[slot]
hipError_t launch_newview(hipStream_t st, const Geometry &g, uint32_t *vec, const NvOp *ops, int n_ops, uint32_t *cntp,
                          uint32_t nslots);
// chores a refresh launch does for the scan launch behind it on the stream: kids[kid_upd[3i]] = (kid_upd[3i+1], kid_upd[3i+2])
// (chained kernel only) and zero_ptr[0..zero_words) = 0
struct RefreshExtra { const uint32_t *kid_upd = nullptr; int n_kid_upd = 0; uint2 *kids = nullptr; uint32_t *zero_ptr = nullptr; uint32_t zero_words = 0;
                      uint32_t *cnt_host = nullptr; /* pinned host mirror of cnt[]: written by the in-kernel fold */
                      const int32_t *n_lev_ptr = nullptr; /* the schedule was made on the device (launch_sched): level count read from here */
                      // a device-planned sweep (launch_sched's descriptors): the DFS programs of its scan parts are written by EXTRA
                      // workgroups of the refresh launch (launch_newview_levels adds them; they also clear the scan's outputs), on CUs
                      // the refresh leaves idle -- no plan kernel on the critical path
                      const uint2 *wp_kids = nullptr; uint32_t wp_n = 0; const WalkDesc *wp_desc = nullptr; const uint32_t *wp_hdr = nullptr /* {parts, candidates} */;
                      void *wp_prog = nullptr; uint32_t *wp_out = nullptr; uint32_t wp_max_parts = 0;
                      uint32_t *shadow = nullptr; /* the word-major copy (Geometry::shoff; set by the launchers): every vector written goes there */
                      // DNA, one word per lane, the word-major copy current for every valid vector: the refresh reads its operands
                      // from that copy.  k_newview_wgq then writes no rows at all; k_newview_chain writes them while `rows` is set
                      // (the rows of every valid vector are current and shall stay so)
                      int wm_only = 0, rows = 0;
                      int waves_hint = 0; /* launch_newview_levels: waves per workgroup (0 = sixteen); narrow levels need fewer */
                      // launch_newview_self's in-kernel fold and launch_cntsum_slots: a pinned word (zeroed by the caller) that is
                      // set to 1 once every count is in cnt_host -- the host reads them while the launches behind still run
                      uint32_t *cnt_flag = nullptr; };
// Refresh schedule of a COMPLETE tree made on the device from the topology array alone (kids[cid], cids n .. n + n_ops - 1 are
// the inner records): ops in level order, lev_off[0 .. n_lev] as launch_newview_levels reads them, *n_lev.  One workgroup;
// trees of up to kSchedMaxSlots vectors.  Order inside a level is not defined (ops of a level are independent).
constexpr uint32_t kSchedMaxSlots = 16384;
// ... and, by a second workgroup of the same launch, the scan descriptors of a whole sweep (what Engine::plan_walk lays out on the
// host: per prune node the parts of its two neighbourhoods, their candidate counts N(q, maxtrav) and output offsets), radius <= 6
struct SweepDescArgs {
  const uint32_t *nodep = nullptr;   // cid of every prune record in sweep order; nullptr: no descriptors wanted
  uint32_t n_prune = 0, maxtrav = 0, split_cands = 0;
  WalkDesc *desc = nullptr;          // out: one per scan part, as launch_walk_plan / launch_scan_prog read them
  uint2 *parts = nullptr;            // out: (output offset, candidates) per part, for launch_part_min
  uint32_t *part_node = nullptr;     // out, pinned host memory: index of the prune node behind every part
  uint32_t *hdr_host = nullptr;      // out, pinned host memory: {parts, candidates, 0, flag raised behind everything}
  uint32_t *hdr_dev = nullptr;       // out, device memory: {parts, candidates} for the kernels that follow
};
// kids (and sw.nodep) may be PINNED HOST memory: the two workgroups read the 8 bytes per vector over the bus themselves (no copy
// dispatch in front of the launch); kids_copy != nullptr: the schedule workgroup leaves a copy in device memory for the kernels
// that follow
hipError_t launch_sched(hipStream_t st, const uint2 *kids, uint32_t n_taxa, uint32_t n_ops, NvOp *ops, int32_t *lev_off, int32_t *n_lev,
                        const SweepDescArgs &sw = SweepDescArgs(), uint2 *kids_copy = nullptr);
// The same refresh WITHOUT a schedule (k_newview_self): every refresh workgroup finds the levels of the complete tree itself, in LDS,
// from the device copy `kids` of the topology array, while its operands are on their way -- no launch_sched in front, no ops, no
// level offsets.  Tiles, data loop, counts (cntp[tile][slot], slots n_taxa .. n_taxa + n_ops) and the fold behind `done` as
// launch_newview_levels' one-word-per-lane kernel; x.wm_only as there.  sw.nodep != nullptr: one more workgroup lays out the
// sweep's scan descriptors beside the refresh, from the pinned array kids_host.  diag (device): {levels, 10 ns ticks workgroup 0
// needed for the topology and its first list -- the listing that no load overlaps --, ticks of the descriptor workgroup}.  Trees of
// up to kSchedMaxSlots vectors -- all that launch_sched takes.
bool newview_self_supported(const Geometry &g, uint32_t n_taxa, uint32_t n_ops);
hipError_t launch_newview_self(hipStream_t st, const Geometry &g, uint32_t *vec, const uint2 *kids, uint32_t n_taxa, uint32_t n_ops,
                               uint32_t *cntp, uint32_t nslots, uint32_t *cnt, uint32_t *done, int32_t *diag, const uint2 *kids_host,
                               const SweepDescArgs &sw, const RefreshExtra &x,
                               // both or neither: a further workgroup that only lists leaves the schedule as launch_sched would (ops
                               // by level, lev_off[0 .. levels]; the level count is diag[0]), for a replay by launch_newview_levels
                               NvOp *ops_out = nullptr, int32_t *lev_off_out = nullptr);
// dst[first .. first + count) = src[first .. first + count), one thread per record (src: pinned host memory)
hipError_t launch_kids_copy(hipStream_t st, const uint2 *src, uint2 *dst, uint32_t first, uint32_t count);
// launch_cntsum for the slots first .. first + n_ops; x.wp_desc != nullptr: further workgroups of the same launch plan the scan
// that follows and clear its outputs (x.wp_*, as they rode on launch_newview_levels).  x.cnt_flag needs x.cnt_host and `done`, a
// zeroed device word that is left zeroed
hipError_t launch_cntsum_slots(hipStream_t st, uint32_t first, int n_ops, const uint32_t *cntp, uint32_t nslots, uint32_t *cnt, int tiles,
                               const RefreshExtra &x, uint32_t *done = nullptr);
// every level in ONE launch (one 16-wave workgroup per tile, workgroup barrier between levels)
// Fitch mode also folds the per-tile counts into cnt[dst] (last workgroup; `done` = a zeroed device word, left zeroed);
// weighted mode leaves that to launch_cntsum
hipError_t launch_newview_levels(hipStream_t st, const Geometry &g, uint32_t *vec, const NvOp *ops, const int32_t *lev_off,
                                 int n_lev, uint32_t *cntp, uint32_t nslots, uint32_t *cnt, uint32_t *done,
                                 const RefreshExtra &x = RefreshExtra());
// the same refresh cut into chains (Fitch mode): ops laid out per (level, wave), wl_off[16 * n_lev + 1]; NvOp::a = 0xFFFFFFFF
// takes the previous op's result from registers
hipError_t launch_newview_chains(hipStream_t st, const Geometry &g, uint32_t *vec, const NvOp *ops, const int32_t *wl_off,
                                 int n_lev, int n_ops, uint32_t *cntp, uint32_t nslots, uint32_t *cnt, uint32_t *done,
                                 const RefreshExtra &x);
// pmin[i] = min(out[parts[i].x .. parts[i].x + parts[i].y)); pmin may be pinned host memory.  cnt_host != nullptr: cnt[0 .. n_cnt)
// is copied there as well; done != nullptr (a zeroed device word, left zeroed): pmin[n_parts] = 1 once everything is written
hipError_t launch_part_min(hipStream_t st, const uint32_t *out, const uint2 *parts, int n_parts, uint32_t *pmin,
                           const uint32_t *cnt = nullptr, uint32_t *cnt_host = nullptr, uint32_t n_cnt = 0, uint32_t *done = nullptr);
hipError_t launch_cntsum(hipStream_t st, const Geometry &g, const NvOp *ops, int n_ops, const uint32_t *cntp,
                         uint32_t nslots, uint32_t *cnt, int tiles = 0 /* 0 = tiles_for(g) */,
                         uint32_t *cnt_host = nullptr /* pinned host mirror of cnt[] */);
int tiles_for(const Geometry &g);
int newview_tile(const Geometry &g);
int tiles_for_levels(const Geometry &g);      // tiles (rows of cntp) launch_newview_levels uses: 32-word tiles for one word per lane
// word_major: read DNA from the word-major copy (Geometry::shoff), which the caller knows to be current
hipError_t launch_evaluate(hipStream_t st, const Geometry &g, const uint32_t *vec, const EvOp *ops, int n_ops,
                           uint32_t *out, bool word_major = false);
// rows of the listed vectors (slots[0 .. n_slots)) rewritten from their word-major copies (DNA with a word-major copy only)
hipError_t launch_rows_from_wm(hipStream_t st, const Geometry &g, uint32_t *vec, const uint32_t *slots, int n_slots);
// NNI scoring: the two moves of every branch (cids of the subtrees A, B at node1 and C0, C1 at node2; move k swaps A with C_k).
// out[i] (zeroed by the caller) = steps of move 0 | steps of move 1 << 32, the subtrees' own scores not included.
// vw = words per lane of the row-major store (1 | 2 | 4, DNA; other alphabets run 1); word_major: read DNA from the word-major
// copy (Geometry::shoff), which the caller knows to be current
struct NniDesc { uint32_t a, b, c0, c1; };
hipError_t launch_nni_eval(hipStream_t st, const Geometry &g, const uint32_t *vec, const NniDesc *desc, int n_br,
                           unsigned long long *out, int vw, bool word_major);
// ... for a tracked climb (k_nni_eval_masks): the same counts, and per branch i the per-site count 0..3 of "no common state" joins
// among the three joins the NNI changes, as two bit planes: row 3 i = the current tree's three joins (h), rows 3 i + 1 / 3 i + 2 =
// those of the tree after move 0 / move 1 (c_0, c_1); plane0 / plane1: [3 * n_br][Wp] words, sites in the order of launch_join_masks
hipError_t launch_nni_eval_masks(hipStream_t st, const Geometry &g, const uint32_t *vec, const NniDesc *desc, int n_br,
                                 unsigned long long *out, int vw, bool word_major, uint32_t *plane0, uint32_t *plane1);
// ... on the weighted engine (k_snk_nni_eval): the same descriptors; out[i] = the FULL weighted length after move 0 | after move 1
// << 32, rooted at the branch with node2's side as the parent (ParsTree::computeParsimonyBranch) -- nothing to add on the host.
// wide_addr: 64-bit pointers per row whatever the size of the store (what a transform half of 4 GiB and more takes by itself)
// vals / vmax (both or neither; the tracked climb, k_snk_nni_eval_vals): rows 2 i and 2 i + 1 of vals[][g.Wp] take the per-pattern
// lengths of the trees after move 0 / move 1 of branch i, 16 bits each, laid out as launch_scan's vals rows; *vmax the largest of them
hipError_t launch_snk_nni_eval(hipStream_t st, const Geometry &g, const uint32_t *vec, const NniDesc *desc, int n_br,
                               unsigned long long *out, bool wide_addr = false, uint16_t *vals = nullptr, uint32_t *vmax = nullptr);
// Parsimony branch lengths: every branch of the tree in one launch (cids of the two directional vectors of the branch; a tip's own
// vector at a pendant branch).  out[i] (zeroed by the caller) = number of sites whose two state sets have nothing in common
// (k_branch_subst; vw / word_major as launch_nni_eval)
// (BranchDesc: host/list_tree.hpp)
hipError_t launch_branch_subst(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                               uint32_t *out, int vw, bool word_major);
// ... on the weighted engine (k_snk_branch_eval): out[i] = the FULL weighted length of the tree rooted at branch i, a = the side
// that enters as it is (the parent side, the rows of the matrix), b = the side whose stored transform is read
// (ParsTree::computeParsimonyBranch's dad_branch / node_branch).  wide_addr as launch_snk_nni_eval
hipError_t launch_snk_branch_eval(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                                  uint32_t *out, bool wide_addr = false);
// what launch_scan dispatched for a weighted batch: wide = rows read through 64-bit pointers (k_snk_scan / k_snk_scan_deep
// <..., BUF = false>: a half of the store reaches 4 GiB, or the caller asked for wide addresses), deep = k_snk_scan_deep (more levels
// than the registers keep), launches = kernel launches the batch took (a deep batch is cut to the scratch)
struct SnkScanRan { int wide = 0, deep = 0, launches = 0; };
hipError_t launch_scan(hipStream_t st, const Geometry &g, const uint32_t *vec, const ScanHdr *hdr, int n_scans,
                       const ScanOp *ops, uint32_t *out, int max_depth,
                       uint32_t *host_out = nullptr, uint32_t n_out = 0, uint32_t *done = nullptr,   // as launch_scan_walk
                       // weighted mode, online UFBoot: vals[out index][npat] = per-pattern lengths of every tentative tree
                       // (16 bits each), *vmax = the largest of them (atomic max)
                       uint16_t *vals = nullptr, uint32_t npat = 0, uint32_t *vmax = nullptr,
                       bool wide_addr = false /* weighted mode: as launch_snk_nni_eval */,
                       SnkScanRan *ran = nullptr /* weighted mode: what was dispatched */);
hipError_t launch_scan_walk(hipStream_t st, const Geometry &g, const uint32_t *vec, const uint2 *kids, int n_taxa,
                            const WalkDesc *desc, int n_scans, uint32_t *out, uint32_t *ncand, int max_depth,
                            uint32_t *masks = nullptr, uint2 *info = nullptr,   // masks != nullptr: UFBoot variant (ufboot.hip)
                            // host_out != nullptr: the last workgroup copies out[0..n_out) to pinned host memory (done: zeroed word)
                            uint32_t *host_out = nullptr, uint32_t n_out = 0, uint32_t *done = nullptr,
                            bool word_major = false /* read the vectors from the word-major copy (Geometry::shoff): the caller knows it is current */);
// planned-program scan (radius <= 6, DNA): launch_walk_plan turns the descriptors into one DFS program per (scan part, gap end)
// -- WalkDesc::pad1 must hold the number of candidates behind the FIRST gap end (xa) of the part --, launch_scan_prog runs
// them with the children's vectors requested one expansion ahead.  Same outputs as launch_scan_walk.
hipError_t launch_walk_plan(hipStream_t st, const uint2 *kids, int n_taxa, const WalkDesc *desc, int n_scans, void *prog,
                            uint32_t *zero_ptr = nullptr, uint32_t zero_words = 0);   // zero_ptr: cleared by the same launch (the scan's outputs)
size_t scan_prog_bytes(int n_scans);
bool scan_prog_supported(const Geometry &g, int max_depth);
hipError_t launch_scan_prog(hipStream_t st, const Geometry &g, const uint32_t *vec, const WalkDesc *desc, int n_scans,
                            const void *prog, uint32_t *out, uint32_t *ncand, uint32_t *host_out = nullptr, uint32_t n_out = 0,
                            uint32_t *done = nullptr,
                            unsigned long long *trace = nullptr /* diagnostic: 4 words per workgroup (begin, end on the 100 MHz clock, where, what) */,
                            bool word_major = false /* read the vectors from the word-major copy (Geometry::shoff; the caller knows it is current) */);
size_t scan_prog_blocks(const Geometry &g, int n_scans);
// per-pattern Fitch lengths: ops = the (a, b) joins of a rooted traversal of the current tree; `planes` is
// scratch of site_planes_words() words; ptn_out[p] = length of pattern p (0 where first_site[p] < 0)
hipError_t launch_site_counts(hipStream_t st, const Geometry &g, const uint32_t *vec, const EvOp *ops, int n_ops,
                              uint32_t *planes, const int32_t *ptn_first_site, int n_ptn, uint16_t *ptn_out);
size_t site_planes_words(const Geometry &g, int n_ops);
// the bit-sliced per-site counters behind it: chunks of kPlaneChunk mask rows, kPlanes planes each ([chunk][plane][Wp] words);
// launch_pattern_sum reads every pattern's first site out of n_chunks of them (k_pattern_sum)
constexpr int kPlaneChunk = 63;
constexpr int kPlanes = 6;
hipError_t launch_pattern_sum(hipStream_t st, const Geometry &g, const uint32_t *planes, int n_chunks, const int32_t *ptn_first_site,
                              int n_ptn, uint16_t *ptn_out);

// Multifurcating trees (polytomy.hip; host/polytomy.cpp): every directed view of a tree given as neighbour lists, by the reference's
// k-ary rules.  An item is one node's accumulation over inputs[in_begin .. in_begin + n_in) (slots) followed by its outputs
// outs[out_begin .. out_begin + n_out): output = the rule over the inputs other than the vector in slot `excl` (0xFFFFFFFF: over all
// of them), stored at slot dst (0xFFFFFFFF: not stored) and, Fitch engine, its step mask ~OR_rows(AND) at masks[mask_row][Wp]
// (0xFFFFFFFF: none).  Items are laid out by level, lev_off[0 .. n_lev]; one launch, a workgroup barrier between levels.
// tile: words (elements) of a row per workgroup, 4 | 8 | 16 | 32; 0 = chosen from the row length (poly_tile)
// PolyItem and PolyOut are defined in host/list_tree.hpp, where the plan is made (listtree::plan_views)
int poly_tile(int W, int want);
hipError_t launch_poly_views(hipStream_t st, const Geometry &g, uint32_t *vec, const PolyItem *items, const PolyOut *outs,
                             const uint32_t *inputs, const int32_t *lev_off, int n_lev, uint32_t *masks, int tile);
// cnt[i] = set bits of mask row i
hipError_t launch_poly_rowsum(hipStream_t st, const Geometry &g, const uint32_t *masks, int n_rows, uint32_t *cnt);
// per-pattern Fitch lengths from the mask rows (planes: site_planes_words(g, n_rows) words of scratch), as launch_site_counts
hipError_t launch_poly_site_counts(hipStream_t st, const Geometry &g, const uint32_t *masks, int n_rows, uint32_t *planes,
                                   const int32_t *ptn_first_site, int n_ptn, uint16_t *ptn_out);

// Sankoff: per-pattern cost of the branch (a, b): ptn[j] = min_x(A[x] + min_y(cost[x][y] + B[y]))
hipError_t launch_sankoff_pattern(hipStream_t st, const Geometry &g, const uint32_t *vec, uint32_t a, uint32_t b,
                                  uint16_t *ptn_out, uint32_t *vmax = nullptr);
hipError_t launch_pack_tips_sankoff(hipStream_t st, const Geometry &g, uint32_t *vec, const uint8_t *codes, int n_taxa,
                                    int n_patterns, const int32_t *inf_index, int n_inf, int datatype);

}  // namespace mpf
