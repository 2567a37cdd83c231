// tbr_plan.hpp -- what a TBR (tree bisection and reconnection) visit is, as far as it follows from back[] alone.  Device-free: no HIP
// header, no engine; host/tbr.cpp and the stand-alone programs tests/tbr_plan_main.cpp and tests/tbr_book_main.cpp read it.
//
// There is no reference function: MPBoot has SPR and NNI only.  A visit is a record p, its edge (p, q = back[p]) and a radius.  Cut
// the edge; G lists the branches of p's part, F those of q's part, both as one_side of Engine::plan_scan enumerates them with
// mintrav = 1 (addTraverseParsimony's order, sprparsimony.cpp:2208-2218).  cost[i][j] is the length of the tree that joins the middle
// of F[i - 1] to the middle of G[j - 1]; index 0 of either side is "the part's own root", so row 0 and column 0 are the SPR tests of
// rearrangeParsimony (sprparsimony.cpp:2259-2376) and cost[0][0] is the tree as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "pair_tile.hpp"

namespace tbrplan {

inline int nx(int r) { return 3 * (r / 3) + (r % 3 + 1) % 3; }
inline bool tip(int n, int r) { return r / 3 <= n; }
// compact vector slot of a record (tips 0 .. n - 1, inner record 3 v + s -> n + 3 (v - n - 1) + s)
inline uint32_t slot(int n, int r) { const int v = r / 3; return v <= n ? (uint32_t)(v - 1) : (uint32_t)(n + 3 * (v - n - 1) + r % 3); }

// one step of a side's chain program, in the layout of the SPR scan's ScanOp (meta = depth | test << 8 | kind << 16):
//   ROOT  : U[0] = vec[own]
//   CHAIN : U[d] = fitch(U[d - 1], vec[sib]);  root set number `out` = fitch(U[d], vec[own])
// own and sib are vector slots, out counts the root sets of the program it belongs to
enum { OP_CHAIN = 0, OP_ROOT = 1 };
struct Op { uint32_t own, sib, meta, out; };

struct Side {
  std::vector<int32_t> rec, depth;        // the list, and how far each entry lies from the cut
  int max_depth = 0;
};

// one_side(x) of Engine::plan_scan with mintrav = 1: the list of x's part, and (ops != nullptr) its chain program appended to *ops
// with root sets numbered from out0
inline void side(int n, const int32_t *back, int x, int maxtrav, Side &s, std::vector<Op> *ops = nullptr, uint32_t out0 = 0)
{
  s.rec.clear();
  s.depth.clear();
  s.max_depth = 0;
  if (maxtrav > n - 3) maxtrav = n - 3;
  if (maxtrav < 1 || tip(n, x)) return;
  const int x1 = back[nx(x)], x2 = back[nx(nx(x))];
  if (tip(n, x1) && tip(n, x2)) return;
  struct Fr { int q, sib, d; };
  std::vector<Fr> st;
  for (int k = 0; k < 2; k++) {
    const int a = k ? x2 : x1, other = k ? x1 : x2;
    if (tip(n, a)) continue;
    if (ops) ops->push_back(Op{slot(n, other), 0u, (uint32_t)OP_ROOT << 16, 0u});
    st.push_back(Fr{back[nx(nx(a))], back[nx(a)], 1});
    st.push_back(Fr{back[nx(a)], back[nx(nx(a))], 1});
    while (!st.empty()) {
      const Fr f = st.back();
      st.pop_back();
      if (ops) ops->push_back(Op{slot(n, f.q), slot(n, f.sib), (uint32_t)f.d | (1u << 8) | ((uint32_t)OP_CHAIN << 16), out0 + (uint32_t)s.rec.size()});
      s.rec.push_back(f.q);
      s.depth.push_back(f.d);
      s.max_depth = std::max(s.max_depth, f.d);
      if (!tip(n, f.q) && f.d < maxtrav) {
        const int c1 = back[nx(f.q)], c2 = back[nx(nx(f.q))];
        st.push_back(Fr{c2, c1, f.d + 1});
        st.push_back(Fr{c1, c2, f.d + 1});
      }
    }
  }
}

// the two lists of a visit: F in q's part, G in p's part
struct Visit {
  int p = 0, q = 0;
  Side F, G;
  size_t rows() const { return 1 + F.rec.size(); }
  size_t cols() const { return 1 + G.rec.size(); }
  size_t vectors() const { return F.rec.size() + G.rec.size(); }      // root sets the visit keeps in the scratch store
};
inline void visit(int n, const int32_t *back, int p, int maxtrav, Visit &v)
{
  v.p = p;
  v.q = back[p];
  side(n, back, v.q, maxtrav, v.F);
  side(n, back, p, maxtrav, v.G);
}

// ---- the sweep in chunks: consecutive visits whose root sets together stay within `cap` vectors; a visit that needs more than
// that alone is a chunk of its own.  The matrices of a chunk stay within kChunkEntries entries in the same way (short rows: the vector
// cap alone would let them grow with the square of the lists).  -> [begin, end) per chunk
constexpr size_t kChunkEntries = (size_t)1 << 26;      // 256 MiB of costs
inline std::vector<std::pair<size_t, size_t>> chunks(const std::vector<size_t> &need, size_t cap, const std::vector<size_t> &entries,
                                                     size_t entry_cap = kChunkEntries)
{
  std::vector<std::pair<size_t, size_t>> out;
  size_t begin = 0, sum = 0, cells = 0;
  for (size_t i = 0; i < need.size(); i++) {
    if (i > begin && (sum + need[i] > cap || cells + entries[i] > entry_cap)) {
      out.push_back({begin, i});
      begin = i;
      sum = cells = 0;
    }
    sum += need[i];
    cells += entries[i];
  }
  if (need.size() > begin) out.push_back({begin, need.size()});
  return out;
}

// ---- tiles of the pair product (csrc/tbr.hip).  A workgroup owns tf rows x tg columns of one visit's matrix, in one of the two
// shapes of the taxon-insertion product: the rows of its table (pair_tile.hpp) for the engine kind, which k_tbr_costs is instantiated
// from too.  weighted: the weighted (-cost) engine, where 20 state rows take the 64 x 64 wide tile
enum { TILE_AUTO = mpf::PLACE_AUTO, TILE_NARROW = mpf::PLACE_NARROW, TILE_WIDE = mpf::PLACE_WIDE };
struct TileDims { int tf, tg; };
constexpr TileDims tile_dims(int S, int shape, bool weighted = false)
{
  return TileDims{mpf::place_shape(S, weighted, shape).tq, mpf::place_shape(S, weighted, shape).tb};
}
constexpr size_t tiles_of(size_t rows, size_t cols, TileDims d) { return ((rows + (size_t)d.tf - 1) / (size_t)d.tf) * ((cols + (size_t)d.tg - 1) / (size_t)d.tg); }
// TILE_AUTO: the shape whose tiles cover fewer outputs, padding included.  A wide lane holds 4 x 4 (2 x 2) outputs and reads each
// staged word once for four (two) of them, a narrow lane holds 4 x 1: a narrow output is charged twice
// On the weighted engine that rule lost: a wide workgroup walks the whole row alone (a weighted row is 16 to 32 times as long as the
// Fitch row of the same alignment), so a wide launch takes that long however few tiles it has, while the narrow shape's time grows
// with the outputs.  Measured on whole sweeps (profiles/tbr/timing_weighted.json): the forced narrow shape took a third
// of the rule's time at radius 6 and was never slower, the forced wide shape 6 to 17 times the narrow one's.  TILE_AUTO there is
// narrow below kWeightedWideFrom entries of the visit's own matrix -- near where taxon insertion's two weighted shapes cross
// (2.45e5 to 3.5e5 outputs; no TBR visit of that size has been timed) -- and wide from there on
constexpr size_t kWeightedWideFrom = (size_t)1 << 18;
inline int pick(int S, size_t rows, size_t cols, int tile, bool weighted = false)
{
  if (tile == TILE_NARROW || tile == TILE_WIDE) return tile;
  if (weighted) return rows * cols < kWeightedWideFrom ? TILE_NARROW : TILE_WIDE;
  const TileDims a = tile_dims(S, TILE_NARROW, weighted), w = tile_dims(S, TILE_WIDE, weighted);
  const size_t narrow = 2 * tiles_of(rows, cols, a) * (size_t)(a.tf * a.tg), wide = tiles_of(rows, cols, w) * (size_t)(w.tf * w.tg);
  return narrow < wide ? TILE_NARROW : TILE_WIDE;
}
struct Item { uint32_t visit, ft, gt, pad; };        // visit: index within the chunk; tile (ft, gt) of its matrix
inline void tiles(uint32_t visit, size_t rows, size_t cols, TileDims d, std::vector<Item> &out)
{
  if (rows * cols <= 1) return;                      // (a 1 x 1 matrix: the tree as it is, nothing to score)
  for (size_t ft = 0; ft * (size_t)d.tf < rows; ft++)
    for (size_t gt = 0; gt * (size_t)d.tg < cols; gt++) out.push_back(Item{visit, (uint32_t)ft, (uint32_t)gt, 0u});
}

// ---- a sweep under a UFBoot tracker (host/tbr.cpp).  Every entry of every visit's matrix is handed to the tracker: the visits in
// sweep order, a visit's entries in row-major order from [0][0] (the tree as it is).  A batch is a stretch of that sequence of at
// most `cap` entries; the part of one visit that falls into a batch is a run.  A visit larger than what is left of a batch goes on in
// the next one, so a large visit is booked in consecutive blocks of its matrix, wherever in a row a block may end.
struct BookRun { uint32_t visit, pad; uint64_t begin, end; };      // entries [begin, end) of the visit's matrix, row-major
// entries[v] = rows x columns of visit v  ->  runs, and off: batch b is runs[off[b] .. off[b + 1])
inline void book_batches(const std::vector<size_t> &entries, size_t cap, std::vector<BookRun> &runs, std::vector<size_t> &off)
{
  runs.clear();
  off.assign(1, 0);
  if (cap < 1) cap = 1;
  size_t room = cap;
  for (size_t v = 0; v < entries.size(); v++)
    for (size_t at = 0; at < entries[v];) {
      if (!room) { off.push_back(runs.size()); room = cap; }
      const size_t take = std::min(room, entries[v] - at);
      runs.push_back(BookRun{(uint32_t)v, 0u, (uint64_t)at, (uint64_t)(at + take)});
      at += take;
      room -= take;
    }
  if (!runs.empty()) off.push_back(runs.size());
}

// The automatic batch cap of a tracked sweep on the weighted engine (k_tbr_snk_vals, csrc/tbr.hip): the most entries of a batch such
// that its 16-bit rows (npat values each), its K bit planes (plane_words words a row) and its product C (samples_p sums a row) each
// stay within `limit` bytes.  mask_rows gives a batch of c entries at most 2 c rows (every run that has a home row has an entry that
// takes part), and the planes and C are padded to whole row tiles: the cap is half the largest multiple of row_tile rows that fits.
// K is not known before the kernel has run; value_bits bounds it on the host: every value is at most `top` (n_taxa x highest_cost,
// k_tbr_snk_vals's comment), K is the number of bits of the largest value written and never more than 16
inline int value_bits(uint64_t top)
{
  int k = 1;
  while (k < 16 && (top >> k)) k++;
  return k;
}
inline size_t book_cap(size_t npat, size_t plane_words, size_t samples_p, int k_bits, size_t row_tile, size_t limit = (size_t)256 << 20)
{
  const size_t per_row = std::max(std::max(npat * sizeof(uint16_t), (size_t)k_bits * plane_words * sizeof(uint32_t)), samples_p * sizeof(uint32_t));
  const size_t rows = (limit / std::max<size_t>(per_row, 1)) / row_tile * row_tile;
  return std::max<size_t>(1, rows / 2);
}

// The mask rows one batch needs (k_tbr_masks, csrc/tbr.hip): one per entry that takes part, and per run with such an entry the
// visit's home row M[0][0] in front of them -- also where the run begins behind [0][0].  Entry [0][0] itself never takes a row of its
// own (it is the current tree).  A MaskRun is one matrix row of one visit with at most kMaskRunCols listed columns: one wave's work.
// take[c]: entry c of the batch, counted through its runs, takes part.  -> rows used; crow[c] = the row of entry c, home[r] = the home
// row of run r, kNoRow where there is none
constexpr uint32_t kNoRow = 0xFFFFFFFFu, kMaskRunCols = 32;
struct MaskRun { uint32_t visit, row, begin, end; };      // columns cols[begin .. end)
struct MaskCol { uint32_t col, out; };                    // column of the matrix, output row
inline uint32_t mask_rows(const BookRun *runs, size_t n_runs, const uint32_t *ncols /* by visit */, const uint8_t *take,
                          std::vector<MaskRun> &mr, std::vector<MaskCol> &mc, std::vector<uint32_t> &crow, std::vector<uint32_t> &home)
{
  mr.clear();
  mc.clear();
  crow.clear();
  home.assign(n_runs, kNoRow);
  uint32_t rows = 0;
  size_t c = 0;
  auto add = [&](uint32_t visit, uint32_t row, uint32_t col, uint32_t out) {
    if (mr.empty() || mr.back().visit != visit || mr.back().row != row || mr.back().end - mr.back().begin >= kMaskRunCols)
      mr.push_back(MaskRun{visit, row, (uint32_t)mc.size(), (uint32_t)mc.size()});
    mc.push_back(MaskCol{col, out});
    mr.back().end = (uint32_t)mc.size();
  };
  for (size_t r = 0; r < n_runs; r++) {
    const BookRun &run = runs[r];
    const uint64_t ng = ncols[run.visit];
    for (uint64_t e = run.begin; e < run.end; e++, c++) {
      crow.push_back(kNoRow);
      if (e == 0 || !take[c]) continue;
      if (home[r] == kNoRow) { home[r] = rows; add(run.visit, 0u, 0u, rows++); }
      crow.back() = rows;
      add(run.visit, (uint32_t)(e / ng), (uint32_t)(e % ng), rows++);
    }
  }
  return rows;
}

// ---- the edit.  removeNodeParsimony + insertParsimony (sprparsimony.cpp:2245-2257, :1942-1952) on back[]: the node of record p leaves
// its place and goes into the middle of branch (g, back g)
inline void apply_spr(int32_t *back, int p, int g)
{
  const int a1 = back[nx(p)], a2 = back[nx(nx(p))];
  back[a1] = a2;
  back[a2] = a1;
  const int r = back[g];
  back[nx(p)] = g;
  back[g] = nx(p);
  back[nx(nx(p))] = r;
  back[r] = nx(nx(p));
}
// cut (p, q = back[p]) and join the middle of f (q's part; -1: its own root) to the middle of g (p's part; -1 likewise): two SPR
// steps on disjoint links
inline void apply(int32_t *back, int p, int f, int g)
{
  const int q = back[p];
  if (g >= 0) apply_spr(back, p, g);
  if (f >= 0) apply_spr(back, q, f);
}

// first minimum of a matrix in row-major order, entry [0][0] left out: (value, index), index = SIZE_MAX for a 1 x 1 matrix
inline std::pair<uint32_t, size_t> first_min(const uint32_t *cost, size_t count)
{
  std::pair<uint32_t, size_t> best{0xFFFFFFFFu, (size_t)-1};
  for (size_t i = 1; i < count; i++)
    if (best.second == (size_t)-1 || cost[i] < best.first) best = {cost[i], i};
  return best;
}

}  // namespace tbrplan
