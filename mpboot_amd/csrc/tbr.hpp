// tbr.hpp -- launch interface of the TBR kernels (tbr.hip; host/tbr.cpp; the plan of a visit: host/tbr_plan.hpp).
//
// There is no reference function (MPBoot has SPR and NNI).  Cut the edge (p, q = back[p]).  The part on p's side, rooted on a branch
// (g, back g) inside it, shows R_p(g) = fitch(U(g), vec[g]), U the chain of the SPR scan: U(child) = fitch(U(parent), vec[sibling]),
// U(x1) = vec[x2], U(x2) = vec[x1] for p's children; rooted on its own merged edge it shows vec[p].  The same on q's side.  The tree
// that joins the middle of f to the middle of g has length sc[p] + sc[q] + #sites where R_q(f) and R_p(g) share no state.
//
// On the weighted engine (symmetric cost matrices), m() the stored min-plus transform: MU(x1) = m(vec[x2]), MU(child) = m(MU(parent) +
// m(vec[sibling])), R_p(g) = MU(g) + m(vec[g]); the joined tree has the FULL length sum_ptn w * min_x(R_q(f)[x] + m(R_p(g))[x]), no
// base.  The root sets of p's part (the columns) are stored transformed; column 0 is the stored transform of vec[p].
#pragma once
#include "kernels.hpp"
#include "../host/tbr_plan.hpp"

namespace mpf {

// levels of U that k_tbr_roots keeps in LDS (a level is S rows x 64 words); deeper levels live in HBM scratch
constexpr int tbr_lds_levels(int S) { return S == 4 ? 16 : 7; }      // 16 KiB | 35 KiB (20 rows) | 56 KiB (32 rows)

// words of a row of the store and of the scratch store: Wp site words; on the weighted engine We elements, one per pattern or, in
// the 16-bit store, one per pair of patterns.  A vector is S rows
inline int tbr_row_words(const Geometry &g) { return g.sankoff && g.snk16 ? g.Wp / 2 : g.Wp; }

// one side of a visit: its chain program ops[op_begin .. op_end) and where its levels beyond the LDS ones go: `deep_levels` levels
// per site tile, `deep_off` words into the scratch area.  pad bit 0 (weighted engine): a side of G, its root sets are stored transformed
struct TbrSide { uint32_t op_begin, op_end, deep_levels, pad; uint64_t deep_off; };
// one visit of the pair product: row i of its matrix reads vec slot_q (i = 0) or root set f0 + i - 1 of the scratch store, column j
// vec slot_p or root set g0 + j - 1; cost[i][j] goes to out[at + i * ng + j] with base = sc[p] + sc[q] added
struct TbrVisit { uint32_t slot_q, slot_p, f0, g0, nf, ng, base, pad; uint64_t at; };

// the words of HBM scratch the deep levels of these sides take (sides[i].deep_off filled in)
size_t tbr_deep_words(const Geometry &g, TbrSide *sides, size_t n_sides);
// store[op.out] = the root set of every chain step, rows as in the engine's store (S rows x tbr_row_words(g) words); weighted engine:
// k_tbr_snk_roots, a side whose pad bit 0 is set stores m(R)
hipError_t launch_tbr_roots(hipStream_t st, const Geometry &g, const uint32_t *vec, const tbrplan::Op *ops, const TbrSide *sides, size_t n_sides,
                            uint32_t *store, uint32_t *deep);
// the matrices of the visits, one workgroup per item; shape: tbrplan::TILE_NARROW | TILE_WIDE, the one the items were cut for (with the
// engine kind: tbrplan::tile_dims(S, shape, g.sankoff)).  Weighted engine: k_tbr_costs over PlaceMinPlus, TbrVisit::base unused
hipError_t launch_tbr_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                            const tbrplan::Item *items, size_t n_items, int shape, uint32_t *out);
// best[3 v] = the first minimum of visit v's matrix in row-major order, [0][0] left out, best[3 v + 1], [3 v + 2] = its row and
// column; 0xFFFFFFFF all three for a 1 x 1 matrix (one wave per visit)
hipError_t launch_tbr_best(hipStream_t st, const TbrVisit *visits, size_t n_visits, const uint32_t *out, uint32_t *best);
// Under a UFBoot tracker (k_tbr_masks; Fitch engine).  Per site, pattern_pars(T_ij) = pattern_pars(T) - M[0][0] + M[i][j] with M[i][j]
// the 1-bit-per-site word "R_q(F_i) and R_p(G_j) share no state" (each part's own per-site length does not depend on where it is
// rooted).  masks[col.out][0 .. Wp) = M[run.row][col.col] of visit run.visit for every column cols[run.begin .. run.end) of every run:
// rows in the form of launch_join_masks, ready for the REPS product.  Every `out` must lie inside masks; one entry, one writer
hipError_t launch_tbr_masks(hipStream_t st, const Geometry &g, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                            const tbrplan::MaskRun *runs, size_t n_runs, const tbrplan::MaskCol *cols, uint32_t *masks);
// ... on the weighted engine (k_tbr_snk_vals; a Fitch geometry is refused as launch_tbr_masks refuses a weighted one).  A joined tree's
// _pattern_pars row is, per pattern, min_x(R_q(F_i)[x] + m(R_p(G_j))[x]): the terms whose weighted sum cost[i][j] is.
// vals[col.out][0 .. g.Wp) = that row as 16-bit values for every listed column of every run, in the layout of launch_snk_nni_eval's
// vals (launch_vals_planes reads it); *vmax takes the largest value written (atomic max: the caller zeroes it).  The same lists as
// launch_tbr_masks.  tbr_snk_vals_fit: every value fits 16 bits, n_taxa x highest_cost < 65536 -- implied by the 16-bit store's own
// condition, required of the 32-bit store (the launcher refuses a geometry that does not fit; nothing is truncated)
bool tbr_snk_vals_fit(const Geometry &g, int n_taxa);
hipError_t launch_tbr_snk_vals(hipStream_t st, const Geometry &g, int n_taxa, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                               const tbrplan::MaskRun *runs, size_t n_runs, const tbrplan::MaskCol *cols, uint16_t *vals, uint32_t *vmax);

}  // namespace mpf
