// tbr.hip -- the TBR neighbourhood on gfx950: root sets of both parts of a cut edge, and the pair product over them (host/tbr.cpp).
//
// No reference function: MPBoot has SPR and NNI only.  With every directional view resident, the tree that joins the middle of branch
// f of q's part to the middle of branch g of p's part costs one popcount over two root sets (tbr.hpp); row 0 and column 0 of a
// visit's matrix are the insertion tests of rearrangeParsimony (sprparsimony.cpp:2259-2376).
//
//   k_tbr_roots  one wave per (side, tile of 64 site words) walks the side's chain program; U per depth in LDS, beyond tbr_lds_levels
//                in HBM scratch as k_scan_deep keeps its levels; every chain step stores fitch(U, vec[own]) into the scratch store
//   k_tbr_costs  k_place_costs' skeleton (place.hip) over the and-or algebra of PlaceFitch, without the join: a workgroup owns a tile
//                of F rows x G columns of ONE visit and walks the row of words in slices through LDS, the next slice's loads issued
//                before this slice's arithmetic.  Index 0 of either side reads the resident vector, the rest the scratch store:
//                absolute 64-bit row pointers.  The launch is a flat list of (visit, F tile, G tile) items.  One writer per output
//   k_tbr_best   one wave per visit: the first minimum of its matrix, [0][0] left out
//   k_tbr_masks  under a UFBoot tracker: the "no common state" word itself, one mask row per listed entry (host/tbr.cpp)
// Padding bits are set in every state row of every resident vector, so they are in every U and every root set, and always match.
//
// On the weighted (-cost) engine (option "tbr_weighted", symmetric cost matrices) the same plan runs over the min-plus algebra, m()
// the stored transform with the viewer as the parent:
//   k_tbr_snk_roots  the chain of k_snk_scan: MU[0] = m(vec[own]) as stored, U = MU[d - 1] + m(vec[sib]), MU[d] = m(U), root set
//                    R = MU[d] + m(vec[own]); MU per depth where k_tbr_roots keeps U.  A side of F stores R, a side of G stores m(R),
//                    so the S x S transform is paid once per root set and not once per pair
//   k_tbr_costs      over PlaceMinPlus: cost[i][j] = sum_ptn w * min_x(RF_i[x] + m(RG_j)[x]), the FULL length, no additive base;
//                    row 0 reads vec[slot_q] as it is, column 0 the stored transform of slot_p
//   k_tbr_snk_vals   under a UFBoot tracker (option "tbr_weighted_tracked"): the per-pattern terms min_x(RF_i[x] + m(RG_j)[x]) themselves,
//                    one 16-bit row per listed entry
#include "tbr.hpp"
#include "pair_algebra.hpp"
#include "wave_min.hpp"

namespace mpf {

namespace {

// r = fitch(a, b) in place of a: the intersection where it is not empty, the union elsewhere
template <int S>
__device__ __forceinline__ void fitch_into(uint32_t (&a)[S], const uint32_t (&b)[S])
{
  uint32_t any = 0u;
#pragma unroll
  for (int s = 0; s < S; s++) any |= a[s] & b[s];
#pragma unroll
  for (int s = 0; s < S; s++) a[s] = (a[s] & b[s]) | (~any & (a[s] | b[s]));
}

template <int S, int LD>
__global__ __launch_bounds__(64) void k_tbr_roots(const uint32_t *__restrict__ vec, const tbrplan::Op *__restrict__ ops,
                                                  const TbrSide *__restrict__ sides, int tiles, int Wp, uint32_t *__restrict__ store,
                                                  uint32_t *__restrict__ deep)
{
  __shared__ uint32_t su[LD * S * 64];               // [level][state row][lane]: a lane reads and writes its own column only, no barrier
  const int lane = (int)threadIdx.x;
  const size_t side = (size_t)blockIdx.x / (size_t)tiles, tile = (size_t)blockIdx.x % (size_t)tiles;
  const size_t w = tile * 64 + (size_t)lane, row = (size_t)Wp, vsz = (size_t)S * row;
  if (w >= row) return;                              // (Wp is a multiple of 32: the last tile may be half full)
  const TbrSide sd = sides[side];
  uint32_t *dl = deep + sd.deep_off + tile * (size_t)sd.deep_levels * (size_t)(S * 64) + (size_t)lane;
  auto level = [&](int d) -> uint32_t * { return d < LD ? &su[d * S * 64 + lane] : dl + (size_t)(d - LD) * (size_t)(S * 64); };
  for (uint32_t i = sd.op_begin; i < sd.op_end; i++) {
    const tbrplan::Op o = ops[i];
    const int d = (int)(o.meta & 255u);
    uint32_t u[S], x[S];
    if ((o.meta >> 16) == (uint32_t)tbrplan::OP_ROOT) {
      const uint32_t *v = vec + (size_t)o.own * vsz + w;
      uint32_t *l0 = level(0);
#pragma unroll
      for (int s = 0; s < S; s++) l0[s * 64] = v[(size_t)s * row];
      continue;
    }
    const uint32_t *vs = vec + (size_t)o.sib * vsz + w, *vo = vec + (size_t)o.own * vsz + w;
    const uint32_t *up = level(d - 1);
#pragma unroll
    for (int s = 0; s < S; s++) { u[s] = up[s * 64]; x[s] = vs[(size_t)s * row]; }
    fitch_into<S>(u, x);
#pragma unroll
    for (int s = 0; s < S; s++) x[s] = vo[(size_t)s * row];
    uint32_t *ud = level(d);
#pragma unroll
    for (int s = 0; s < S; s++) ud[s * 64] = u[s];
    fitch_into<S>(u, x);
    uint32_t *r = store + (size_t)o.out * vsz + w;
#pragma unroll
    for (int s = 0; s < S; s++) r[(size_t)s * row] = u[s];
  }
}

// The weighted root sets.  One wave per (side, tile of 64 elements of the row: patterns, or pairs of patterns in the 16-bit store); a
// lane owns its element for the whole program.  MU[d] = m(U[d]) per depth, in LDS and beyond tbr_lds_levels in HBM scratch exactly
// as k_tbr_roots keeps U; every operand read from the engine's store is a STORED transform (the `moff` half), so a chain step costs
// one transform, m(U), and a side of G (TbrSide::pad bit 0) one more, m(R): the costs product then adds and takes minima only.
// 16-bit store: U[d] = MU[d - 1] + m(vec[sib]) and R = MU[d] + m(vec[own]) are sums of transforms over disjoint parts of ONE side
// of the cut edge.  A tip's vector is 0 or highest_cost, a view the sum of its children's transforms, and m(v)[z] <= v[z] + cost[z][z]
// = v[z], so a part of t tips stays within t highest_cost: U and R within the side's tips, the costs product's RF_i[x] + m(RG_j)[x]
// within n highest_cost, and inside a transform v[x] + cost[z][x] within (n + 1) highest_cost -- all below what Engine::pack guards,
// 3 n highest_cost < 65536.  No 32-bit fall-back is needed.
template <int S, bool PK, int LD>
__global__ __launch_bounds__(64) void k_tbr_snk_roots(const uint32_t *__restrict__ mvec, const tbrplan::Op *__restrict__ ops,
                                                      const TbrSide *__restrict__ sides, int tiles, int We,
                                                      const uint32_t *__restrict__ cost, uint32_t *__restrict__ store,
                                                      uint32_t *__restrict__ deep)
{
  typedef SnkT<PK> T;
  typedef typename T::E E;
  __shared__ uint32_t su[LD * S * 64];               // [level][state row][lane]: a lane reads and writes its own column only, no barrier
  const int lane = (int)threadIdx.x;
  const size_t side = (size_t)blockIdx.x / (size_t)tiles, tile = (size_t)blockIdx.x % (size_t)tiles;
  const size_t e = tile * 64 + (size_t)lane, row = (size_t)We, vsz = (size_t)S * row;
  if (e >= row) return;                              // (We is a multiple of 16: the last tile may be partly full; no lane waits on another)
  const TbrSide sd = sides[side];
  const bool transformed = (sd.pad & 1u) != 0u;      // a side of G: the root sets are stored as m(R)
  uint32_t *dl = deep + sd.deep_off + tile * (size_t)sd.deep_levels * (size_t)(S * 64) + (size_t)lane;
  auto level = [&](int d) -> uint32_t * { return d < LD ? &su[d * S * 64 + lane] : dl + (size_t)(d - LD) * (size_t)(S * 64); };
  for (uint32_t i = sd.op_begin; i < sd.op_end; i++) {
    const tbrplan::Op o = ops[i];
    const int d = (int)(o.meta & 255u);
    Costs<S, PK> u, x, mu;
    if ((o.meta >> 16) == (uint32_t)tbrplan::OP_ROOT) {
      load_costs<S, PK>(x, mvec, o.own, We, (int)e);
      uint32_t *l0 = level(0);
#pragma unroll
      for (int s = 0; s < S; s++) l0[s * 64] = __builtin_bit_cast(uint32_t, x.v[s]);
      continue;
    }
    load_costs<S, PK>(x, mvec, o.sib, We, (int)e);
    const uint32_t *up = level(d - 1);
#pragma unroll
    for (int s = 0; s < S; s++) u.v[s] = T::add(__builtin_bit_cast(E, up[s * 64]), x.v[s]);      // U[d]
    mplus_fast<S, PK>(mu, u, cost);
    load_costs<S, PK>(x, mvec, o.own, We, (int)e);
    uint32_t *ud = level(d);
#pragma unroll
    for (int s = 0; s < S; s++) ud[s * 64] = __builtin_bit_cast(uint32_t, mu.v[s]);
#pragma unroll
    for (int s = 0; s < S; s++) u.v[s] = T::add(mu.v[s], x.v[s]);                               // R
    if (transformed) { mplus_fast<S, PK>(mu, u, cost); u = mu; }
    uint32_t *r = store + (size_t)o.out * vsz + e;
#pragma unroll
    for (int s = 0; s < S; s++) r[(size_t)s * row] = __builtin_bit_cast(uint32_t, u.v[s]);
  }
}

// out[at + i ng + j] = A::finish of the sum over the row's `len` elements of A::weigh(the sum over the state rows of A::mul(row i of F,
// row j of G)).  PlaceFitch: base + 32 len - the sum over the row's words of popc(OR over the state rows of (row i of F & row j of
// G)).  PlaceMinPlus: the weighted sum of min_x(F_i[x] + G_j[x]) over the patterns; column 0 is read `moff` words behind vec (the
// stored transform of slot_p), pwgt holds the pattern weights (0 on padding)
template <class A, int TQ, int TB, int RQ, int RB, int KS, int KT>
__global__ __launch_bounds__(256) void k_tbr_costs(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ store,
                                                   const TbrVisit *__restrict__ visits, const tbrplan::Item *__restrict__ items, int len_,
                                                   uint32_t *__restrict__ out, size_t moff, const uint32_t *__restrict__ pwgt)
{
  typedef typename A::E E;
  constexpr int S = A::S, NW = KS * A::NP, TBT = TB / RB, TQT = TQ / RQ;
  static_assert(A::template slice_ok<KS>, "the algebra's slice");
  static_assert(TBT * TQT * KT == 256 && TB % RB == 0 && TQ % RQ == 0 && KS % KT == 0, "lane mapping");
  static_assert(KT == 1 || KT * TQ * TB <= KS * (S * TB + 64 / KS), "the partial sums reuse the column slice");
  static_assert(64 % KS == 0 && (64 / KS) % 4 == 0, "padding keeps the 16-byte alignment");
  constexpr int BI = (TB * KS + 255) / 256, QI = (TQ * KS + 255) / 256;      // staged (vector, word) items per lane
  // [word of the slice][state row][column | row], 64 / KS words of padding behind every word of the slice (place.hip)
  constexpr int XP = S * TB + 64 / KS, QP = S * TQ + 64 / KS;
  __shared__ __attribute__((aligned(16))) uint32_t sx[KS * XP];
  __shared__ __attribute__((aligned(16))) uint32_t sq[KS * QP];
  __shared__ uint32_t sw[NW ? NW : 1];                       // (NW == 0: never touched, takes no LDS)
  const size_t len = (size_t)len_, vsz = (size_t)S * len;
  const int tid = (int)threadIdx.x;
  const int tb = tid % TBT, tq = (tid / TBT) % TQT, kt = tid / (TBT * TQT);
  const tbrplan::Item it = items[blockIdx.x];
  const TbrVisit vd = visits[it.visit];
  const int nf = (int)vd.nf, ng = (int)vd.ng, f_lo = (int)it.ft * TQ, g_lo = (int)it.gt * TB;

  const uint32_t *pg[BI], *pf[QI];
#pragma unroll
  for (int i = 0; i < BI; i++) {
    const int idx = tid + 256 * i;
    const int j = min(g_lo + min(idx / KS, TB - 1), ng - 1);               // (columns past the end repeat the last: loads stay inside)
    pg[i] = (j == 0 ? vec + (NW ? moff : (size_t)0) + (size_t)vd.slot_p * vsz : store + ((size_t)vd.g0 + (size_t)(j - 1)) * vsz) + (size_t)(idx % KS);
  }
#pragma unroll
  for (int i = 0; i < QI; i++) {
    const int idx = tid + 256 * i;
    const int f = min(f_lo + min(idx / KS, TQ - 1), nf - 1);
    pf[i] = (f == 0 ? vec + (size_t)vd.slot_q * vsz : store + ((size_t)vd.f0 + (size_t)(f - 1)) * vsz) + (size_t)(idx % KS);
  }
  uint32_t rg[BI][S], rf[QI][S], rw = 0u;
  auto fetch = [&](size_t k0) {
#pragma unroll
    for (int i = 0; i < BI; i++)
      if (tid + 256 * i < TB * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) rg[i][s] = pg[i][(size_t)s * len + k0];
      }
#pragma unroll
    for (int i = 0; i < QI; i++)
      if (tid + 256 * i < TQ * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) rf[i][s] = pf[i][(size_t)s * len + k0];
      }
    if constexpr (NW > 0)
      if (tid < NW) rw = pwgt[k0 * A::NP + (size_t)tid];
  };
  fetch(0);

  uint32_t acc[RQ][RB];
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) acc[i][j] = 0u;

  for (size_t k0 = 0; k0 < len; k0 += KS) {                  // (a row is whole slices: Wp is a multiple of 32, We of 16)
    __syncthreads();                                         // the last slice has been read by everybody
#pragma unroll
    for (int i = 0; i < BI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TB * KS) {
        uint32_t *d = &sx[(idx % KS) * XP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++) d[s * TB] = rg[i][s];
      }
    }
#pragma unroll
    for (int i = 0; i < QI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TQ * KS) {
        uint32_t *d = &sq[(idx % KS) * QP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++) d[s * TQ] = rf[i][s];
      }
    }
    if constexpr (NW > 0)
      if (tid < NW) sw[tid] = rw;
    __syncthreads();
    if (k0 + KS < len) fetch(k0 + KS);                       // the next slice is on its way while this one is summed
#pragma unroll 2
    for (int k = kt; k < KS; k += KT) {
      E m[RQ][RB];
#pragma unroll
      for (int s = 0; s < S; s++) {
        E xv[RB], qv[RQ];
#pragma unroll
        for (int j = 0; j < RB; j++) xv[j] = __builtin_bit_cast(E, sx[k * XP + s * TB + tb * RB + j]);
#pragma unroll
        for (int i = 0; i < RQ; i++) qv[i] = __builtin_bit_cast(E, sq[k * QP + s * TQ + tq * RQ + i]);
#pragma unroll
        for (int i = 0; i < RQ; i++)
#pragma unroll
          for (int j = 0; j < RB; j++) {
            const E t = A::mul(qv[i], xv[j]);
            m[i][j] = s == 0 ? t : A::add(m[i][j], t);
          }
      }
#pragma unroll
      for (int i = 0; i < RQ; i++)
#pragma unroll
        for (int j = 0; j < RB; j++) acc[i][j] += A::weigh(m[i][j], sw, k);
    }
  }

  if constexpr (KT > 1) {
    // the KT word classes of an output meet in LDS; class 0 adds them up in a fixed order
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RQ; i++)
#pragma unroll
      for (int j = 0; j < RB; j++) sx[(kt * TQ + tq * RQ + i) * TB + tb * RB + j] = acc[i][j];
    __syncthreads();
    if (kt != 0) return;
#pragma unroll
    for (int i = 0; i < RQ; i++)
#pragma unroll
      for (int j = 0; j < RB; j++) {
        uint32_t s = 0u;
        for (int c = 0; c < KT; c++) s += sx[(c * TQ + tq * RQ + i) * TB + tb * RB + j];
        acc[i][j] = s;
      }
  }
  const uint32_t bits = 32u * (uint32_t)len_ + vd.base;      // (the sites of a row of words; the two parts' own lengths)
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int f = f_lo + tq * RQ + i, g = g_lo + tb * RB + j;
      if (f < nf && g < ng) out[vd.at + (size_t)f * (size_t)ng + (size_t)g] = A::finish(acc[i][j], bits);
    }
}

// one wave per visit: the lowest entry of its matrix behind [0][0] and the lowest row-major index that has it
__global__ __launch_bounds__(64) void k_tbr_best(const TbrVisit *__restrict__ visits, const uint32_t *__restrict__ out, uint32_t *__restrict__ best)
{
  const TbrVisit vd = visits[blockIdx.x];
  const uint32_t *m = out + vd.at;
  const size_t count = (size_t)vd.nf * (size_t)vd.ng;
  uint32_t v = 0xFFFFFFFFu;
  size_t at = (size_t)-1;
  for (size_t e = 1 + (size_t)threadIdx.x; e < count; e += 64) {
    const uint32_t x = m[e];
    if (at == (size_t)-1 || x < v) { v = x; at = e; }      // (a lane's indices rise: the first of equal values stays)
  }
  const MinAt<size_t> w = wave_first_min(v, at);      // (a lane without an entry has at = (size_t)-1 still: the helper's empty lane)
  if (threadIdx.x == 0) {
    uint32_t *b = best + 3 * (size_t)blockIdx.x;
    if (w.at == (size_t)-1) { b[0] = b[1] = b[2] = 0xFFFFFFFFu; }
    else { b[0] = w.v; b[1] = (uint32_t)(w.at / vd.ng); b[2] = (uint32_t)(w.at % vd.ng); }
  }
}

// The mask rows a UFBoot tracker needs of a visit's matrix (host/tbr.cpp): masks[out][w] = ~OR over the state rows of (row i of F
// & column j of G), the very word whose popcount k_tbr_costs takes, laid out as k_join_masks lays a row (Wp words, bit b of word w =
// site 32 w + b; padding bits are set in every state row of both operands and so come out 0).  One wave per (run, tile of 64 site
// words): a run is one row i of one visit with a list of its columns; the lane keeps its word of RF_i's S state rows in registers,
// walks the run's columns and stores one coalesced 256-byte stretch per column.  Index 0 of either side reads the resident vector.
// One writer per word, no LDS, no atomics; the run and column records are wave-uniform
template <int S>
__global__ __launch_bounds__(64) void k_tbr_masks(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ store,
                                                  const TbrVisit *__restrict__ visits, const tbrplan::MaskRun *__restrict__ runs,
                                                  const tbrplan::MaskCol *__restrict__ cols, int tiles, int Wp, uint32_t *__restrict__ masks)
{
  const size_t run = (size_t)blockIdx.x / (size_t)tiles, tile = (size_t)blockIdx.x % (size_t)tiles;
  const size_t w = tile * 64 + (size_t)threadIdx.x, row = (size_t)Wp, vsz = (size_t)S * row;
  if (w >= row) return;                              // (Wp is a multiple of 32: the last tile may be half full)
  const tbrplan::MaskRun r = runs[run];
  const TbrVisit vd = visits[r.visit];
  const uint32_t *pf = (r.row == 0 ? vec + (size_t)vd.slot_q * vsz : store + ((size_t)vd.f0 + (size_t)(r.row - 1)) * vsz) + w;
  uint32_t rf[S];
#pragma unroll
  for (int s = 0; s < S; s++) rf[s] = pf[(size_t)s * row];
  for (uint32_t c = r.begin; c < r.end; c++) {
    const tbrplan::MaskCol cj = cols[c];
    const uint32_t *pg = (cj.col == 0 ? vec + (size_t)vd.slot_p * vsz : store + ((size_t)vd.g0 + (size_t)(cj.col - 1)) * vsz) + w;
    uint32_t any = 0u;
#pragma unroll
    for (int s = 0; s < S; s++) any |= rf[s] & pg[(size_t)s * row];
    masks[(size_t)cj.out * row + w] = ~any;
  }
}

// The rows a UFBoot tracker needs of a visit's matrix on the weighted engine (host/tbr.cpp): vals[out][p] = min_x(RF_i[x] +
// m(RG_j)[x]) of pattern p, the very terms whose weighted sum k_tbr_costs<PlaceMinPlus> returns as cost[i][j] -- the _pattern_pars
// row of the joined tree.  The shape is k_tbr_masks's, the algebra k_snk_branch_eval's: one wave per (run, tile of 64 elements of a
// row of We elements), a run one row i of one visit with a list of its columns.  The lane keeps its element of RF_i's S state rows
// in registers (row 0: vec at slot_q), walks the run's columns (wave-uniform records), loads its element of m(RG_j)'s S rows -- the
// chunk's G sets are stored transformed, column 0 is the STORED transform of vec at slot_p: nothing is transformed here -- and stores
// the minimum into vals[out][npat] in the layout k_snk_nni_eval_vals writes and k_vals_planes reads: a us2 per lane in the 16-bit
// store (patterns 2 e, 2 e + 1), one uint16_t in the 32-bit store.  One writer per element, no LDS, one atomicMax per wave into vmax.
// Lanes at and beyond We are clamped onto the last element (lane_word's rule): they load real data, store nothing and add nothing to
// the maximum; padding patterns inside a row are stored as they come, as k_snk_nni_eval_vals stores them (their sample weights are 0).
// 16 bits: RF_i and RG_j are sums of transforms over disjoint parts holding the n tips between them, a tip's vector is 0 or
// highest_cost and m(v)[z] <= v[z], so RF_i[x] + m(RG_j)[x] <= n highest_cost (k_tbr_snk_roots above, DESIGN 5q "16-bit store").  The
// 16-bit store exists under 3 n highest_cost < 65536 only (Engine::pack).  The 32-bit store has no such guard of its own -- the
// rows k_snk_scan writes there rest on the lengths of real data being small -- so the launcher serves it only where the same bound,
// n highest_cost < 65536, holds, and refuses it otherwise: no value is ever truncated.
template <int S, bool PK>
__global__ __launch_bounds__(64) void k_tbr_snk_vals(const uint32_t *__restrict__ vec, const uint32_t *__restrict__ mvec,
                                                     const uint32_t *__restrict__ store, const TbrVisit *__restrict__ visits,
                                                     const tbrplan::MaskRun *__restrict__ runs, const tbrplan::MaskCol *__restrict__ cols,
                                                     int tiles, int We, uint16_t *__restrict__ vals, uint32_t npat, uint32_t *__restrict__ vmax)
{
  typedef SnkT<PK> T;
  typedef typename T::E E;
  const size_t run = (size_t)blockIdx.x / (size_t)tiles, tile = (size_t)blockIdx.x % (size_t)tiles;
  const int lane = (int)threadIdx.x;
  const bool valid = tile * 64 + (size_t)lane < (size_t)We;
  const int e0 = valid ? (int)(tile * 64) + lane : We - 1;
  const tbrplan::MaskRun r = runs[run];
  const TbrVisit vd = visits[r.visit];
  Costs<S, PK> rf;
  if (r.row == 0) load_costs<S, PK>(rf, vec, vd.slot_q, We, e0);
  else load_costs<S, PK>(rf, store, vd.f0 + (r.row - 1), We, e0);
  uint32_t m = 0;
  for (uint32_t c = r.begin; c < r.end; c++) {
    const tbrplan::MaskCol cj = cols[c];
    Costs<S, PK> mg;
    if (cj.col == 0) load_costs<S, PK>(mg, mvec, vd.slot_p, We, e0);
    else load_costs<S, PK>(mg, store, vd.g0 + (cj.col - 1), We, e0);
    E best = T::inf();
#pragma unroll
    for (int x = 0; x < S; x++) best = T::mn(best, T::add(rf.v[x], mg.v[x]));
    if (valid) {
      uint16_t *row = vals + (size_t)cj.out * npat;
      if constexpr (PK) {
        *reinterpret_cast<us2 *>(row + 2 * e0) = best;
        m = max(m, max((uint32_t)best.x, (uint32_t)best.y));
      } else {
        row[e0] = (uint16_t)best;
        m = max(m, (uint32_t)best);
      }
    }
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, sh, 64));
  if (lane == 0 && m) atomicMax(vmax, m);
}

}  // namespace

bool tbr_snk_vals_fit(const Geometry &g, int n_taxa)
{
  return g.sankoff && (uint64_t)n_taxa * (uint64_t)g.highest_cost < 65536ull;
}

hipError_t launch_tbr_snk_vals(hipStream_t st, const Geometry &g, int n_taxa, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                               const tbrplan::MaskRun *runs, size_t n_runs, const tbrplan::MaskCol *cols, uint16_t *vals, uint32_t *vmax)
{
  if (!vec) return hipErrorInvalidValue;
  if (!g.sankoff || !g.moff || g.costT || g.Wp <= 0 || g.Wp % 32) return hipErrorInvalidValue;      // (a vals row is a min-plus join)
  if (!tbr_snk_vals_fit(g, n_taxa) || !vals || !vmax) return hipErrorInvalidValue;
  if (!n_runs) return hipSuccess;
  const int We = tbr_row_words(g);
  const size_t tiles = ((size_t)We + 63) / 64;
  if (n_runs * tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  dispatch_snk(g, [&](auto S, auto PK) {
    hipLaunchKernelGGL((k_tbr_snk_vals<S, PK>), dim3((unsigned)(n_runs * tiles)), dim3(64), 0, st, vec, vec + g.moff, store, visits, runs, cols,
                       (int)tiles, We, vals, (uint32_t)g.Wp, vmax);
  });
  return hipGetLastError();
}

hipError_t launch_tbr_masks(hipStream_t st, const Geometry &g, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                            const tbrplan::MaskRun *runs, size_t n_runs, const tbrplan::MaskCol *cols, uint32_t *masks)
{
  if (!vec) return hipErrorInvalidValue;
  if (g.sankoff || g.Wp <= 0 || g.Wp % 32) return hipErrorInvalidValue;      // (a mask row is a Fitch join)
  if (!n_runs) return hipSuccess;
  const size_t tiles = ((size_t)g.Wp + 63) / 64;
  if (n_runs * tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  dispatch_states(g.S, [&](auto S) {
    hipLaunchKernelGGL((k_tbr_masks<S>), dim3((unsigned)(n_runs * tiles)), dim3(64), 0, st, vec, store, visits, runs, cols, (int)tiles, g.Wp, masks);
  });
  return hipGetLastError();
}

size_t tbr_deep_words(const Geometry &g, TbrSide *sides, size_t n_sides)
{
  const size_t tiles = ((size_t)tbr_row_words(g) + 63) / 64;
  size_t at = 0;
  for (size_t i = 0; i < n_sides; i++) {
    sides[i].deep_off = at;
    at += tiles * (size_t)sides[i].deep_levels * (size_t)g.S * 64;
  }
  return at;
}

hipError_t launch_tbr_roots(hipStream_t st, const Geometry &g, const uint32_t *vec, const tbrplan::Op *ops, const TbrSide *sides, size_t n_sides,
                            uint32_t *store, uint32_t *deep)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (g.Wp <= 0 || g.Wp % 32 || (g.sankoff && (!g.moff || !g.cost || g.costT))) return hipErrorInvalidValue;
  if (!n_sides) return hipSuccess;
  const int We = tbr_row_words(g);
  const size_t tiles = ((size_t)We + 63) / 64;
  if (n_sides * tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (g.sankoff) {
    dispatch_snk(g, [&](auto S, auto PK) {
      hipLaunchKernelGGL((k_tbr_snk_roots<S, PK, tbr_lds_levels(S)>), dim3((unsigned)(n_sides * tiles)), dim3(64), 0, st, vec + g.moff, ops, sides,
                         (int)tiles, We, g.cost, store, deep);
    });
    return hipGetLastError();
  }
  dispatch_states(g.S, [&](auto S) {
    hipLaunchKernelGGL((k_tbr_roots<S, tbr_lds_levels(S)>), dim3((unsigned)(n_sides * tiles)), dim3(64), 0, st, vec, ops, sides, (int)tiles, g.Wp,
                       store, deep);
  });
  return hipGetLastError();
}

hipError_t launch_tbr_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const uint32_t *store, const TbrVisit *visits,
                            const tbrplan::Item *items, size_t n_items, int shape, uint32_t *out)
{
  if (!vec) return hipErrorInvalidValue;
  if (g.Wp <= 0 || g.Wp % 32 || (shape != tbrplan::TILE_NARROW && shape != tbrplan::TILE_WIDE)) return hipErrorInvalidValue;
  if (g.sankoff && (!g.moff || !g.pwgt || g.costT)) return hipErrorInvalidValue;
  if (!n_items) return hipSuccess;
  if (n_items > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // the algebra's kernel in the shape its row of the one table (host/pair_tile.hpp) gives it
  auto launch = [&](auto a, auto WEIGHTED) {
    typedef decltype(a) A;
    dispatch_bool(shape == tbrplan::TILE_NARROW, [&](auto NARROW) {
      constexpr int SH = NARROW ? tbrplan::TILE_NARROW : tbrplan::TILE_WIDE;
      constexpr PlaceShape sh = place_shape(A::S, WEIGHTED, SH);
      static_assert(tbrplan::tile_dims(A::S, SH, WEIGHTED).tf == sh.tq && tbrplan::tile_dims(A::S, SH, WEIGHTED).tg == sh.tb,
                    "the items were cut for another tile");
      hipLaunchKernelGGL((k_tbr_costs<A, sh.tq, sh.tb, sh.rq, sh.rb, sh.ks, sh.kt>), dim3((unsigned)n_items), dim3(256), 0, st, vec, store, visits,
                         items, tbr_row_words(g), out, g.moff, g.pwgt);
    });
  };
  if (g.sankoff) dispatch_snk(g, [&](auto S, auto PK) { launch(PlaceMinPlus<S, PK, true>(), bool_c<true>()); });
  else dispatch_states(g.S, [&](auto S) { launch(PlaceFitch<S>(), bool_c<false>()); });
  return hipGetLastError();
}

hipError_t launch_tbr_best(hipStream_t st, const TbrVisit *visits, size_t n_visits, const uint32_t *out, uint32_t *best)
{
  if (!n_visits) return hipSuccess;
  hipLaunchKernelGGL(k_tbr_best, dim3((unsigned)n_visits), dim3(64), 0, st, visits, out, best);
  return hipGetLastError();
}

}  // namespace mpf
