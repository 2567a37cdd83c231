// place.hip -- taxon insertion on gfx950: the cost of attaching every query tip to every branch of a backbone tree (host/place.cpp).
//
// Reference: PhyloTree::addTaxonMPFast (phylotree.cpp:1322-1378) calls computeParsimonyBranch once per (taxon, branch).  Fitch length
// does not depend on the root, so with the two directed views A, B of a branch (k_poly_views made all of them in one launch) and the
// query tip's own vector T the tree with T in the middle of the branch is len(tree) + #sites where X and T share no state,
//   X = A & B at the sites where some state row of it is set, A | B elsewhere.
// Sites are weight-replicated bits and padding bits are set in every state row of every vector, so the sum is a popcount and the
// padding always matches: delta = 32 Wp - popc(OR_s(X_s & T_s)) summed over the row.
//
// k_place_costs is k_rf_shared's scheme (splits.hip) with the state rows as a second inner dimension: a workgroup owns a tile of TQ
// queries x TB branches and walks the row in slices of KS elements.  Both operands of a slice go through LDS; the branch operand is
// loaded as its two views and JOINED on the way in, so X never exists in HBM and one query costs no extra pass.  The next slice's
// global loads are issued before this slice's arithmetic.  A lane holds RQ x RB outputs; per (query, branch, element) the work is S
// products, S - 1 sums and one accumulate.  In the narrow shape the 256 lanes also split the elements of a slice KT ways and the
// partial sums meet in LDS at the end -- every output has one writer, no atomics, the same sum every run.  No workgroup waits on
// another.
//
// The kernel is written once over an algebra A, which supplies what the two engines do differently:
//   PlaceFitch<S>            and-or over words of 32 sites (v_and / v_and_or), one v_bcnt with accumulate per element
//   PlaceMinPlus<S, PK, BIG> the weighted (-cost) engine: min-plus over the stored transforms, a weighted sum per element
#include "place.hpp"
#include "pair_algebra.hpp"
#include "wave_min.hpp"

namespace mpf {

namespace {

// out[q * ld + b] = A::finish of the sum over the row's `len` elements of A::weigh(the sum over the state rows of
// A::mul(row of vector qslot[q], A::join(rows of vectors desc[b].a, desc[b].b))); vector v's row s starts (v S + s) len words behind base
template <class A, int TQ, int TB, int RQ, int RB, int KS, int KT>
__global__ __launch_bounds__(256) void k_place_costs(const uint32_t *__restrict__ base, const BranchDesc *__restrict__ desc, int n_br,
                                                    const uint32_t *__restrict__ qslot, int n_query, int len_,
                                                    const uint32_t *__restrict__ pwgt, uint32_t *__restrict__ out, int ld)
{
  typedef typename A::Off Off;
  typedef typename A::E E;
  constexpr int S = A::S, NW = KS * A::NP, TBT = TB / RB, TQT = TQ / RQ;
  static_assert(TBT * TQT * KT == 256 && TB % RB == 0 && TQ % RQ == 0 && KS % KT == 0, "lane mapping");
  static_assert(KT == 1 || KT * TQ * TB <= KS * (S * TB + 64 / KS), "the partial sums reuse the branch slice");
  static_assert(64 % KS == 0 && (64 / KS) % 4 == 0, "padding keeps the 16-byte alignment");
  static_assert(A::template slice_ok<KS>, "the algebra's slice");
  constexpr int BI = (TB * KS + 255) / 256, QI = (TQ * KS + 255) / 256;      // staged (vector, element) items per lane
  // [element of the slice][state row][branch | query], 64 / KS words of padding behind every element of the slice: the staging stores
  // of a wave (KS consecutive elements of 64 / KS vectors) then fall on 64 different banks, and every row still starts on 16 bytes
  constexpr int XP = S * TB + 64 / KS, QP = S * TQ + 64 / KS;
  __shared__ __attribute__((aligned(16))) uint32_t sx[KS * XP];
  __shared__ __attribute__((aligned(16))) uint32_t sq[KS * QP];
  __shared__ uint32_t sw[NW ? NW : 1];                       // (NW == 0: never touched, takes no LDS)
  const Off len = (Off)len_;
  const int tid = (int)threadIdx.x;
  const int tb = tid % TBT, tq = (tid / TBT) % TQT, kt = tid / (TBT * TQT);

  // staging: item idx -> vector idx / KS of the tile, element idx % KS of the slice (a lane group reads KS consecutive elements of a row)
  typename A::Row pa[BI], pb[BI], pq[QI];
#pragma unroll
  for (int i = 0; i < BI; i++) {
    const int idx = tid + 256 * i;
    const int b = min((int)blockIdx.x * TB + min(idx / KS, TB - 1), n_br - 1);      // (rows past the end repeat the last: loads stay inside)
    const BranchDesc d = desc[b];
    pa[i] = A::row(base, (Off)d.a * (Off)S * len) + (Off)(idx % KS);
    pb[i] = A::row(base, (Off)d.b * (Off)S * len) + (Off)(idx % KS);
  }
#pragma unroll
  for (int i = 0; i < QI; i++) {
    const int idx = tid + 256 * i;
    const int q = min((int)blockIdx.y * TQ + min(idx / KS, TQ - 1), n_query - 1);
    pq[i] = A::row(base, (Off)qslot[q] * (Off)S * len) + (Off)(idx % KS);
  }
  uint32_t ra[BI][S], rb[BI][S], rq[QI][S], rw = 0u;
  auto fetch = [&](Off k0) {
#pragma unroll
    for (int i = 0; i < BI; i++)
      if (tid + 256 * i < TB * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) { ra[i][s] = A::load(base, pa[i], (Off)s * len, k0); rb[i][s] = A::load(base, pb[i], (Off)s * len, k0); }
      }
#pragma unroll
    for (int i = 0; i < QI; i++)
      if (tid + 256 * i < TQ * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) rq[i][s] = A::load(base, pq[i], (Off)s * len, k0);
      }
    if constexpr (NW > 0)
      if (tid < NW) rw = pwgt[(size_t)k0 * A::NP + (size_t)tid];
  };
  fetch(0);

  uint32_t acc[RQ][RB];
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) acc[i][j] = 0u;

  for (Off k0 = 0; k0 < len; k0 += KS) {                    // (a row is whole slices: Wp is a multiple of 32, We of 16)
    __syncthreads();                                         // the last slice has been read by everybody
#pragma unroll
    for (int i = 0; i < BI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TB * KS) {
        uint32_t all = 0u;
#pragma unroll
        for (int s = 0; s < S; s++) all = A::gather(all, ra[i][s], rb[i][s]);
        uint32_t *d = &sx[(idx % KS) * XP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++) d[s * TB] = A::join(all, ra[i][s], rb[i][s]);
      }
    }
#pragma unroll
    for (int i = 0; i < QI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TQ * KS) {
        uint32_t *d = &sq[(idx % KS) * QP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++) d[s * TQ] = rq[i][s];
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
    // the KT element classes of an output meet in LDS; class 0 adds them up in a fixed order
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
  const uint32_t bits = 32u * (uint32_t)len_;               // (the sites of a row of words)
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int q = (int)blockIdx.y * TQ + tq * RQ + i, b = (int)blockIdx.x * TB + tb * RB + j;
      if (q < n_query && b < n_br) out[(size_t)q * (size_t)ld + (size_t)b] = A::finish(acc[i][j], bits);
    }
}

// one wave per query: the minimum of its row and the lowest branch index that has it
__global__ __launch_bounds__(64) void k_place_best(const uint32_t *__restrict__ delta, int n_br, int ld, uint32_t *__restrict__ best)
{
  const uint32_t *row = delta + (size_t)blockIdx.x * (size_t)ld;
  uint32_t v = 0xFFFFFFFFu, at = 0xFFFFFFFFu;
  for (int b = (int)threadIdx.x; b < n_br; b += 64) {
    const uint32_t x = row[b];
    if (x < v) { v = x; at = (uint32_t)b; }                  // (a lane's indices rise: the first of equal values stays)
  }
  const MinAt<uint32_t> m = wave_first_min(v, at);
  if (threadIdx.x == 0) { best[2 * blockIdx.x] = m.v; best[2 * blockIdx.x + 1] = m.at; }
}

// the algebra's kernel in the shape place_shape (host/pair_tile.hpp) gives it for `narrow`
template <class A>
void launch_shape(hipStream_t st, bool narrow, const uint32_t *base, const BranchDesc *desc, int n_br, const uint32_t *qslot, int n_query,
                  int len, const uint32_t *pwgt, uint32_t *out, int ld)
{
  dispatch_bool(narrow, [&](auto NARROW) {
    constexpr PlaceShape sh = place_shape(A::S, A::NP > 0, NARROW ? PLACE_NARROW : PLACE_WIDE);
    const dim3 grid((unsigned)((n_br + sh.tb - 1) / sh.tb), (unsigned)((n_query + sh.tq - 1) / sh.tq));
    hipLaunchKernelGGL((k_place_costs<A, sh.tq, sh.tb, sh.rq, sh.rb, sh.ks, sh.kt>), grid, dim3(256), 0, st, base, desc, n_br, qslot, n_query, len,
                       pwgt, out, ld);
  });
}

}  // namespace

int place_pick(int n_query, int n_br, int tile, long long narrow_below)
{
  if (tile == PLACE_NARROW || tile == PLACE_WIDE) return tile;
  return (long long)n_query * (long long)n_br < narrow_below ? PLACE_NARROW : PLACE_WIDE;
}

long long place_narrow_below()
{
  // A wide workgroup walks the whole row alone, so a wide launch takes that long however few tiles it has; the narrow shape's time
  // grows with the outputs.  Measured on C3 (narrow 0.19 ms at 64 x 1485 outputs and 0.81 ms at 256 x 1485, wide 0.58 ms
  // at both) they cross near 2.7e5 outputs: sixty-four 64 x 64 tiles
  return 262144ll;
}

long long place_snk_narrow_below(int S, bool packed)
{
  // A wide workgroup walks the whole row alone, so a wide launch takes that long however few tiles it has (C3, 16-bit store: 15.1 -
  // 15.3 ms from 1 x 1995 to 256 x 1485 outputs); the narrow shape's time grows with the outputs (1.5 ms at 16 x 1485, 3.2 ms at
  // 64 x 1485, 16.3 ms at 256 x 1485)
  if (packed) return 5ll << 16;                      // 327 680: 4 rows cross near 3.5e5 (C3), 20 rows near 3.4e5 (1200 x 1000 protein)
  return S == 4 ? 15ll << 14 : 17ll << 14;           // 245 760 | 278 528: near 2.45e5 and 2.75e5 (32 rows: not measured, the 20-row line)
}

hipError_t launch_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br, const uint32_t *qslot,
                              int n_query, uint32_t *delta, int ld, int tile)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (g.sankoff || g.Wp <= 0 || g.Wp % 32 || ld < n_br) return hipErrorInvalidValue;
  if (n_br <= 0 || n_query <= 0) return hipSuccess;
  const bool narrow = place_pick(n_query, n_br, tile, place_narrow_below()) == PLACE_NARROW;
  dispatch_states(g.S, [&](auto S) { launch_shape<PlaceFitch<S>>(st, narrow, vec, desc, n_br, qslot, n_query, g.Wp, nullptr, delta, ld); });
  return hipGetLastError();
}

hipError_t launch_snk_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                                  const uint32_t *qslot, int n_query, uint32_t *out, int ld, int tile, bool wide_addr)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (!g.sankoff || !g.moff || !g.pwgt || g.Wp <= 0 || g.Wp % 32 || ld < n_br) return hipErrorInvalidValue;
  if (n_br <= 0 || n_query <= 0) return hipSuccess;
  const bool narrow = place_pick(n_query, n_br, tile, place_snk_narrow_below(g.S, g.snk16 != 0)) == PLACE_NARROW;
  const bool big = wide_addr || (unsigned long long)g.moff * 4ull >= (1ull << 32);
  dispatch_snk(g, [&](auto S, auto PK) {
    dispatch_bool(big, [&](auto BIG) {
      launch_shape<PlaceMinPlus<S, PK, BIG>>(st, narrow, vec + g.moff, desc, n_br, qslot, n_query, PK ? g.Wp / 2 : g.Wp, g.pwgt, out, ld);
    });
  });
  return hipGetLastError();
}

hipError_t launch_place_best(hipStream_t st, const uint32_t *delta, int n_br, int n_query, int ld, uint32_t *best)
{
  if (n_br <= 0 || n_query <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_place_best, dim3((unsigned)n_query), dim3(64), 0, st, delta, n_br, ld, best);
  return hipGetLastError();
}

}  // namespace mpf
