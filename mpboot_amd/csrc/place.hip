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
// queries x TB branches and walks the row in slices of KS words.  Both operands of a slice go through LDS; the branch operand is
// loaded as its two views and JOINED on the way in, so X never exists in HBM and one query costs no extra pass.  The next slice's
// global loads are issued before this slice's arithmetic.  A lane holds RQ x RB outputs; per (query, branch, word) the work is S
// v_and / v_and_or and one v_bcnt with accumulate.  In the narrow shape the 256 lanes also split the words of a slice KT ways and
// the partial sums meet in LDS at the end -- every output has one writer, no atomics, the same sum every run.  No workgroup waits
// on another.
//
// k_snk_place_costs, further down, is the same scheme on the weighted (-cost) engine: a min-plus product over the stored transforms.
#include "place.hpp"
#include "snk_elem.hpp"

namespace mpf {

namespace {

template <int S, int TQ, int TB, int RQ, int RB, int KS, int KT>
__global__ __launch_bounds__(256) void k_place_costs(const uint32_t *__restrict__ vec, const BranchDesc *__restrict__ desc, int n_br,
                                                     const uint32_t *__restrict__ qslot, int n_query, int Wp_, uint32_t *__restrict__ delta,
                                                     int ld)
{
  constexpr int TBT = TB / RB, TQT = TQ / RQ;
  static_assert(TBT * TQT * KT == 256 && TB % RB == 0 && TQ % RQ == 0 && KS % KT == 0, "lane mapping");
  static_assert(KT == 1 || KT * TQ * TB <= KS * (S * TB + 64 / KS), "the partial sums reuse the branch slice");
  static_assert(64 % KS == 0 && (64 / KS) % 4 == 0, "padding keeps the 16-byte alignment");
  constexpr int BI = (TB * KS + 255) / 256, QI = (TQ * KS + 255) / 256;      // staged (vector, word) items per lane
  // [word of the slice][state row][branch | query], 64 / KS words of padding behind every word of the slice: the staging stores of a
  // wave (KS consecutive words of 64 / KS vectors) then fall on 64 different banks, and every row still starts on 16 bytes
  constexpr int XP = S * TB + 64 / KS, QP = S * TQ + 64 / KS;
  __shared__ __attribute__((aligned(16))) uint32_t sx[KS * XP];
  __shared__ __attribute__((aligned(16))) uint32_t sq[KS * QP];
  const size_t Wp = (size_t)Wp_;
  const int tid = (int)threadIdx.x;
  const int tb = tid % TBT, tq = (tid / TBT) % TQT, kt = tid / (TBT * TQT);

  // staging: item idx -> vector idx / KS of the tile, word idx % KS of the slice (a lane group reads KS consecutive words of a row)
  const uint32_t *pa[BI], *pb[BI], *pq[QI];
#pragma unroll
  for (int i = 0; i < BI; i++) {
    const int idx = tid + 256 * i;
    const int b = min((int)blockIdx.x * TB + min(idx / KS, TB - 1), n_br - 1);      // (rows past the end repeat the last: loads stay inside)
    const BranchDesc d = desc[b];
    pa[i] = vec + (size_t)d.a * (size_t)S * Wp + (size_t)(idx % KS);
    pb[i] = vec + (size_t)d.b * (size_t)S * Wp + (size_t)(idx % KS);
  }
#pragma unroll
  for (int i = 0; i < QI; i++) {
    const int idx = tid + 256 * i;
    const int q = min((int)blockIdx.y * TQ + min(idx / KS, TQ - 1), n_query - 1);
    pq[i] = vec + (size_t)qslot[q] * (size_t)S * Wp + (size_t)(idx % KS);
  }
  uint32_t ra[BI][S], rb[BI][S], rq[QI][S];
  auto fetch = [&](size_t k0) {
#pragma unroll
    for (int i = 0; i < BI; i++)
      if (tid + 256 * i < TB * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) { ra[i][s] = pa[i][(size_t)s * Wp + k0]; rb[i][s] = pb[i][(size_t)s * Wp + k0]; }
      }
#pragma unroll
    for (int i = 0; i < QI; i++)
      if (tid + 256 * i < TQ * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) rq[i][s] = pq[i][(size_t)s * Wp + k0];
      }
  };
  fetch(0);

  uint32_t acc[RQ][RB];
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) acc[i][j] = 0u;

  for (size_t k0 = 0; k0 < Wp; k0 += KS) {                   // (Wp is a multiple of 32, KS divides 32)
    __syncthreads();                                         // the last slice has been read by everybody
#pragma unroll
    for (int i = 0; i < BI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TB * KS) {
        uint32_t any = 0u;
#pragma unroll
        for (int s = 0; s < S; s++) any |= ra[i][s] & rb[i][s];
        uint32_t *d = &sx[(idx % KS) * XP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++) d[s * TB] = (ra[i][s] & rb[i][s]) | (~any & (ra[i][s] | rb[i][s]));
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
    __syncthreads();
    if (k0 + KS < Wp) fetch(k0 + KS);                        // the next slice is on its way while this one is counted
#pragma unroll 2
    for (int k = kt; k < KS; k += KT) {
      uint32_t m[RQ][RB];
#pragma unroll
      for (int i = 0; i < RQ; i++)
#pragma unroll
        for (int j = 0; j < RB; j++) m[i][j] = 0u;
#pragma unroll
      for (int s = 0; s < S; s++) {
        uint32_t xv[RB], qv[RQ];
#pragma unroll
        for (int j = 0; j < RB; j++) xv[j] = sx[k * XP + s * TB + tb * RB + j];
#pragma unroll
        for (int i = 0; i < RQ; i++) qv[i] = sq[k * QP + s * TQ + tq * RQ + i];
#pragma unroll
        for (int i = 0; i < RQ; i++)
#pragma unroll
          for (int j = 0; j < RB; j++) m[i][j] |= qv[i] & xv[j];
      }
#pragma unroll
      for (int i = 0; i < RQ; i++)
#pragma unroll
        for (int j = 0; j < RB; j++) acc[i][j] += (uint32_t)__popc(m[i][j]);
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
  const uint32_t bits = 32u * (uint32_t)Wp_;
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int q = (int)blockIdx.y * TQ + tq * RQ + i, b = (int)blockIdx.x * TB + tb * RB + j;
      if (q < n_query && b < n_br) delta[(size_t)q * (size_t)ld + (size_t)b] = bits - acc[i][j];
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
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t ov = (uint32_t)__shfl_xor((int)v, off, 64), oat = (uint32_t)__shfl_xor((int)at, off, 64);
    if (ov < v || (ov == v && oat < at)) { v = ov; at = oat; }
  }
  if (threadIdx.x == 0) { best[2 * blockIdx.x] = v; best[2 * blockIdx.x + 1] = at; }
}

// ---------------------------------------------------------------- the weighted (-cost) engine
//
// On a ParsTree addTaxonMPFast's score is the FULL length of the completed tree evaluated at the new taxon's edge
// (computeParsimonyBranch(added_node->neighbors[0], added_node), parstree.cpp:439-541; the leaf swap at :449-457 makes the taxon
// the transformed side, the rest of the tree the rows of the matrix).  With A, B the two directed views of the branch and T the
// taxon's cost row, m() the min-plus transform with the viewer as the parent:
//   cost(q, b) = sum_ptn w * min_i( m(T_q)[i] + m(A_b)[i] + m(B_b)[i] )
// All three transforms are STORED (k_poly_snk_views and k_snk_pack write m(v) `moff` words behind v), so nothing is transformed
// here.  16-bit store: a sum of three transforms over disjoint sides that hold at most n tips together -- the shape Engine::pack
// guards (3 n highest_cost < 65536).
//
// k_snk_place_costs is k_place_costs with min-plus for and-or: a tile of TQ queries x TB branches per workgroup, the row of We
// elements (patterns, or pairs of patterns in the 16-bit store) walked in slices of KS; the branch operand is loaded as the two
// transforms and ADDED on the way into LDS, so m(A) + m(B) never exists in HBM; the slice's pattern weights ride along.  Per
// (query, branch, element) a lane does S add / min pairs (v_pk_add_u16 / v_pk_min_u16 in the 16-bit store: two patterns each) and
// one weighted sum.  Padding elements have weight 0.  Narrow shape: KT lane classes split a slice, partial sums meet in LDS and
// are added in a fixed order.  One writer per output, no atomics, no workgroup waits on another.
// The element type is SnkT<PK> of the other weighted kernels (snk_elem.hpp).

// BIG: 64-bit element offsets (a transform half of 4 GiB or more); otherwise 32-bit offsets from the half's base
template <int S, bool PK, bool BIG, int TQ, int TB, int RQ, int RB, int KS, int KT>
__global__ __launch_bounds__(256) void k_snk_place_costs(const uint32_t *__restrict__ mvec, const BranchDesc *__restrict__ desc, int n_br,
                                                         const uint32_t *__restrict__ qslot, int n_query, int We_,
                                                         const uint32_t *__restrict__ pwgt, uint32_t *__restrict__ out, int ld)
{
  typedef SnkT<PK> T;
  typedef typename T::E E;
  typedef typename std::conditional<BIG, size_t, uint32_t>::type Off;
  constexpr int TBT = TB / RB, TQT = TQ / RQ, NP = PK ? 2 : 1;
  static_assert(TBT * TQT * KT == 256 && TB % RB == 0 && TQ % RQ == 0 && KS % KT == 0, "lane mapping");
  static_assert(KT == 1 || KT * TQ * TB <= KS * (S * TB + 64 / KS), "the partial sums reuse the branch slice");
  static_assert(64 % KS == 0 && (64 / KS) % 4 == 0 && 16 % KS == 0, "padding keeps the 16-byte alignment; a row is whole slices");
  static_assert(KS * NP <= 256, "one lane per weight of a slice");
  constexpr int BI = (TB * KS + 255) / 256, QI = (TQ * KS + 255) / 256;      // staged (vector, element) items per lane
  // [element of the slice][state row][branch | query], padded as k_place_costs pads
  constexpr int XP = S * TB + 64 / KS, QP = S * TQ + 64 / KS;
  __shared__ __attribute__((aligned(16))) uint32_t sx[KS * XP];
  __shared__ __attribute__((aligned(16))) uint32_t sq[KS * QP];
  __shared__ uint32_t sw[KS * NP];
  const Off We = (Off)We_;
  const int tid = (int)threadIdx.x;
  const int tb = tid % TBT, tq = (tid / TBT) % TQT, kt = tid / (TBT * TQT);

  Off oa[BI], ob[BI], oq[QI];
#pragma unroll
  for (int i = 0; i < BI; i++) {
    const int idx = tid + 256 * i;
    const int b = min((int)blockIdx.x * TB + min(idx / KS, TB - 1), n_br - 1);      // (rows past the end repeat the last: loads stay inside)
    const BranchDesc d = desc[b];
    oa[i] = (Off)d.a * (Off)S * We + (Off)(idx % KS);
    ob[i] = (Off)d.b * (Off)S * We + (Off)(idx % KS);
  }
#pragma unroll
  for (int i = 0; i < QI; i++) {
    const int idx = tid + 256 * i;
    const int q = min((int)blockIdx.y * TQ + min(idx / KS, TQ - 1), n_query - 1);
    oq[i] = (Off)qslot[q] * (Off)S * We + (Off)(idx % KS);
  }
  uint32_t ra[BI][S], rb[BI][S], rq[QI][S], rw = 0u;
  auto fetch = [&](Off k0) {
#pragma unroll
    for (int i = 0; i < BI; i++)
      if (tid + 256 * i < TB * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) { ra[i][s] = mvec[oa[i] + (Off)s * We + k0]; rb[i][s] = mvec[ob[i] + (Off)s * We + k0]; }
      }
#pragma unroll
    for (int i = 0; i < QI; i++)
      if (tid + 256 * i < TQ * KS) {
#pragma unroll
        for (int s = 0; s < S; s++) rq[i][s] = mvec[oq[i] + (Off)s * We + k0];
      }
    if (tid < KS * NP) rw = pwgt[(size_t)k0 * NP + (size_t)tid];
  };
  fetch(0);

  uint32_t acc[RQ][RB];
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) acc[i][j] = 0u;

  for (Off k0 = 0; k0 < We; k0 += KS) {                     // (We is a multiple of 16, KS divides 16)
    __syncthreads();                                         // the last slice has been read by everybody
#pragma unroll
    for (int i = 0; i < BI; i++) {
      const int idx = tid + 256 * i;
      if (idx < TB * KS) {
        uint32_t *d = &sx[(idx % KS) * XP + idx / KS];
#pragma unroll
        for (int s = 0; s < S; s++)
          d[s * TB] = __builtin_bit_cast(uint32_t, T::add(__builtin_bit_cast(E, ra[i][s]), __builtin_bit_cast(E, rb[i][s])));
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
    if (tid < KS * NP) sw[tid] = rw;
    __syncthreads();
    if (k0 + KS < We) fetch(k0 + KS);                        // the next slice is on its way while this one is summed
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
            const E t = T::add(qv[i], xv[j]);
            m[i][j] = s == 0 ? t : T::mn(m[i][j], t);
          }
      }
#pragma unroll
      for (int i = 0; i < RQ; i++)
#pragma unroll
        for (int j = 0; j < RB; j++) acc[i][j] += T::wsum(m[i][j], sw, k);
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
#pragma unroll
  for (int i = 0; i < RQ; i++)
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int q = (int)blockIdx.y * TQ + tq * RQ + i, b = (int)blockIdx.x * TB + tb * RB + j;
      if (q < n_query && b < n_br) out[(size_t)q * (size_t)ld + (size_t)b] = acc[i][j];
    }
}

template <int S, bool PK, int TQ, int TB, int RQ, int RB, int KS, int KT>
void launch_snk_shape(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br, const uint32_t *qslot,
                      int n_query, uint32_t *out, int ld, bool wide_addr)
{
  const dim3 grid((unsigned)((n_br + TB - 1) / TB), (unsigned)((n_query + TQ - 1) / TQ));
  const int We = PK ? g.Wp / 2 : g.Wp;
  dispatch_bool(wide_addr, [&](auto BIG) {
    hipLaunchKernelGGL((k_snk_place_costs<S, PK, BIG, TQ, TB, RQ, RB, KS, KT>), grid, dim3(256), 0, st, vec + g.moff, desc, n_br, qslot, n_query,
                       We, g.pwgt, out, ld);
  });
}

template <int S, int TQ, int TB, int RQ, int RB, int KS, int KT>
void launch_shape(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br, const uint32_t *qslot, int n_query,
                  uint32_t *delta, int ld)
{
  const dim3 grid((unsigned)((n_br + TB - 1) / TB), (unsigned)((n_query + TQ - 1) / TQ));
  hipLaunchKernelGGL((k_place_costs<S, TQ, TB, RQ, RB, KS, KT>), grid, dim3(256), 0, st, vec, desc, n_br, qslot, n_query, g.Wp, delta, ld);
}

}  // namespace

PlaceShape place_shape(int S, int tile)
{
  if (tile == PLACE_NARROW) return PlaceShape{4, 16, 16};
  return S == 4 ? PlaceShape{64, 64, 16} : PlaceShape{32, 32, 4};
}

int place_pick(int n_query, int n_br, int tile)
{
  if (tile == PLACE_NARROW || tile == PLACE_WIDE) return tile;
  // A wide workgroup walks the whole row alone, so a wide launch takes that long however few tiles it has; the narrow shape's time
  // grows with the outputs.  Measured on C3 (narrow 0.19 ms at 64 x 1485 outputs and 0.81 ms at 256 x 1485, wide 0.58 ms
  // at both) they cross near 2.7e5 outputs: sixty-four 64 x 64 tiles
  return (long long)n_query * (long long)n_br < 262144ll ? PLACE_NARROW : PLACE_WIDE;
}

hipError_t launch_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br, const uint32_t *qslot,
                              int n_query, uint32_t *delta, int ld, int tile)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (g.sankoff || g.Wp <= 0 || g.Wp % 32 || ld < n_br) return hipErrorInvalidValue;
  if (n_br <= 0 || n_query <= 0) return hipSuccess;
  const bool narrow = place_pick(n_query, n_br, tile) == PLACE_NARROW;
  dispatch_states(g.S, [&](auto S) {
    if (narrow) launch_shape<S, 4, 16, 4, 1, 16, 16>(st, g, vec, desc, n_br, qslot, n_query, delta, ld);
    else if constexpr (S == 4) launch_shape<S, 64, 64, 4, 4, 16, 1>(st, g, vec, desc, n_br, qslot, n_query, delta, ld);
    else launch_shape<S, 32, 32, 2, 2, 4, 1>(st, g, vec, desc, n_br, qslot, n_query, delta, ld);
  });
  return hipGetLastError();
}

PlaceShape place_snk_shape(int S, int tile)
{
  if (tile == PLACE_NARROW) return PlaceShape{4, 16, 16};
  return S == 32 ? PlaceShape{32, 32, 4} : (S == 20 ? PlaceShape{64, 64, 4} : PlaceShape{64, 64, 16});
}

long long place_snk_narrow_below(int S, bool packed)
{
  if (packed) return 5ll << 16;                      // 327 680: 4 rows cross near 3.5e5 (C3), 20 rows near 3.4e5 (1200 x 1000 protein)
  return S == 4 ? 15ll << 14 : 17ll << 14;           // 245 760 | 278 528: near 2.45e5 and 2.75e5 (32 rows: not measured, the 20-row line)
}

int place_snk_pick(int S, bool packed, int n_query, int n_br, int tile)
{
  if (tile == PLACE_NARROW || tile == PLACE_WIDE) return tile;
  // A wide workgroup walks the whole row alone, so a wide launch takes that long however few tiles it has (C3, 16-bit store: 15.1 -
  // 15.3 ms from 1 x 1995 to 256 x 1485 outputs); the narrow shape's time grows with the outputs (1.5 ms at 16 x 1485, 3.2 ms at
  // 64 x 1485, 16.3 ms at 256 x 1485)
  return (long long)n_query * (long long)n_br < place_snk_narrow_below(S, packed) ? PLACE_NARROW : PLACE_WIDE;
}

hipError_t launch_snk_place_costs(hipStream_t st, const Geometry &g, const uint32_t *vec, const BranchDesc *desc, int n_br,
                                  const uint32_t *qslot, int n_query, uint32_t *out, int ld, int tile, bool wide_addr)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (!g.sankoff || !g.moff || !g.pwgt || g.Wp <= 0 || g.Wp % 32 || ld < n_br) return hipErrorInvalidValue;
  if (n_br <= 0 || n_query <= 0) return hipSuccess;
  const bool narrow = place_snk_pick(g.S, g.snk16 != 0, n_query, n_br, tile) == PLACE_NARROW;
  const bool big = wide_addr || (unsigned long long)g.moff * 4ull >= (1ull << 32);
  dispatch_snk(g, [&](auto S, auto PK) {
    if (narrow) launch_snk_shape<S, PK, 4, 16, 4, 1, 16, 16>(st, g, vec, desc, n_br, qslot, n_query, out, ld, big);
    else if constexpr (S == 4) launch_snk_shape<S, PK, 64, 64, 4, 4, 16, 1>(st, g, vec, desc, n_br, qslot, n_query, out, ld, big);
    else if constexpr (S == 20) launch_snk_shape<S, PK, 64, 64, 4, 4, 4, 1>(st, g, vec, desc, n_br, qslot, n_query, out, ld, big);
    else launch_snk_shape<S, PK, 32, 32, 2, 2, 4, 1>(st, g, vec, desc, n_br, qslot, n_query, out, ld, big);
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
