// polytomy.hip -- directional views of a MULTIFURCATING tree on gfx950 (host/polytomy.cpp).
//
// The reference scores a node of degree > 3 by its generic rules, which are not the bifurcating rule on some binary resolution:
//   Fitch    (PhyloTree::computePartialParsimony, phylotree.cpp:869-931): the set of a node is the AND of ALL its children's sets;
//            where that is empty it is the OR of all of them and ONE step is counted, whatever the degree;
//   weighted (ParsTree::computePartialParsimony, parstree.cpp:191-214): the cost row of a node is the sum over all children of the
//            child's min-plus transform.
// Branch lengths need both sides of every branch, i.e. every directed view.  A node of degree d has d inputs (the views of its
// neighbours towards it) and d outputs, output k being the rule over the inputs other than k.  The work per node is O(d):
//   Fitch: four accumulators per state row and 32-site word over the inputs,
//            Z1 / Z2 = at least one / at least two inputs have a 0 there,  O1 / O2 = the same for 1s,
//          and then, from a second read of input k alone,
//            AND_{j != k} = ~Z2 & (~Z1 | ~in_k),   OR_{j != k} = O2 | (O1 & ~in_k);
//          the view is the AND where some row of it is non-empty, else the OR; the step mask is ~OR_rows(AND);
//   weighted: T = the sum of all inputs' stored transforms (Geometry::moff); output k = T - m(in_k), then its own transform.
//          Sums are formed in 32 bits on either store: in the 16-bit store the two costs of a word are unpacked first, so a
//          node of any degree cannot overflow a lane half (the results are bounded as the binary engine's are and fit again).
// No indexed registers and no LDS: the accumulators are plain register arrays with compile-time indices.
//
// Schedule: sites are independent, so ONE workgroup owns a tile of TW words (elements) of every row for the whole tree and walks the
// items level by level with a workgroup barrier between levels, as k_newview_wg does: up views (towards the root leaf) by height
// from the tips, the root edge, then down views by depth, each node's accumulators formed once and d - 1 outputs written.  One
// launch per tree.  A thread is (node lane, word of the tile): 256 / TW items of a level are in flight per workgroup.
#include "kernels.hpp"

namespace mpf {

constexpr uint32_t kNone = 0xFFFFFFFFu;

template <int S>
__device__ __forceinline__ void poly_load(uint32_t (&t)[S], const uint32_t *vec, uint32_t slot, size_t Wp, size_t w)
{
  const uint32_t *p = vec + (size_t)slot * (size_t)S * Wp + w;
#pragma unroll
  for (int k = 0; k < S; k++) t[k] = p[(size_t)k * Wp];
}

template <int S, int TW>
__global__ __launch_bounds__(256) void k_poly_views(uint32_t *vec, const PolyItem *__restrict__ items, const PolyOut *__restrict__ outs,
                                                    const uint32_t *__restrict__ inputs, const int32_t *__restrict__ lev_off, int n_lev,
                                                    uint32_t *__restrict__ masks, int Wp_)
{
  constexpr int NL = 256 / TW;
  const size_t Wp = (size_t)Wp_;
  const int nl = (int)threadIdx.x / TW;
  const size_t w = (size_t)blockIdx.x * TW + (threadIdx.x % TW);      // (Wp is a multiple of TW: every thread has a word)
  for (int l = 0; l < n_lev; l++) {
    const int b = lev_off[l], e = lev_off[l + 1];
    for (int i = b + nl; i < e; i += NL) {
      const PolyItem it = items[i];
      uint32_t z1[S], z2[S], o1[S], o2[S];
#pragma unroll
      for (int k = 0; k < S; k++) z1[k] = z2[k] = o1[k] = o2[k] = 0u;
      for (uint32_t j = 0; j < it.n_in; j++) {
        uint32_t x[S];
        poly_load<S>(x, vec, inputs[it.in_begin + j], Wp, w);
#pragma unroll
        for (int k = 0; k < S; k++) {
          z2[k] |= z1[k] & ~x[k];
          z1[k] |= ~x[k];
          o2[k] |= o1[k] & x[k];
          o1[k] |= x[k];
        }
      }
      for (uint32_t q = 0; q < it.n_out; q++) {
        const PolyOut o = outs[it.out_begin + q];
        uint32_t a[S], r[S], any = 0u;
        if (o.excl == kNone) {
#pragma unroll
          for (int k = 0; k < S; k++) { a[k] = ~z1[k]; r[k] = o1[k]; any |= a[k]; }
        } else {
          uint32_t x[S];
          poly_load<S>(x, vec, o.excl, Wp, w);
#pragma unroll
          for (int k = 0; k < S; k++) {
            a[k] = ~z2[k] & (~z1[k] | ~x[k]);
            r[k] = o2[k] | (o1[k] & ~x[k]);
            any |= a[k];
          }
        }
        if (o.dst != kNone) {
          uint32_t *d = vec + (size_t)o.dst * (size_t)S * Wp + w;
#pragma unroll
          for (int k = 0; k < S; k++) d[(size_t)k * Wp] = a[k] | (~any & r[k]);
        }
        if (o.mask_row != kNone) masks[(size_t)o.mask_row * Wp + w] = ~any;
      }
    }
    __syncthreads();
  }
}

// weighted: one 32-bit element of the store per thread (PK: two 16-bit costs, worked on as two 32-bit values)
template <int S, bool PK>
__device__ __forceinline__ void snk_load(uint32_t (&t)[S][PK ? 2 : 1], const uint32_t *vec, uint32_t slot, size_t We, size_t e)
{
  const uint32_t *p = vec + (size_t)slot * (size_t)S * We + e;
#pragma unroll
  for (int k = 0; k < S; k++) {
    const uint32_t v = p[(size_t)k * We];
    if constexpr (PK) { t[k][0] = v & 0xFFFFu; t[k][1] = v >> 16; }
    else t[k][0] = v;
  }
}

template <int S, bool PK>
__device__ __forceinline__ void snk_store(const uint32_t (&t)[S][PK ? 2 : 1], uint32_t *vec, uint32_t slot, size_t We, size_t e)
{
  uint32_t *p = vec + (size_t)slot * (size_t)S * We + e;
#pragma unroll
  for (int k = 0; k < S; k++) {
    if constexpr (PK) p[(size_t)k * We] = (t[k][0] & 0xFFFFu) | (t[k][1] << 16);
    else p[(size_t)k * We] = t[k][0];
  }
}

template <int S, bool PK, int TW>
__global__ __launch_bounds__(256) void k_poly_snk_views(uint32_t *vec, size_t moff, const PolyItem *__restrict__ items,
                                                        const PolyOut *__restrict__ outs, const uint32_t *__restrict__ inputs,
                                                        const int32_t *__restrict__ lev_off, int n_lev, const uint32_t *__restrict__ cost,
                                                        int We_)
{
  constexpr int NL = 256 / TW, NP = PK ? 2 : 1;
  const size_t We = (size_t)We_;
  const int nl = (int)threadIdx.x / TW;
  const size_t e0 = (size_t)blockIdx.x * TW + (threadIdx.x % TW);
  uint32_t *mvec = vec + moff;
  for (int l = 0; l < n_lev; l++) {
    const int b = lev_off[l], e = lev_off[l + 1];
    for (int i = b + nl; i < e; i += NL) {
      const PolyItem it = items[i];
      uint32_t tot[S][NP];
#pragma unroll
      for (int k = 0; k < S; k++)
#pragma unroll
        for (int h = 0; h < NP; h++) tot[k][h] = 0u;
      for (uint32_t j = 0; j < it.n_in; j++) {
        uint32_t x[S][NP];
        snk_load<S, PK>(x, mvec, inputs[it.in_begin + j], We, e0);
#pragma unroll
        for (int k = 0; k < S; k++)
#pragma unroll
          for (int h = 0; h < NP; h++) tot[k][h] += x[k][h];
      }
      for (uint32_t q = 0; q < it.n_out; q++) {
        const PolyOut o = outs[it.out_begin + q];
        uint32_t c[S][NP], m[S][NP];
        if (o.excl == kNone) {
#pragma unroll
          for (int k = 0; k < S; k++)
#pragma unroll
            for (int h = 0; h < NP; h++) c[k][h] = tot[k][h];
        } else {
          uint32_t x[S][NP];
          snk_load<S, PK>(x, mvec, o.excl, We, e0);
#pragma unroll
          for (int k = 0; k < S; k++)
#pragma unroll
            for (int h = 0; h < NP; h++) c[k][h] = tot[k][h] - x[k][h];
        }
        // m[z] = min_x(c[x] + cost[z][x]) (the viewer is the parent: the rows of the matrix), as mplus in kernels.hip
#pragma unroll
        for (int z = 0; z < S; z++) {
#pragma unroll
          for (int h = 0; h < NP; h++) m[z][h] = 0xFFFFFFFFu;
#pragma unroll
          for (int x = 0; x < S; x++) {
            const uint32_t cz = cost[z * S + x] & 0xFFFFu;           // (the 16-bit store's matrix holds c | c << 16)
#pragma unroll
            for (int h = 0; h < NP; h++) m[z][h] = min(m[z][h], c[x][h] + cz);
          }
        }
        snk_store<S, PK>(c, vec, o.dst, We, e0);
        snk_store<S, PK>(m, mvec, o.dst, We, e0);
      }
    }
    __syncthreads();
  }
}

// cnt[row] = set bits of mask row `row` (one wave per row: no atomics, the same sum every run)
__global__ __launch_bounds__(64) void k_poly_rowsum(const uint32_t *__restrict__ masks, int Wp, uint32_t *__restrict__ cnt)
{
  const uint32_t *row = masks + (size_t)blockIdx.x * (size_t)Wp;
  uint32_t s = 0;
  for (int w = (int)threadIdx.x; w < Wp; w += 64) s += (uint32_t)__popc(row[w]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += (uint32_t)__shfl_xor((int)s, off, 64);
  if (threadIdx.x == 0) cnt[blockIdx.x] = s;
}

// the mask rows of a tree added per site into bit-sliced counter planes, kPlaneChunk rows per chunk: k_site_planes' layout with the
// masks read instead of formed from two vectors (a k-ary node's mask is no join of two stored vectors), for k_pattern_sum
__global__ __launch_bounds__(256) void k_poly_planes(const uint32_t *__restrict__ masks, int n_rows, uint32_t *__restrict__ planes, int Wp)
{
  const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int chunk = (int)blockIdx.y;
  if (w >= Wp) return;
  uint32_t c[kPlanes];
#pragma unroll
  for (int j = 0; j < kPlanes; j++) c[j] = 0u;
  const int b = chunk * kPlaneChunk, e = min(n_rows, b + kPlaneChunk);
  for (int i = b; i < e; i++) {
    uint32_t carry = masks[(size_t)i * (size_t)Wp + w];
#pragma unroll
    for (int j = 0; j < kPlanes; j++) {
      const uint32_t t = c[j] & carry;
      c[j] ^= carry;
      carry = t;
    }
  }
#pragma unroll
  for (int j = 0; j < kPlanes; j++) planes[((size_t)chunk * kPlanes + j) * (size_t)Wp + w] = c[j];
}

// ---------------------------------------------------------------- launch wrappers

int poly_tile(int W, int want)
{
  if (want == 4 || want == 8 || want == 16 || want == 32) return (W % want == 0) ? want : 16;
  int tw = (W % 32 == 0) ? 32 : 16;
  while (tw > 4 && W / tw < 128) tw /= 2;                           // (enough workgroups for the device before wider row segments)
  return tw;
}

template <class F> static decltype(auto) dispatch_tw(int tw, F &&f)
{
  if (tw == 4) return f(int_c<4>());
  if (tw == 8) return f(int_c<8>());
  if (tw == 16) return f(int_c<16>());
  return f(int_c<32>());
}

hipError_t launch_poly_views(hipStream_t st, const Geometry &g, uint32_t *vec, const PolyItem *items, const PolyOut *outs,
                             const uint32_t *inputs, const int32_t *lev_off, int n_lev, uint32_t *masks, int tile)
{
  if (!vec) return hipErrorInvalidValue;            // (Engine::vec_rows: the rows could not be brought up to date)
  if (n_lev <= 0) return hipSuccess;
  if (g.sankoff) {
    const int We = g.snk16 ? g.Wp / 2 : g.Wp;
    const int tw = poly_tile(We, tile);
    dispatch_snk(g, [&](auto S, auto PK) {
      dispatch_tw(tw, [&](auto TW) {
        hipLaunchKernelGGL((k_poly_snk_views<S, PK, TW>), dim3(We / tw), dim3(256), 0, st, vec, g.moff, items, outs, inputs, lev_off, n_lev,
                           g.cost, We);
      });
    });
  } else {
    const int tw = poly_tile(g.Wp, tile);
    dispatch_states(g.S, [&](auto S) {
      dispatch_tw(tw, [&](auto TW) {
        hipLaunchKernelGGL((k_poly_views<S, TW>), dim3(g.Wp / tw), dim3(256), 0, st, vec, items, outs, inputs, lev_off, n_lev, masks, g.Wp);
      });
    });
  }
  return hipGetLastError();
}

hipError_t launch_poly_rowsum(hipStream_t st, const Geometry &g, const uint32_t *masks, int n_rows, uint32_t *cnt)
{
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_poly_rowsum, dim3(n_rows), dim3(64), 0, st, masks, g.Wp, cnt);
  return hipGetLastError();
}

hipError_t launch_poly_site_counts(hipStream_t st, const Geometry &g, const uint32_t *masks, int n_rows, uint32_t *planes,
                                   const int32_t *ptn_first_site, int n_ptn, uint16_t *ptn_out)
{
  if (n_rows <= 0) return hipSuccess;
  const int n_chunks = (n_rows + kPlaneChunk - 1) / kPlaneChunk;
  hipLaunchKernelGGL(k_poly_planes, dim3((g.Wp + 255) / 256, n_chunks), dim3(256), 0, st, masks, n_rows, planes, g.Wp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_pattern_sum(st, g, planes, n_chunks, ptn_first_site, n_ptn, ptn_out);
}

}  // namespace mpf
