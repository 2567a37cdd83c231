// splits.hip -- the bipartitions (splits) of a weighted set of complete trees on the same n taxa, counted exactly (gfx950, wave64).
//
// What the reference does through Newick strings, Split objects and a hash map (MTreeSet::convertSplits, mtreeset.cpp:288-470),
// on the trees as the engine holds them (back[] records):
//
//   k_split_keys     one workgroup per tree.  The records go into LDS, one lane walks the tree from tip 1: pos[tip] = the tip's
//                    index in DFS order, and every inner branch but the one at tip 1 is an interval [lo, hi) of that order -- its
//                    cluster, the side without tip 1 (the normal form of trees.splits).  The cluster's 64-bit key is the wrapping
//                    sum of a per-taxon constant (splitmix64 of the taxon number) over its tips, taken as the difference of the
//                    running sum at hi and at lo.  It depends on the SET alone: not on node numbers, slot order or walk order.
//   k_split_insert   every cluster claims a slot of an open-addressing table in HBM by a 64-bit atomicCAS on the key (linear
//                    probing, bounded by the table size); the slot's representative is the smallest cluster number (atomicMin).
//   k_split_count    a launch of its own behind the insert launch: every cluster is compared with its slot's representative AS A
//                    SET (equal sizes, and every tip of its interval inside the other's interval, read through the two pos
//                    arrays: no n-bit set in memory).  Equal: the tree's weight is added to the slot's 64-bit count.  Not equal:
//                    a true key collision, the cluster goes to an overflow list that the host resolves exactly.
//   k_split_compact  the used slots as a dense list (representative, count).
//   k_split_gather   the counts of one tree's clusters (the supports of a target tree).
//   k_split_bits     the n-bit sets of the clusters that are handed out: a lane makes a word from 32 pos comparisons.
//
// The key only routes; what decides is the set comparison.  No kernel waits for another workgroup: every atomic either returns
// at once or is not looked at again before the next launch.
#include "splits.hpp"

namespace mpf {

namespace {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

constexpr unsigned long long kTaxonSalt = 0x6D70626F6F745F73ull;

__device__ __forceinline__ int ring_next(int r) { const int v = r / 3, s = r - 3 * v; return 3 * v + (s == 2 ? 0 : s + 1); }

// grid: n_trees; any block size.  LDS: split_keys_lds_bytes(n).  bad[t] != 0: tree t's records are not one tree over all n tips
// (the walk is bounded by the node counts of a tree, so a malformed one ends it early instead of running on)
__global__ void __launch_bounds__(256) k_split_keys(const int32_t *__restrict__ backs, int n, int key_bits, int32_t *__restrict__ pos,
                                                    int32_t *__restrict__ order, SplitCluster *__restrict__ cl, int32_t *__restrict__ bad)
{
  extern __shared__ int32_t lds[];
  const int len = 3 * (2 * n - 1), cap = 2 * n + 4, C = n - 3;
  int32_t *bk = lds, *stk = lds + len;
  const size_t t = blockIdx.x;
  const int32_t *src = backs + t * (size_t)len;
  for (int i = threadIdx.x; i < len; i += blockDim.x) bk[i] = src[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  int32_t *my_pos = pos + t * (size_t)n, *my_order = order + t * (size_t)(n - 1);
  SplitCluster *my_cl = cl + t * (size_t)C;
  const unsigned long long mask = key_bits >= 64 ? ~0ull : ((1ull << key_bits) - 1ull);
  int sp = 0, cnt = 0, inner = 0, err = 0;
  unsigned long long acc = 0;
  if (bk[3] >= 3) stk[sp++] = bk[3];
  while (sp > 0) {
    const int x = stk[--sp];
    if (x < 0) {                                   // the cluster opened at -(x + 1) closes: its key is the sum since then
      SplitCluster &c = my_cl[-x - 1];
      unsigned long long k = (acc - c.key) & mask;
      if (k == kSplitEmpty) k = kSplitEmpty - 1;
      c.hi = (uint32_t)cnt;
      c.key = k;
      continue;
    }
    if (x < 3 || x >= len) { err = 1; break; }
    const int v = x / 3;
    if (v <= n) {
      if (v == 1 || cnt >= n - 1) { err = 1; break; }
      my_pos[v - 1] = cnt;
      my_order[cnt++] = v;
      acc += splitmix64(kTaxonSalt ^ (unsigned long long)v);
      continue;
    }
    if (inner >= n - 2 || sp + 3 > cap) { err = 1; break; }
    const int ci = inner++ - 1;                    // the node next to tip 1 holds every other tip: no split
    if (ci >= 0) {
      my_cl[ci].lo = (uint32_t)cnt;
      my_cl[ci].key = acc;                         // (parked here until the cluster closes)
      stk[sp++] = -(ci + 1);
    }
    const int a = ring_next(x), b = ring_next(a);
    if (bk[a] < 3 || bk[b] < 3) { err = 1; break; }  // (an unused record: only a negative entry the walk made itself closes a cluster)
    stk[sp++] = bk[b];
    stk[sp++] = bk[a];
  }
  my_pos[0] = n - 1;                               // tip 1: outside every interval
  bad[t] = (err || cnt != n - 1 || inner != n - 2) ? 1 : 0;
}

__device__ __forceinline__ uint32_t slot_hash(unsigned long long k) { return (uint32_t)(splitmix64(k) >> 17); }

// one thread per cluster
__global__ void __launch_bounds__(256) k_split_insert(const SplitCluster *__restrict__ cl, uint32_t n_clusters, unsigned long long *tkey,
                                                      unsigned long long *trep, uint32_t tsize, uint32_t *__restrict__ slot_of)
{
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_clusters) return;
  const unsigned long long k = cl[g].key;
  const uint32_t tmask = tsize - 1;
  uint32_t h = slot_hash(k) & tmask, got = kSplitNoSlot;
  for (uint32_t i = 0; i < tsize; i++) {
    const unsigned long long old = atomicCAS(&tkey[h], kSplitEmpty, k);
    if (old == kSplitEmpty || old == k) { got = h; break; }
    h = (h + 1) & tmask;
  }
  // (the table has at least twice as many slots as there are clusters: the probe always ends on a slot)
  if (got != kSplitNoSlot) atomicMin(&trep[got], (unsigned long long)g);
  slot_of[g] = got;
}

// one lane per cluster, the set comparisons of a wave's 64 clusters done by the whole wave one after the other: 64 lanes stride
// over the interval, coalesced on order[], one vote.  counters[0]: length of the overflow list
__global__ void __launch_bounds__(256) k_split_count(const SplitCluster *__restrict__ cl, uint32_t n_clusters, int n, const int32_t *__restrict__ pos,
                                                     const int32_t *__restrict__ order, const unsigned long long *__restrict__ trep,
                                                     uint32_t *__restrict__ slot_of, const int32_t *__restrict__ weights, unsigned long long *tcount,
                                                     uint32_t *__restrict__ ovf, uint32_t *counters)
{
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t C = (uint32_t)(n - 3);
  const bool live = g < n_clusters;
  uint32_t lo = 0, hi = 0, tg = 0, tr = 0, rlo = 0, rhi = 0, h = kSplitNoSlot;
  bool eq = false, need = false;
  if (live) {
    h = slot_of[g];
    lo = cl[g].lo;
    hi = cl[g].hi;
    tg = g / C;
    if (h != kSplitNoSlot) {
      const uint32_t r = (uint32_t)trep[h];
      if (r == g) eq = true;
      else {
        tr = r / C;
        rlo = cl[r].lo;
        rhi = cl[r].hi;
        // two clusters of one tree are two different sets; sets of different sizes are different
        need = tr != tg && rhi - rlo == hi - lo;
      }
    }
  }
  unsigned long long todo = __ballot(need);
  while (todo) {
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t jlo = __shfl(lo, j), jhi = __shfl(hi, j), jtg = __shfl(tg, j), jtr = __shfl(tr, j), jrlo = __shfl(rlo, j), jrhi = __shfl(rhi, j);
    const int32_t *ord = order + (size_t)jtg * (size_t)(n - 1), *rpos = pos + (size_t)jtr * (size_t)n;
    bool ok = true;
    for (uint32_t p = jlo + (uint32_t)lane; p < jhi; p += 64) {
      const uint32_t q = (uint32_t)rpos[ord[p] - 1];
      ok = ok && q >= jrlo && q < jrhi;
    }
    const bool all = __all(ok);
    if (lane == j) eq = all;
  }
  if (!live) return;
  if (eq) atomicAdd(&tcount[h], (unsigned long long)weights[tg]);
  else {
    ovf[atomicAdd(&counters[0], 1u)] = g;          // (at most n_clusters entries: every cluster comes here once)
    slot_of[g] = kSplitNoSlot;
  }
}

// one thread per slot.  counters[1]: number of entries
__global__ void __launch_bounds__(256) k_split_compact(const unsigned long long *__restrict__ trep, const unsigned long long *__restrict__ tcount,
                                                       uint32_t tsize, SplitEntry *__restrict__ out, uint32_t *counters)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= tsize) return;
  const unsigned long long r = trep[s];
  if (r == kSplitEmpty) return;
  out[atomicAdd(&counters[1], 1u)] = SplitEntry{(uint32_t)r, s, tcount[s]};
}

// out[i] = the count of the slot of cluster first + i, -1 if that cluster is on the overflow list
__global__ void __launch_bounds__(256) k_split_gather(const uint32_t *__restrict__ slot_of, uint32_t first, uint32_t m,
                                                      const unsigned long long *__restrict__ tcount, long long *__restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t h = slot_of[first + i];
  out[i] = h == kSplitNoSlot ? -1ll : (long long)tcount[h];
}

// one thread per (listed cluster, word): bit b of word j = tip 32 j + b + 1 lies in the cluster
__global__ void __launch_bounds__(256) k_split_bits(const SplitCluster *__restrict__ cl, const uint32_t *__restrict__ ids, uint32_t m, int n,
                                                    const int32_t *__restrict__ pos, uint32_t *__restrict__ bits)
{
  const uint32_t words = (uint32_t)(n + 31) >> 5;
  const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (unsigned long long)m * words) return;
  const uint32_t i = (uint32_t)(idx / words), j = (uint32_t)(idx % words);
  const uint32_t g = ids[i], t = g / (uint32_t)(n - 3);
  const uint32_t lo = cl[g].lo, hi = cl[g].hi;
  const int32_t *p = pos + (size_t)t * (size_t)n;
  uint32_t w = 0;
  for (int b = 0; b < 32; b++) {
    const int tip0 = (int)(32 * j) + b;
    if (tip0 < n) {
      const uint32_t q = (uint32_t)p[tip0];
      w |= (uint32_t)(q >= lo && q < hi) << b;
    }
  }
  bits[idx] = w;
}

inline unsigned blocks_for(unsigned long long items) { return (unsigned)((items + 255) / 256); }

}  // namespace

hipError_t launch_split_keys(hipStream_t st, const int32_t *backs, int n_trees, int n, int key_bits, int32_t *pos, int32_t *order,
                             SplitCluster *cl, int32_t *bad)
{
  if (n < 4 || n > kSplitMaxTaxa || n_trees < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_split_keys, dim3((unsigned)n_trees), dim3(256), split_keys_lds_bytes(n), st, backs, n, key_bits, pos, order, cl, bad);
  return hipGetLastError();
}

hipError_t launch_split_insert(hipStream_t st, const SplitCluster *cl, uint32_t n_clusters, unsigned long long *tkey, unsigned long long *trep,
                               uint32_t tsize, uint32_t *slot_of)
{
  if (!n_clusters || (tsize & (tsize - 1)) || (unsigned long long)tsize < 2ull * n_clusters) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_split_insert, dim3(blocks_for(n_clusters)), dim3(256), 0, st, cl, n_clusters, tkey, trep, tsize, slot_of);
  return hipGetLastError();
}

hipError_t launch_split_count(hipStream_t st, const SplitCluster *cl, uint32_t n_clusters, int n, const int32_t *pos, const int32_t *order,
                              const unsigned long long *trep, uint32_t *slot_of, const int32_t *weights, unsigned long long *tcount,
                              uint32_t *ovf, uint32_t *counters)
{
  hipLaunchKernelGGL(k_split_count, dim3(blocks_for(n_clusters)), dim3(256), 0, st, cl, n_clusters, n, pos, order, trep, slot_of, weights, tcount,
                     ovf, counters);
  return hipGetLastError();
}

hipError_t launch_split_compact(hipStream_t st, const unsigned long long *trep, const unsigned long long *tcount, uint32_t tsize, SplitEntry *out,
                                uint32_t *counters)
{
  hipLaunchKernelGGL(k_split_compact, dim3(blocks_for(tsize)), dim3(256), 0, st, trep, tcount, tsize, out, counters);
  return hipGetLastError();
}

hipError_t launch_split_gather(hipStream_t st, const uint32_t *slot_of, uint32_t first, uint32_t m, const unsigned long long *tcount, long long *out)
{
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_split_gather, dim3(blocks_for(m)), dim3(256), 0, st, slot_of, first, m, tcount, out);
  return hipGetLastError();
}

hipError_t launch_split_bits(hipStream_t st, const SplitCluster *cl, const uint32_t *ids, uint32_t m, int n, const int32_t *pos, uint32_t *bits)
{
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_split_bits, dim3(blocks_for((unsigned long long)m * (unsigned)((n + 31) / 32))), dim3(256), 0, st, cl, ids, m, n, pos, bits);
  return hipGetLastError();
}

}  // namespace mpf
