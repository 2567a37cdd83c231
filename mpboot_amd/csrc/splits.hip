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
//   k_split_keys_lists  the same for a tree given as CSR neighbour lists, inner nodes of any degree >= 3 (a consensus tree, a user
//                    tree with polytomies): the lists go into LDS, the walk goes through the children in list order.  A tree with m
//                    inner nodes has m - 1 clusters; the rest of its n - 3 cluster slots are dead (key kSplitEmpty) and skipped by
//                    every later kernel, so that tree = cluster / (n - 3) holds for both forms.
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
// Robinson-Foulds distances between the trees of a call (MTreeSet::computeRFDist, mtreeset.cpp:484-660) on the same table.  Every
// tree has weight 1 there, so a slot's count is the number of trees that hold its split, and RF(i, j) = 2 (n - 3) - 2 shared(i, j):
//
//   k_rf_columns     one thread per slot: a used slot with count >= 2 gets a dense column number (a split of one tree is shared
//                    by no pair and gets none, which bounds the columns by half the clusters).
//   k_rf_rows        the trees x columns incidence matrix B of a chunk of columns [c0, c1) as bits: one thread per cluster,
//                    atomicOr of its column's bit into its tree's row.  Rows are padded with zero words to kRfKStep words and the
//                    row count with zero rows to kRfTile, so that the product has no edge branches on its loads.
//   k_rf_patch       the same for the (cluster, column) pairs the host made of the overflow list (true key collisions).
//   k_rf_shared      shared[i][j] (+)= popcount(B[i][k] & B'[j][k]) over the chunk's words: a tiled integer matrix product on
//                    v_and_b32 + v_bcnt_u32_b32.  64 x 64 outputs per 256-thread workgroup, 4 x 4 per lane, 32-word K slices of both
//                    operands in LDS (8 KiB each, stored word-major: [k][64 rows], so that a lane's four rows of one word are one
//                    ds_read_b128 -- the A read is a broadcast of 4 addresses per wave, the B' read touches 16 distinct 16-byte
//                    slots per 16-lane group: all 64 banks once), the next slice's global loads issued before the current slice's
//                    arithmetic.  All pairs: only tiles on or above the diagonal, each writes its mirror image.  The first chunk
//                    stores, later chunks add; no atomics on the result.
//   k_rf_pairs       adjacent pairs (i, i + 1) only: one wave per pair strides over the two rows.
//   k_rf_finish      shared -> 2 (n - 3) - 2 shared, the diagonal of an all-pairs matrix 0; with list trees in the call
//                    c_i + c_j - 2 shared from the per-tree split counts (the reference's size(A) + size(B) - 2 common).
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

// grid: n_lists; any block size.  LDS: split_keys_lists_lds_bytes(n).  The counterpart of k_split_keys for a tree given as neighbour
// lists.  A fully resolved tree gets the same clusters as its record form AS SETS AND KEYS only: the children are taken in list
// order here and in ring order behind the entering record there, so pos[], order[], the intervals and the cluster numbers differ.  A stack entry is dad << 16 | node (node numbers are below 2 n <= 4094), a negative one closes cluster -(x + 1).  The host
// has checked the lists; all the same every number read from them is checked before it indexes anything, and the walk is bounded by
// the node counts of a tree: a malformed list ends it with bad[t] = 1
__global__ void __launch_bounds__(256) k_split_keys_lists(const SplitListDesc *__restrict__ desc, const int32_t *__restrict__ data, int n, int key_bits,
                                                          int32_t *__restrict__ pos, int32_t *__restrict__ order, SplitCluster *__restrict__ cl,
                                                          int32_t *__restrict__ bad)
{
  extern __shared__ int32_t lds[];
  const SplitListDesc d = desc[blockIdx.x];
  const int C = n - 3, m = d.n_inner, E = d.n_nbr, N = n + m;
  const size_t t = (size_t)d.tree;
  SplitCluster *my_cl = cl + t * (size_t)C;
  // (the launcher's host has sized the staging by these numbers; out of range: nothing is read)
  const bool sizes_ok = m >= 1 && m <= n - 2 && E >= 0 && E <= 3 * (n - 2);
  // the slots no cluster of this tree will fill
  for (int i = (sizes_ok ? m - 1 : 0) + (int)threadIdx.x; i < C; i += blockDim.x) my_cl[i] = SplitCluster{0u, 0u, kSplitEmpty};
  if (!sizes_ok) { if (threadIdx.x == 0) bad[t] = 1; return; }
  int32_t *fi = lds, *nb = lds + (m + 1), *stk = nb + E;
  const int cap = (int)split_lists_stack_words(n, m);
  for (int i = threadIdx.x; i <= m; i += blockDim.x) fi[i] = data[(size_t)d.first_at + i];
  for (int i = threadIdx.x; i < E; i += blockDim.x) nb[i] = data[(size_t)d.nbr_at + i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  int32_t *my_pos = pos + t * (size_t)n, *my_order = order + t * (size_t)(n - 1);
  const unsigned long long mask = key_bits >= 64 ? ~0ull : ((1ull << key_bits) - 1ull);
  int sp = 0, cnt = 0, inner = 0, err = 0;
  unsigned long long acc = 0;
  {
    // the walk starts at the inner node next to tip 1, which must list tip 1
    const int r = d.root;
    bool has1 = false;
    if (r > n && r <= N) {
      const int f0 = fi[r - n - 1], f1 = fi[r - n];
      if (f0 >= 0 && f1 >= f0 && f1 <= E)
        for (int k = f0; k < f1; k++) has1 = has1 || nb[k] == 1;
    }
    if (has1) stk[sp++] = (1 << 16) | r;
    else err = 1;
  }
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
    const int v = x & 0xFFFF, dad = x >> 16;
    if (v < 1 || v > N) { err = 1; break; }
    if (v <= n) {
      if (v == 1 || cnt >= n - 1) { err = 1; break; }
      my_pos[v - 1] = cnt;
      my_order[cnt++] = v;
      acc += splitmix64(kTaxonSalt ^ (unsigned long long)v);
      continue;
    }
    if (inner >= m) { err = 1; break; }
    const int f0 = fi[v - n - 1], f1 = fi[v - n];
    if (f0 < 0 || f1 < f0 || f1 > E || sp + (f1 - f0) + 1 > cap) { err = 1; break; }
    const int ci = inner++ - 1;                    // the node next to tip 1 holds every other tip: no split
    if (ci >= 0) {
      my_cl[ci].lo = (uint32_t)cnt;
      my_cl[ci].key = acc;                         // (parked here until the cluster closes)
      stk[sp++] = -(ci + 1);
    }
    for (int k = f1 - 1; k >= f0; k--) {           // children in list order: the first one on top
      const int u = nb[k];
      if (u == dad) continue;
      if (u < 1 || u > N) { err = 1; break; }
      stk[sp++] = (v << 16) | u;
    }
    if (err) break;
  }
  my_pos[0] = n - 1;                               // tip 1: outside every interval
  err = err || cnt != n - 1 || inner != m;
  // a walk that ended early may have left a cluster open (a parked sum as its key): no slot of a bad tree is looked at, but mark
  // them all the same so that nothing depends on it
  if (err)
    for (int i = 0; i < C; i++) my_cl[i] = SplitCluster{0u, 0u, kSplitEmpty};
  bad[t] = err ? 1 : 0;
}

__device__ __forceinline__ uint32_t slot_hash(unsigned long long k) { return (uint32_t)(splitmix64(k) >> 17); }

// one thread per cluster
__global__ void __launch_bounds__(256) k_split_insert(const SplitCluster *__restrict__ cl, uint32_t n_clusters, unsigned long long *tkey,
                                                      unsigned long long *trep, uint32_t tsize, uint32_t *__restrict__ slot_of)
{
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_clusters) return;
  const unsigned long long k = cl[g].key;
  if (k == kSplitEmpty) { slot_of[g] = kSplitNoSlot; return; }      // a dead slot of a list tree: no cluster
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
  bool live = g < n_clusters;
  uint32_t lo = 0, hi = 0, tg = 0, tr = 0, rlo = 0, rhi = 0, h = kSplitNoSlot;
  bool eq = false, need = false;
  if (live) {
    h = slot_of[g];
    const SplitCluster c = cl[g];
    lo = c.lo;
    hi = c.hi;
    live = c.key != kSplitEmpty;                   // a dead slot of a list tree: counted nowhere, never on the overflow list
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

// ---- Robinson-Foulds distances

// one thread per slot.  counters[2]: number of columns
__global__ void __launch_bounds__(256) k_rf_columns(const unsigned long long *__restrict__ trep, const unsigned long long *__restrict__ tcount,
                                                    uint32_t tsize, uint32_t *__restrict__ col_of_slot, uint32_t *counters)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= tsize) return;
  uint32_t c = kRfNoColumn;
  if (trep[s] != kSplitEmpty && tcount[s] >= 2ull) c = atomicAdd(&counters[2], 1u);
  col_of_slot[s] = c;
}

// row of tree t in B: the second set starts on a tile edge of its own
__device__ __forceinline__ uint32_t rf_row(uint32_t t, uint32_t n1, uint32_t row2) { return t < n1 ? t : row2 + (t - n1); }

// one thread per cluster; B (rows x row_words, zeroed before) gets the bits of the columns in [c0, c1)
__global__ void __launch_bounds__(256) k_rf_rows(const uint32_t *__restrict__ slot_of, uint32_t n_clusters, uint32_t C,
                                                 const uint32_t *__restrict__ col_of_slot, uint32_t c0, uint32_t c1, uint32_t n1, uint32_t row2,
                                                 uint32_t row_words, uint32_t *B)
{
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_clusters) return;
  const uint32_t h = slot_of[g];
  if (h == kSplitNoSlot) return;
  const uint32_t c = col_of_slot[h];
  if (c == kRfNoColumn || c < c0 || c >= c1) return;
  const uint32_t b = c - c0;
  atomicOr(&B[(size_t)rf_row(g / C, n1, row2) * row_words + (b >> 5)], 1u << (b & 31));
}

// one thread per (cluster, column) pair of the overflow groups
__global__ void __launch_bounds__(256) k_rf_patch(const uint32_t *__restrict__ patch, uint32_t m, uint32_t C, uint32_t c0, uint32_t c1,
                                                  uint32_t n1, uint32_t row2, uint32_t row_words, uint32_t *B)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t g = patch[2 * i], c = patch[2 * i + 1];
  if (c < c0 || c >= c1) return;
  const uint32_t b = c - c0;
  atomicOr(&B[(size_t)rf_row(g / C, n1, row2) * row_words + (b >> 5)], 1u << (b & 31));
}

// grid: the tiles (all pairs: nt (nt + 1) / 2 of them, on or above the diagonal; two sets: nt_a * nt_b).  block: 256.
// A = B + a_row0 * row_words, B' = B + b_row0 * row_words; both have whole tiles of rows and row_words % kRfKStep == 0.
// out[i * ld + j], i < na, j < nb.  accumulate = 0: store, 1: add to what is there
__global__ void __launch_bounds__(256) k_rf_shared(const uint32_t *__restrict__ B, uint32_t a_row0, uint32_t b_row0, uint32_t row_words,
                                                   uint32_t nt_b, int symmetric, uint32_t na, uint32_t nb, uint32_t ld, int accumulate,
                                                   int32_t *out)
{
  __shared__ __attribute__((aligned(16))) uint32_t sa[kRfKStep * kRfTile];
  __shared__ __attribute__((aligned(16))) uint32_t sb[kRfKStep * kRfTile];
  uint32_t ti, tj;
  if (symmetric) {
    // tile number -> (ti, tj), ti <= tj, rows of the upper triangle one after the other: row r starts at r nt - r (r - 1) / 2
    const uint32_t t = blockIdx.x, nt = nt_b;
    uint32_t r = (uint32_t)(((double)(2 * nt + 1) - sqrt((double)(2 * nt + 1) * (double)(2 * nt + 1) - 8.0 * (double)t)) * 0.5);
    if (r >= nt) r = nt - 1;
    while (r > 0 && (unsigned long long)r * nt - (unsigned long long)r * (r - 1) / 2 > t) r--;
    while (r + 1 < nt && (unsigned long long)(r + 1) * nt - (unsigned long long)(r + 1) * r / 2 <= t) r++;
    ti = r;
    tj = r + (t - (uint32_t)((unsigned long long)r * nt - (unsigned long long)r * (r - 1) / 2));
  } else {
    ti = blockIdx.x / nt_b;
    tj = blockIdx.x - ti * nt_b;
  }
  const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  // staging: thread -> row tid / 4 of the tile, words 8 (tid % 4) .. + 8 of the slice (two 16-byte loads per operand)
  const uint32_t lr = tid >> 2, lq = (tid & 3) * 8;
  const uint32_t *ga = B + ((size_t)a_row0 + (size_t)ti * kRfTile + lr) * row_words + lq;
  const uint32_t *gb = B + ((size_t)b_row0 + (size_t)tj * kRfTile + lr) * row_words + lq;
  uint4 ra0 = *reinterpret_cast<const uint4 *>(ga), ra1 = *reinterpret_cast<const uint4 *>(ga + 4);
  uint4 rb0 = *reinterpret_cast<const uint4 *>(gb), rb1 = *reinterpret_cast<const uint4 *>(gb + 4);
  uint32_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0;
  for (uint32_t k0 = 0; k0 < row_words; k0 += kRfKStep) {
    __syncthreads();                               // the last slice has been read by everybody
    {
      const uint32_t wa[8] = {ra0.x, ra0.y, ra0.z, ra0.w, ra1.x, ra1.y, ra1.z, ra1.w};
      const uint32_t wb[8] = {rb0.x, rb0.y, rb0.z, rb0.w, rb1.x, rb1.y, rb1.z, rb1.w};
#pragma unroll
      for (int q = 0; q < 8; q++) {
        sa[(lq + q) * kRfTile + lr] = wa[q];
        sb[(lq + q) * kRfTile + lr] = wb[q];
      }
    }
    __syncthreads();
    if (k0 + kRfKStep < row_words) {               // the next slice is on its way while this one is multiplied
      ga += kRfKStep;
      gb += kRfKStep;
      ra0 = *reinterpret_cast<const uint4 *>(ga);
      ra1 = *reinterpret_cast<const uint4 *>(ga + 4);
      rb0 = *reinterpret_cast<const uint4 *>(gb);
      rb1 = *reinterpret_cast<const uint4 *>(gb + 4);
    }
#pragma unroll 8
    for (int k = 0; k < kRfKStep; k++) {
      const uint4 a = *reinterpret_cast<const uint4 *>(&sa[k * kRfTile + 4 * ty]);
      const uint4 b = *reinterpret_cast<const uint4 *>(&sb[k * kRfTile + 4 * tx]);
      const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += (uint32_t)__popc(av[i] & bv[j]);
    }
  }
  const uint32_t i0 = ti * kRfTile + 4 * ty, j0 = tj * kRfTile + 4 * tx;
  const bool mirror = symmetric && ti != tj;       // (the diagonal tile holds both halves itself)
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t gi = i0 + i, gj = j0 + j;
      if (gi >= na || gj >= nb) continue;
      int32_t *o = out + (size_t)gi * ld + gj;
      const int32_t v = (int32_t)acc[i][j] + (accumulate ? *o : 0);
      *o = v;
      if (mirror) out[(size_t)gj * ld + gi] = v;
    }
}

// adjacent pairs: one wave per pair (i, i + 1) of the first n_pairs + 1 rows.  block: 256 = 4 pairs
__global__ void __launch_bounds__(256) k_rf_pairs(const uint32_t *__restrict__ B, uint32_t row_words, uint32_t n_pairs, int accumulate, int32_t *out)
{
  const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n_pairs) return;
  const uint32_t *x = B + (size_t)p * row_words, *y = x + row_words;
  uint32_t s = 0;
  for (uint32_t k = lane; k < row_words; k += 64) s += (uint32_t)__popc(x[k] & y[k]);
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) out[p] = (int32_t)s + (accumulate ? out[p] : 0);
}

// one thread per entry: shared -> 2 C - 2 shared; diag > 0: entries i * diag + i (the diagonal of an all-pairs matrix) are 0.
// COUNTS: trees of the call have fewer than C splits (list trees): c_a + c_b - 2 shared, a and b from the result's layout
template <bool COUNTS>
__global__ void __launch_bounds__(256) k_rf_finish(int32_t *out, unsigned long long entries, int32_t C, uint32_t diag,
                                                   const int32_t *__restrict__ n_splits, uint32_t n1, uint32_t n2)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= entries) return;
  const bool on_diag = diag && (i / diag) == (i % diag);
  int32_t both = 2 * C;
  if (COUNTS) {
    uint32_t a, b;
    if (diag) { a = (uint32_t)(i / diag); b = (uint32_t)(i % diag); }
    else if (n2) { a = (uint32_t)(i / n2); b = n1 + (uint32_t)(i % n2); }
    else { a = (uint32_t)i; b = a + 1; }
    both = n_splits[a] + n_splits[b];
  }
  out[i] = on_diag ? 0 : both - 2 * out[i];
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

hipError_t launch_split_keys_lists(hipStream_t st, const SplitListDesc *desc, int n_lists, const int32_t *data, int n, int key_bits, int32_t *pos,
                                   int32_t *order, SplitCluster *cl, int32_t *bad)
{
  if (n < 4 || n > kSplitMaxTaxa || n_lists < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_split_keys_lists, dim3((unsigned)n_lists), dim3(256), split_keys_lists_lds_bytes(n), st, desc, data, n, key_bits, pos, order,
                     cl, bad);
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

hipError_t launch_rf_columns(hipStream_t st, const unsigned long long *trep, const unsigned long long *tcount, uint32_t tsize, uint32_t *col_of_slot,
                             uint32_t *counters)
{
  hipLaunchKernelGGL(k_rf_columns, dim3(blocks_for(tsize)), dim3(256), 0, st, trep, tcount, tsize, col_of_slot, counters);
  return hipGetLastError();
}

hipError_t launch_rf_rows(hipStream_t st, const uint32_t *slot_of, uint32_t n_clusters, int n, const uint32_t *col_of_slot, uint32_t c0, uint32_t c1,
                          uint32_t n1, uint32_t row2, uint32_t row_words, uint32_t *B)
{
  if (n < 4 || !n_clusters || c1 < c0 || (uint64_t)(c1 - c0) > 32ull * row_words) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rf_rows, dim3(blocks_for(n_clusters)), dim3(256), 0, st, slot_of, n_clusters, (uint32_t)(n - 3), col_of_slot, c0, c1, n1, row2,
                     row_words, B);
  return hipGetLastError();
}

hipError_t launch_rf_patch(hipStream_t st, const uint32_t *patch, uint32_t m, int n, uint32_t c0, uint32_t c1, uint32_t n1, uint32_t row2,
                           uint32_t row_words, uint32_t *B)
{
  if (!m) return hipSuccess;
  if (n < 4 || c1 < c0 || (uint64_t)(c1 - c0) > 32ull * row_words) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rf_patch, dim3(blocks_for(m)), dim3(256), 0, st, patch, m, (uint32_t)(n - 3), c0, c1, n1, row2, row_words, B);
  return hipGetLastError();
}

hipError_t launch_rf_shared(hipStream_t st, const uint32_t *B, uint32_t a_row0, uint32_t b_row0, uint32_t row_words, bool symmetric, uint32_t na,
                            uint32_t nb, bool accumulate, int32_t *out)
{
  if (!na || !nb || !row_words || row_words % kRfKStep || a_row0 % kRfTile || b_row0 % kRfTile || (symmetric && (na != nb || a_row0 != b_row0)))
    return hipErrorInvalidValue;
  const unsigned long long nt_a = rf_tiles(na), nt_b = rf_tiles(nb);
  const unsigned long long tiles = symmetric ? nt_a * (nt_a + 1) / 2 : nt_a * nt_b;
  if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rf_shared, dim3((unsigned)tiles), dim3(256), 0, st, B, a_row0, b_row0, row_words, (uint32_t)nt_b, symmetric ? 1 : 0, na, nb,
                     nb, accumulate ? 1 : 0, out);
  return hipGetLastError();
}

hipError_t launch_rf_pairs(hipStream_t st, const uint32_t *B, uint32_t row_words, uint32_t n_pairs, bool accumulate, int32_t *out)
{
  if (!n_pairs) return hipSuccess;
  hipLaunchKernelGGL(k_rf_pairs, dim3((n_pairs + 3) / 4), dim3(256), 0, st, B, row_words, n_pairs, accumulate ? 1 : 0, out);
  return hipGetLastError();
}

hipError_t launch_rf_finish(hipStream_t st, int32_t *out, unsigned long long entries, int n, uint32_t diag, const int32_t *n_splits, uint32_t n1,
                            uint32_t n2)
{
  if (!entries) return hipSuccess;
  if (entries > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (n_splits) hipLaunchKernelGGL(k_rf_finish<true>, dim3(blocks_for(entries)), dim3(256), 0, st, out, entries, (int32_t)(n - 3), diag, n_splits, n1, n2);
  else hipLaunchKernelGGL(k_rf_finish<false>, dim3(blocks_for(entries)), dim3(256), 0, st, out, entries, (int32_t)(n - 3), diag, n_splits, n1, n2);
  return hipGetLastError();
}

}  // namespace mpf
