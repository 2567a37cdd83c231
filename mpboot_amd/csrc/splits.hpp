// splits.hpp -- launchers of splits.hip: the bipartitions of a set of complete trees, counted exactly on the device, and the
// Robinson-Foulds distances between the trees on the same table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpf {

// a cluster of a tree: the tips whose DFS position lies in [lo, hi), and the wrapping sum of their per-taxon constants
struct SplitCluster { uint32_t lo, hi; unsigned long long key; };
// a used slot of the table: its representative cluster (the smallest cluster number that claimed it) and the summed weight of the
// clusters that ARE that set
struct SplitEntry { uint32_t rep, slot; unsigned long long count; };

constexpr unsigned long long kSplitEmpty = ~0ull;        // an unclaimed key / representative; as a cluster's key: a dead slot
constexpr uint32_t kSplitNoSlot = 0xFFFFFFFFu;           // slot_of[] of a cluster that went to the overflow list
// k_split_keys keeps a tree's records (3 (2n - 1) words) and its walk's stack (2n + 4 words) in LDS: 32 n + 4 bytes.  Within the
// 64 KiB a workgroup gets without asking for more that is n <= 2047
constexpr int kSplitMaxTaxa = 2047;
inline size_t split_keys_lds_bytes(int n) { return sizeof(int32_t) * ((size_t)3 * (2 * (size_t)n - 1) + 2 * (size_t)n + 4); }
// A tree given as neighbour lists (tips 1 .. n, inner node i = node n + 1 + i, neighbours nbr[first[i] .. first[i + 1])): tree
// `tree` of the call, its first[] (n_inner + 1 words) at data[first_at], its nbr[] (n_nbr words) at data[nbr_at]; root = the inner
// node next to tip 1.  It has n_inner - 1 clusters; every tree keeps n - 3 cluster slots, the unused ones are dead (key kSplitEmpty,
// which the walk never emits) and no later kernel looks at them
struct SplitListDesc { int32_t tree, n_inner, first_at, nbr_at, n_nbr, root; };
// k_split_keys_lists keeps the lists (at most (n - 1) + (3 n - 6) words) and its walk's stack (n + 2 n_inner + 2 <= 3 n - 2 words)
// in LDS: less than 28 n bytes, within split_keys_lds_bytes(n) for every n >= 4
constexpr size_t split_lists_stack_words(int n, int n_inner) { return (size_t)n + 2 * (size_t)n_inner + 2; }
inline size_t split_keys_lists_lds_bytes(int n) { return sizeof(int32_t) * (((size_t)n - 1) + 3 * ((size_t)n - 2) + split_lists_stack_words(n, n - 2)); }

// Robinson-Foulds distances: the incidence matrix B (trees x columns, bits) is multiplied in tiles of kRfTile x kRfTile outputs over
// slices of kRfKStep words; its rows are padded to both.  B is built and multiplied in chunks of columns so that rows x words of a
// chunk stay within kRfBudgetBytes, whatever the number of distinct splits
constexpr uint32_t kRfNoColumn = 0xFFFFFFFFu;            // col_of_slot[] of a slot whose split fewer than two trees hold
constexpr int kRfTile = 64, kRfKStep = 32;
constexpr size_t kRfBudgetBytes = (size_t)256 << 20;
inline unsigned long long rf_tiles(unsigned long long rows) { return (rows + kRfTile - 1) / kRfTile; }

hipError_t launch_split_keys(hipStream_t st, const int32_t *backs, int n_trees, int n, int key_bits, int32_t *pos, int32_t *order,
                             SplitCluster *cl, int32_t *bad);
// one workgroup per list tree: pos / order / cl / bad of tree desc[i].tree, laid out as launch_split_keys lays them out
hipError_t launch_split_keys_lists(hipStream_t st, const SplitListDesc *desc, int n_lists, const int32_t *data, int n, int key_bits, int32_t *pos,
                                   int32_t *order, SplitCluster *cl, int32_t *bad);
hipError_t launch_split_insert(hipStream_t st, const SplitCluster *cl, uint32_t n_clusters, unsigned long long *tkey, unsigned long long *trep,
                               uint32_t tsize, uint32_t *slot_of);
hipError_t launch_split_count(hipStream_t st, const SplitCluster *cl, uint32_t n_clusters, int n, const int32_t *pos, const int32_t *order,
                              const unsigned long long *trep, uint32_t *slot_of, const int32_t *weights, unsigned long long *tcount,
                              uint32_t *ovf, uint32_t *counters);
hipError_t launch_split_compact(hipStream_t st, const unsigned long long *trep, const unsigned long long *tcount, uint32_t tsize, SplitEntry *out,
                                uint32_t *counters);
hipError_t launch_split_gather(hipStream_t st, const uint32_t *slot_of, uint32_t first, uint32_t m, const unsigned long long *tcount, long long *out);
hipError_t launch_split_bits(hipStream_t st, const SplitCluster *cl, const uint32_t *ids, uint32_t m, int n, const int32_t *pos, uint32_t *bits);
hipError_t launch_rf_columns(hipStream_t st, const unsigned long long *trep, const unsigned long long *tcount, uint32_t tsize, uint32_t *col_of_slot,
                             uint32_t *counters /* [2]: number of columns */);
// tree t's row: t < n1 ? t : row2 + (t - n1) (the second set of a two-set call starts on a tile edge)
hipError_t launch_rf_rows(hipStream_t st, const uint32_t *slot_of, uint32_t n_clusters, int n, const uint32_t *col_of_slot, uint32_t c0, uint32_t c1,
                          uint32_t n1, uint32_t row2, uint32_t row_words, uint32_t *B);
hipError_t launch_rf_patch(hipStream_t st, const uint32_t *patch /* [m][2]: cluster, column */, uint32_t m, int n, uint32_t c0, uint32_t c1,
                           uint32_t n1, uint32_t row2, uint32_t row_words, uint32_t *B);
hipError_t launch_rf_shared(hipStream_t st, const uint32_t *B, uint32_t a_row0, uint32_t b_row0, uint32_t row_words, bool symmetric, uint32_t na,
                            uint32_t nb, bool accumulate, int32_t *out /* [na][nb] */);
hipError_t launch_rf_pairs(hipStream_t st, const uint32_t *B, uint32_t row_words, uint32_t n_pairs, bool accumulate, int32_t *out);
// n_splits == null: every tree has n - 3 splits.  Else n_splits[t] of tree t; the entry's two trees follow from the layout: diag > 0
// all pairs of diag trees; n2 > 0 two sets (tree i of the first against tree n1 + j); else adjacent pairs
hipError_t launch_rf_finish(hipStream_t st, int32_t *out, unsigned long long entries, int n, uint32_t diag, const int32_t *n_splits = nullptr,
                            uint32_t n1 = 0, uint32_t n2 = 0);

}  // namespace mpf
