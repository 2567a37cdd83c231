// ufb_probe.cpp -- a test-only way into the launchers of ufboot.hpp (libmpfprobe.so = ufboot.o + this file).
//
// Every mpf_probe_* function takes HOST pointers and sizes, allocates device memory, copies, calls the launcher(s) on a stream of
// its own, synchronises, copies back and returns the hipError_t as an int.  Nothing here is part of the product's interface
// (include/mpfitch.h) or of libmpfitch.so; tests/ufb_probe.py is the ctypes face.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ufboot.hpp"

using namespace mpf;

namespace {

#define PCHK(x)                                \
  do {                                         \
    const hipError_t e_ = (x);                 \
    if (e_ != hipSuccess) return (int)e_;      \
  } while (0)

// device (or pinned host) memory that goes away with the call
template <class T> struct Buf {
  T *p = nullptr;
  size_t n = 0;
  bool pinned = false;
  ~Buf()
  {
    if (!p) return;
    if (pinned) (void)hipHostFree(p);
    else (void)hipFree(p);
  }
  // n elements (at least one, so that no kernel is handed a null pointer for an empty range), filled from src where given
  hipError_t dev(size_t count, const T *src = nullptr, size_t n_src = 0)
  {
    n = std::max<size_t>(count, 1);
    hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) e = hipMemset(p, 0, n * sizeof(T));
    if (e == hipSuccess && src && n_src) e = hipMemcpy(p, src, std::min(n_src, count) * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
  hipError_t pin(size_t count)
  {
    n = std::max<size_t>(count, 1);
    pinned = true;
    hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) std::fill(p, p + n, T{});
    return e;
  }
  hipError_t back(T *dst, size_t count) const { return count ? hipMemcpy(dst, p, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
};

struct Stream {
  hipStream_t s = nullptr;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t make() { return hipStreamCreate(&s); }
};

void ran_out(const BitgemmRan &r, int32_t *out)
{
  if (!out) return;
  out[0] = r.tm; out[1] = r.tn; out[2] = r.ksplit; out[3] = r.kb_per_split; out[4] = r.grid_x; out[5] = r.atomic; out[6] = r.m32;
}

// the shapes launch_bitgemm can serve without reading or writing out of bounds: whole column tiles, whole k stages, and a row
// count padded as the callers pad it
bool product_shape_ok(int rows, int rows_padded, int chained, int Wp, int Bp)
{
  if (rows <= 0 || rows_padded < rows || Wp < 8 || Wp % 8 != 0 || Bp <= 0 || Bp % kUfbColTile != 0) return false;
  const int unit = chained ? ufb_row_padding(rows, Bp) : kUfbRowTile;
  return rows_padded == (rows + unit - 1) / unit * unit;
}

}  // namespace

extern "C" {

struct MpfProbeProduct {
  const uint32_t *masks;      // [mask_rows][Wp]
  int32_t mask_rows, rows, rows_padded, chained, Wp, Bp;
  const uint16_t *src;        // [n_cols][P] weights
  int32_t n_cols, P;
  const int32_t *first, *cur; // [P]
  int32_t planes;             // 7-bit weight planes (1..3)
  int32_t *C;                 // [rows_padded][Bp], in (accumulate) and out
  int32_t mult, accumulate;   // plane pl runs with mult << 7 pl; planes behind the first accumulate in any case
  const uint32_t *rowsel;     // optional, [rows_padded] rows of the mask matrix
  int32_t have_limit;
  uint32_t row_limit;
  int32_t *ran;               // optional, [planes][7]
};

struct MpfProbeEvents {
  int32_t route;              // 0 = launch_ufb_events, 1 = launch_ufb_events_publish
  const uint32_t *info;       // [n_idx][2]
  const uint32_t *cost;       // [n_idx]
  const uint32_t *thr, *home; // [n_parts]
  const uint32_t *crow;       // optional, [n_idx]
  const int32_t *C;           // [c_rows][Bp]
  const int32_t *rt;          // [Bp]
  const uint32_t *best;       // [Bp]
  uint32_t n_idx, n_parts, c_rows;
  int32_t Bp, B, fixed_bound, clamp_rt, have_cut;
  uint32_t cut;
  uint32_t *ev;               // out, [ev_cap][3]
  uint32_t ev_cap;
  uint32_t *ev_count;         // out
  // publication (route 1)
  const uint32_t *pub_src[3];
  uint32_t *pub_dst[3];       // out
  uint32_t pub_words[3];
  uint32_t *h_ev;             // out, [h_ev_cap][3]
  uint32_t h_ev_cap;
  uint32_t *h_flag;           // out, [4]
  uint32_t *done;             // out, the ticket word after the launch
};

struct MpfProbeMid {
  int32_t kind;               // 0 = launch_ufb_mid, 1 = launch_ufb_prep, 2 = launch_ufb_self
  int32_t *C;                 // in / out, [c_total] words
  uint32_t c_total, c_words;
  uint32_t *info;             // in / out, [n_idx][2]
  const uint32_t *self_idx;
  uint32_t n_self, code;
  uint32_t *ev_count;         // in / out
  const uint32_t *cost;       // [n_idx]
  const uint32_t *home, *plan_end;   // [n_parts]
  uint32_t n_idx, n_parts;
  uint32_t *cut;              // in / out
  const uint32_t *pub_src[3];
  uint32_t *pub_dst[3];
  uint32_t pub_words[3];
  uint32_t *h_flag;           // out, [4]
  uint32_t *done;             // out
};

int mpf_probe_row_tile(void) { return kUfbRowTile; }
int mpf_probe_row_padding(int rows, int Bp) { return ufb_row_padding(rows, Bp); }
int mpf_probe_events2_max(void) { return (int)kUfbEvents2Max; }
int mpf_probe_chunks(uint32_t n_idx) { return (int)ufb_chunks(n_idx); }

// launch_ufb_layout, then launch_bitgemm per weight plane (mult << 7 pl, accumulating behind the first)
int mpf_probe_product(const MpfProbeProduct *a)
{
  if (!product_shape_ok(a->rows, a->rows_padded, a->chained, a->Wp, a->Bp)) return (int)hipErrorInvalidValue;
  if (a->planes < 1 || a->planes > 3 || a->n_cols > a->Bp || a->P > 32 * a->Wp) return (int)hipErrorInvalidValue;
  for (int p = 0; p < a->P; p++)
    if (a->first[p] >= 32 * a->Wp) return (int)hipErrorInvalidValue;
  const size_t Wp = (size_t)a->Wp, Bp = (size_t)a->Bp;
  // without rowsel the mask matrix is the padded one: the rows behind the caller's hold arbitrary non-zero words
  const size_t mrows = a->rowsel ? (size_t)a->mask_rows : (size_t)a->rows_padded;
  if (!a->rowsel && a->mask_rows > a->rows_padded) return (int)hipErrorInvalidValue;
  if (a->rowsel)
    for (int i = 0; i < a->rows_padded; i++)
      if (a->rowsel[i] >= (uint32_t)a->mask_rows) return (int)hipErrorInvalidValue;
  std::vector<uint32_t> hm(mrows * Wp);
  for (size_t i = 0; i < hm.size(); i++) hm[i] = (uint32_t)(i * 2654435761u) | 1u;
  std::copy(a->masks, a->masks + (size_t)a->mask_rows * Wp, hm.begin());
  Stream st;
  PCHK(st.make());
  Buf<uint32_t> masks, sel, lim;
  Buf<uint16_t> src;
  Buf<int32_t> first, cur, C;
  Buf<uint8_t> wt;
  const size_t plane_bytes = Wp * 32 * Bp;
  PCHK(masks.dev(hm.size(), hm.data(), hm.size()));
  PCHK(src.dev((size_t)a->n_cols * a->P, a->src, (size_t)a->n_cols * a->P));
  PCHK(first.dev(a->P, a->first, a->P));
  PCHK(cur.dev(a->P, a->cur, a->P));
  PCHK(C.dev((size_t)a->rows_padded * Bp, a->C, (size_t)a->rows_padded * Bp));
  PCHK(wt.dev(plane_bytes * a->planes));
  if (a->rowsel) PCHK(sel.dev(a->rows_padded, a->rowsel, a->rows_padded));
  PCHK(lim.dev(1, &a->row_limit, 1));
  PCHK(launch_ufb_layout(st.s, src.p, a->n_cols, a->P, first.p, cur.p, wt.p, a->Bp, a->planes, plane_bytes));
  for (int pl = 0; pl < a->planes; pl++) {
    BitgemmRan ran;
    PCHK(launch_bitgemm(st.s, masks.p, a->rows_padded, a->Wp, wt.p + (size_t)pl * plane_bytes, a->Bp, C.p, a->mult << (7 * pl),
                        (a->accumulate || pl > 0) ? 1 : 0, a->rowsel ? sel.p : nullptr, a->have_limit ? lim.p : nullptr, &ran));
    ran_out(ran, a->ran ? a->ran + 7 * pl : nullptr);
  }
  PCHK(hipStreamSynchronize(st.s));
  return (int)C.back(a->C, (size_t)a->rows_padded * Bp);
}

// launch_vals_planes into the caller's planes[K][rows_p][Wp] (in / out); with n_cols > 0 also the weighted tracker's chain:
// launch_ufb_layout (pattern p at site p), then one product per (bit k, weight plane pl) with mult (1 << k) << 7 pl into C
int mpf_probe_vals(const uint16_t *vals, uint32_t rows, uint32_t npat, int K, uint32_t *planes, uint32_t rows_p, uint32_t Wp,
                   const uint16_t *src, int n_cols, int wplanes, int Bp, int32_t *C, int32_t *ran)
{
  if (!rows || !npat || K < 1 || K > 16 || rows_p < rows || Wp < 2 * ((npat + 63) / 64)) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  Buf<uint16_t> dv, dsrc;
  Buf<uint32_t> dp;
  const size_t plane_words = (size_t)rows_p * Wp;
  PCHK(dv.dev((size_t)rows * npat, vals, (size_t)rows * npat));
  PCHK(dp.dev((size_t)K * plane_words, planes, (size_t)K * plane_words));
  PCHK(launch_vals_planes(st.s, dv.p, rows, npat, K, dp.p, rows_p, Wp));
  PCHK(hipStreamSynchronize(st.s));
  PCHK(dp.back(planes, (size_t)K * plane_words));
  if (n_cols <= 0) return 0;
  if (!product_shape_ok((int)rows, (int)rows_p, 0, (int)Wp, Bp) || wplanes < 1 || wplanes > 3 || n_cols > Bp) return (int)hipErrorInvalidValue;
  std::vector<int32_t> h_first(npat), h_cur(npat, 1);
  for (uint32_t p = 0; p < npat; p++) h_first[p] = (int32_t)p;
  Buf<int32_t> first, cur, dC;
  Buf<uint8_t> wt;
  const size_t plane_bytes = (size_t)Wp * 32 * (size_t)Bp;
  PCHK(dsrc.dev((size_t)n_cols * npat, src, (size_t)n_cols * npat));
  PCHK(first.dev(npat, h_first.data(), npat));
  PCHK(cur.dev(npat, h_cur.data(), npat));
  PCHK(dC.dev((size_t)rows_p * Bp, C, (size_t)rows_p * Bp));          // (the caller's noise: the first product overwrites it)
  PCHK(wt.dev(plane_bytes * wplanes));
  PCHK(launch_ufb_layout(st.s, dsrc.p, n_cols, (int)npat, first.p, cur.p, wt.p, Bp, wplanes, plane_bytes));
  bool is_first = true;
  for (int k = 0; k < K; k++)
    for (int pl = 0; pl < wplanes; pl++) {
      BitgemmRan r;
      PCHK(launch_bitgemm(st.s, dp.p + (size_t)k * plane_words, (int)rows_p, (int)Wp, wt.p + (size_t)pl * plane_bytes, Bp, dC.p,
                          (1 << k) << (7 * pl), is_first ? 0 : 1, nullptr, nullptr, &r));
      if (is_first) ran_out(r, ran);
      is_first = false;
    }
  PCHK(hipStreamSynchronize(st.s));
  return (int)dC.back(C, (size_t)rows_p * Bp);
}

// vec: [n_vec][S][Wp] words; ops: [n_ops][4] (a, b, out, pad); masks out: [n_ops][Wp]
int mpf_probe_join_masks(const uint32_t *vec, uint32_t n_vec, const uint32_t *ops, int n_ops, int S, int Wp, uint32_t *masks)
{
  for (int i = 0; i < n_ops; i++)
    if (ops[4 * i] >= n_vec || ops[4 * i + 1] >= n_vec) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  Buf<uint32_t> dv, dm;
  Buf<EvOp> dops;
  const size_t nv = (size_t)n_vec * S * Wp;
  PCHK(dv.dev(nv, vec, nv));
  PCHK(dops.dev(n_ops, reinterpret_cast<const EvOp *>(ops), n_ops));
  PCHK(dm.dev((size_t)n_ops * Wp, masks, (size_t)n_ops * Wp));
  Geometry g{};
  g.S = S;
  g.Wp = Wp;
  PCHK(launch_join_masks(st.s, g, dv.p, dops.p, n_ops, dm.p));
  PCHK(hipStreamSynchronize(st.s));
  return (int)dm.back(masks, (size_t)n_ops * Wp);
}

// rt[Bp] (in: noise, the launcher zeroes it) = column sums of C[rows][Bp]
int mpf_probe_colsum(const int32_t *C, int rows, int Bp, int32_t *rt)
{
  if (rows <= 0 || Bp <= 0) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  Buf<int32_t> dC, drt;
  PCHK(dC.dev((size_t)rows * Bp, C, (size_t)rows * Bp));
  PCHK(drt.dev(Bp, rt, Bp));
  PCHK(launch_colsum(st.s, dC.p, rows, Bp, drt.p));
  PCHK(hipStreamSynchronize(st.s));
  return (int)drt.back(rt, Bp);
}

int mpf_probe_rt_update(int32_t *rt, const int32_t *C, uint32_t c_rows, int Bp, uint32_t row, uint32_t home)
{
  if (row >= c_rows || home >= c_rows || Bp <= 0) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  Buf<int32_t> dC, drt;
  PCHK(dC.dev((size_t)c_rows * Bp, C, (size_t)c_rows * Bp));
  PCHK(drt.dev(Bp, rt, Bp));
  PCHK(launch_rt_update(st.s, drt.p, dC.p, Bp, row, home));
  PCHK(hipStreamSynchronize(st.s));
  return (int)drt.back(rt, Bp);
}

// out[out_n] (in / out; out_n >= rows) <- column col of C[rows][Bp]
int mpf_probe_column(const int32_t *C, uint32_t rows, int Bp, int col, int32_t *out, uint32_t out_n)
{
  if (col < 0 || col >= Bp || out_n < rows) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  Buf<int32_t> dC, dout;
  PCHK(dC.dev((size_t)rows * Bp, C, (size_t)rows * Bp));
  PCHK(dout.dev(out_n, out, out_n));
  PCHK(launch_ufb_column(st.s, dC.p, Bp, col, rows, dout.p));
  PCHK(hipStreamSynchronize(st.s));
  return (int)dout.back(out, out_n);
}

int mpf_probe_events(const MpfProbeEvents *a)
{
  const uint32_t n = a->n_idx;
  if (a->Bp <= 0 || a->B <= 0 || a->B > a->Bp || !a->c_rows || !a->n_parts) return (int)hipErrorInvalidValue;
  if (a->h_ev_cap > a->ev_cap) return (int)hipErrorInvalidValue;       // (k_ufb_publish copies the host's events out of the device's)
  // every index the kernels can form stays inside its array
  for (uint32_t p = 0; p < a->n_parts; p++)
    if (a->home[p] >= std::max(n, 1u)) return (int)hipErrorInvalidValue;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t part = a->info[2 * i + 1];
    if (part < 0xFFFFFFFEu && part >= a->n_parts) return (int)hipErrorInvalidValue;
    if ((a->crow ? a->crow[i] : (part < 0xFFFFFFFEu ? a->info[2 * i] : 0u)) >= a->c_rows) return (int)hipErrorInvalidValue;
  }
  if (!a->crow)
    for (uint32_t p = 0; p < a->n_parts; p++)
      if (a->home[p] >= a->c_rows) return (int)hipErrorInvalidValue;
  Stream st;
  PCHK(st.make());
  const size_t Bp = (size_t)a->Bp, nc = std::max(ufb_chunks(n), 1u);
  Buf<uint32_t> info, cost, thr, home, crow, best, cmin, pre, ev, evc, cut, done, srcs[3];
  Buf<int32_t> C, rt;
  Buf<uint32_t> h_dst[3], h_ev, h_flag;
  PCHK(info.dev(2 * (size_t)n, a->info, 2 * (size_t)n));
  PCHK(cost.dev(n, a->cost, n));
  PCHK(thr.dev(a->n_parts, a->thr, a->n_parts));
  PCHK(home.dev(a->n_parts, a->home, a->n_parts));
  if (a->crow) PCHK(crow.dev(n, a->crow, n));
  PCHK(C.dev((size_t)a->c_rows * Bp, a->C, (size_t)a->c_rows * Bp));
  PCHK(rt.dev(Bp, a->rt, Bp));
  PCHK(best.dev(Bp, a->best, Bp));
  PCHK(cmin.dev(nc * Bp));
  PCHK(pre.dev(nc * Bp));
  PCHK(ev.dev(3 * (size_t)a->ev_cap));
  PCHK(evc.dev(1));
  PCHK(cut.dev(1, &a->cut, 1));
  PCHK(done.dev(1));
  const uint2 *d_info = reinterpret_cast<const uint2 *>(info.p);
  UfbEvent *d_ev = reinterpret_cast<UfbEvent *>(ev.p);
  if (a->route == 0) {
    PCHK(launch_ufb_events(st.s, d_info, cost.p, thr.p, home.p, a->crow ? crow.p : nullptr, C.p, a->Bp, a->B, rt.p, best.p, n, cmin.p, pre.p, d_ev,
                           a->ev_cap, evc.p, a->fixed_bound));
    PCHK(hipStreamSynchronize(st.s));
  } else {
    UfbPublishArgs pa;
    for (int k = 0; k < 3; k++) {
      PCHK(srcs[k].dev(a->pub_words[k], a->pub_src[k], a->pub_words[k]));
      PCHK(h_dst[k].pin(a->pub_words[k]));
      pa.src[k] = srcs[k].p;
      pa.dst[k] = h_dst[k].p;
      pa.words[k] = a->pub_words[k];
    }
    PCHK(h_ev.pin(3 * (size_t)a->h_ev_cap));
    PCHK(h_flag.pin(4));
    pa.h_ev = reinterpret_cast<UfbEvent *>(h_ev.p);
    pa.h_ev_cap = a->h_ev_cap;
    pa.h_flag = h_flag.p;
    pa.done = done.p;
    PCHK(launch_ufb_events_publish(st.s, d_info, cost.p, thr.p, home.p, a->crow ? crow.p : nullptr, C.p, a->Bp, a->B, rt.p, best.p, n, cmin.p, pre.p,
                                   d_ev, a->ev_cap, evc.p, a->fixed_bound, pa, a->clamp_rt, a->have_cut ? cut.p : nullptr));
    PCHK(hipStreamSynchronize(st.s));
    for (int k = 0; k < 3; k++) std::copy(h_dst[k].p, h_dst[k].p + a->pub_words[k], a->pub_dst[k]);
    std::copy(h_ev.p, h_ev.p + 3 * (size_t)a->h_ev_cap, a->h_ev);
    std::copy(h_flag.p, h_flag.p + 4, a->h_flag);
    PCHK(done.back(a->done, 1));
  }
  PCHK(ev.back(a->ev, 3 * (size_t)a->ev_cap));
  return (int)evc.back(a->ev_count, 1);
}

int mpf_probe_mid(const MpfProbeMid *a)
{
  const uint32_t n = a->n_idx;
  if (a->c_words > a->c_total || a->c_words % 4 != 0) return (int)hipErrorInvalidValue;
  for (uint32_t i = 0; i < a->n_self; i++)
    if (a->self_idx[i] >= n) return (int)hipErrorInvalidValue;
  if (a->kind == 0) {
    for (uint32_t p = 0; p < a->n_parts; p++)
      if (a->home[p] >= n) return (int)hipErrorInvalidValue;
    for (uint32_t i = 0; i < n; i++)
      if (a->info[2 * i + 1] < 0xFFFFFFFEu && a->info[2 * i + 1] >= a->n_parts) return (int)hipErrorInvalidValue;
  }
  Stream st;
  PCHK(st.make());
  Buf<int32_t> C;
  Buf<uint32_t> info, idx, evc, cost, home, pend, cut, done, srcs[3], h_dst[3], h_flag;
  PCHK(C.dev(a->c_total, a->C, a->c_total));
  PCHK(info.dev(2 * (size_t)n, a->info, 2 * (size_t)n));
  PCHK(idx.dev(a->n_self, a->self_idx, a->n_self));
  PCHK(evc.dev(1, a->ev_count, 1));
  PCHK(cut.dev(1, a->cut, 1));
  PCHK(done.dev(1));
  PCHK(h_flag.pin(4));
  uint2 *d_info = reinterpret_cast<uint2 *>(info.p);
  if (a->kind == 0) {
    PCHK(cost.dev(n, a->cost, n));
    PCHK(home.dev(a->n_parts, a->home, a->n_parts));
    PCHK(pend.dev(a->n_parts, a->plan_end, a->n_parts));
    UfbPublishArgs pa;
    for (int k = 0; k < 3; k++) {
      PCHK(srcs[k].dev(a->pub_words[k], a->pub_src[k], a->pub_words[k]));
      PCHK(h_dst[k].pin(a->pub_words[k]));
      pa.src[k] = srcs[k].p;
      pa.dst[k] = h_dst[k].p;
      pa.words[k] = a->pub_words[k];
    }
    pa.h_flag = h_flag.p;
    pa.done = done.p;
    PCHK(launch_ufb_mid(st.s, C.p, a->c_words, d_info, idx.p, a->n_self, a->code, evc.p, pa, cost.p, home.p, pend.p, n, cut.p));
  } else if (a->kind == 1) {
    PCHK(launch_ufb_prep(st.s, C.p, a->c_words, d_info, idx.p, a->n_self, a->code, evc.p));
  } else {
    PCHK(launch_ufb_self(st.s, d_info, idx.p, a->n_self, a->code));
  }
  PCHK(hipStreamSynchronize(st.s));
  if (a->kind == 0)
    for (int k = 0; k < 3; k++) std::copy(h_dst[k].p, h_dst[k].p + a->pub_words[k], a->pub_dst[k]);
  std::copy(h_flag.p, h_flag.p + 4, a->h_flag);
  PCHK(done.back(a->done, 1));
  PCHK(C.back(a->C, a->c_total));
  PCHK(info.back(a->info, 2 * (size_t)n));
  PCHK(evc.back(a->ev_count, 1));
  return (int)cut.back(a->cut, 1);
}

}  // extern "C"
