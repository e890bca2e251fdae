// The running statistics of one logits row of the contrastive slab kernels (clip_fwd_kernel, ssl_fwd_kernel,
// clip_fwd_mfma_kernel): the streaming (max, sum-exp, expectation) update, the first-maximum argmax, the diagonal terms,
// their merges across lanes and waves, and the stats row they end in. NE expectation accumulators sum_j p_j v_j (CLIP: 1,
// v = the logit; SSL: 3, one per temperature bucket, v = the unscaled dot) and ND diagonal terms, the target logit last
// (SSL: the target's unscaled dot in front of it). A kernel keeps how it forms a score, which accumulator a column feeds
// and the assignment of dg[]. Two rules of every merge live here and nowhere else: a state that saw no column (m = -inf)
// weighs 0, never exp(-inf - -inf); of equal maxima the lower column index wins.
// ssl_fwd_kernel and clip_fwd_mfma_kernel still spell `update` out on plain locals in their column loops and build the
// state behind them: through this struct those two loops get other register counts (profiles/loss_exchange_refactor.txt).
#pragma once
#include "common.h"

template <int NE, int ND>
struct RowState {                                         // an aggregate: State{m, l, {ex}, best, {dg}, bi}
  static constexpr int REC = 4 + NE + ND;                 // floats of one record in LDS (store / finish)
  static constexpr int STATS = (2 + NE + ND + 3) & ~3;    // floats of one stats row
  float m = -INFINITY, l = 0.f, ex[NE] = {}, best = -INFINITY, dg[ND] = {};
  int bi = 0x7fffffff;

  // column j with score z; p_j * v joins expectation `slot`. A lane's columns ascend, so `>` keeps the first maximum.
  __device__ __forceinline__ void update(int j, float z, float v, int slot) {
    if (z > best) { best = z; bi = j; }
    const float mn = fmaxf(m, z);
    const float al = __expf(m - mn), p = __expf(z - mn);
    l = l * al + p;
    for (int k = 0; k < NE; ++k) ex[k] = ex[k] * al + (slot == k ? p * v : 0.f);
    m = mn;
  }

  // merge of two states of the same row
  __device__ __forceinline__ void merge(const RowState& o) {
    const float mn = fmaxf(m, o.m);
    const float s1 = m == -INFINITY ? 0.f : __expf(m - mn), s2 = o.m == -INFINITY ? 0.f : __expf(o.m - mn);
    l = l * s1 + o.l * s2;
    for (int k = 0; k < NE; ++k) ex[k] = ex[k] * s1 + o.ex[k] * s2;
    m = mn;
    if (o.best > best || (o.best == best && o.bi < bi)) { best = o.best; bi = o.bi; }
    for (int d = 0; d < ND; ++d) dg[d] += o.dg[d];
  }

  // the state of lane ^ o
  __device__ __forceinline__ RowState shfl_xor(int o) const {
    RowState r{__shfl_xor(m, o, 64), __shfl_xor(l, o, 64), {}, __shfl_xor(best, o, 64), {}, __shfl_xor(bi, o, 64)};
    for (int k = 0; k < NE; ++k) r.ex[k] = __shfl_xor(ex[k], o, 64);
    for (int d = 0; d < ND; ++d) r.dg[d] = __shfl_xor(dg[d], o, 64);
    return r;
  }

  // the VALU kernels' combine, 64 lanes of one row: one rescale to the wave maximum, plain sums; every lane gets the result
  __device__ __forceinline__ void wave_reduce() {
    const float M = wave_max(m);
    const float sc = (m == -INFINITY) ? 0.f : __expf(m - M);
    l = wave_sum(l * sc);
    for (int k = 0; k < NE; ++k) ex[k] = wave_sum(ex[k] * sc);
    for (int d = 0; d < ND; ++d) dg[d] = wave_sum(dg[d]);
    const float wbest = wave_max(best);
    int cand = (best == wbest) ? bi : 0x7fffffff;
    for (int o = 32; o >= 1; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    m = M; best = wbest; bi = cand;
  }

  __device__ __forceinline__ void store(float* q) const {
    q[0] = m; q[1] = l; q[2 + NE] = best; q[3 + NE] = __int_as_float(bi);
    for (int k = 0; k < NE; ++k) q[2 + k] = ex[k];
    for (int d = 0; d < ND; ++d) q[4 + NE + d] = dg[d];
  }

  // The four wave records of one row, `stride` floats apart, in wave order -> its stats row
  //   {log-sum-exp, dg[ND-1], expectations / sum-exp, dg[0..ND-2], max logit, 0 up to STATS}  and its argmax.
  static __device__ __forceinline__ void finish(const float* red, int stride, float* st, int32_t* am) {
    float MM = -INFINITY, bb = -INFINITY, dd[ND] = {}, ll = 0.f, ee[NE] = {};
    int idx = 0x7fffffff;
    for (int w = 0; w < 4; ++w) {
      const float* r = red + w * stride;
      MM = fmaxf(MM, r[0]); bb = fmaxf(bb, r[2 + NE]);
      for (int d = 0; d < ND; ++d) dd[d] += r[4 + NE + d];
    }
    for (int w = 0; w < 4; ++w) {
      const float* r = red + w * stride;
      const float s2 = (r[0] == -INFINITY) ? 0.f : __expf(r[0] - MM);
      ll = fmaf(r[1], s2, ll);         // fmaf: what `ll += r[1] * s2` contracts to, whatever else gets vectorised
      for (int k = 0; k < NE; ++k) ee[k] = fmaf(r[2 + k], s2, ee[k]);
      if (r[2 + NE] == bb) idx = min(idx, __float_as_int(r[3 + NE]));
    }
    st[0] = MM + __logf(ll); st[1] = dd[ND - 1];
    for (int k = 0; k < NE; ++k) st[2 + k] = ee[k] / ll;
    for (int d = 0; d < ND - 1; ++d) st[2 + NE + d] = dd[d];
    st[1 + NE + ND] = bb;
    for (int z = 2 + NE + ND; z < STATS; ++z) st[z] = 0.f;
    *am = idx;
  }
};
