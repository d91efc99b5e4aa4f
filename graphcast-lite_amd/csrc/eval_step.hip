// Fused validation step: the scores of the reference's test() (src/train.py:241-309) for one batch, in one pass over
// the data and without a host read.
//
// Column statistics.  The one-step prediction o is formed on the fly exactly as gcl_ar_advance forms its step_out
// (o = residual ? x_last + delta : delta in float32; static channels take x_last, forcing channels take y) and is
// stored only when the caller passes `out`.  For every (sample b, channel c) seven float64 sums over the G nodes:
//   [0] sum (o - y)^2          [1] sum node_w[g] (o - y)^2
//   [2] sum o'   [3] sum o'^2   [4] sum y'   [5] sum y'^2   [6] sum o' y'      o' = o - o[b,0,c],  y' = y - y[b,0,c]
// The shift by the column's first node takes the cancellation out of the one-pass variances, and a column that is
// constant over the nodes has exactly zero centred sums.  Two launches with a fixed order, as in csrc/verify.hip: the
// partial kernel sums fixed chunks of rows, the combine kernel sums a column's chunks in a fixed order
// (csrc/colsum.h, which also says why a (b, c) result depends on its own data and G only).
//
// Accumulate.  One launch folds the [B,C,7] sums into the float64 state [sum loss, sum acc, sum raw_mse, batches]
// of an evaluation pass: the weighted MSE (src/train.py:85-102), the spatial anomaly correlation (:114-130, per
// sample, unbiased std + 1e-8, static / forcing channels left out unless that leaves none) and the unweighted MSE.
#include "colsum.h"
#include "common.h"

namespace {

using gcl::chunk_rows;
using gcl::kColTile;
using gcl::kRowLanes;
using gcl::num_chunks;

constexpr int kNS = 7;  // sums per (b, c)

struct EvalIn {
  const float *delta, *x_last, *y, *node_w;
  int64_t ldd, bsd, ldx, bsx, ldy, bsy;
  const int32_t* chan_kind;
  int32_t residual;
  float* out;
  int64_t ldo, bso;
};

// The prediction of node g, channel c of sample b: the arithmetic of ar_advance_kernel (csrc/misc.hip).
__device__ __forceinline__ float predict(const EvalIn& a, int kind, int64_t b, int64_t g, int c, float yv) {
  const float xl = a.x_last[b * a.bsx + g * a.ldx + c];
  float v = a.delta[b * a.bsd + g * a.ldd + c];
  if (a.residual) v += xl;
  if (kind == 1) v = xl;
  else if (kind == 2) v = yv;
  return v;
}

// Partial sums of chunk blockIdx.x, columns [kColTile * blockIdx.y, ...), sample blockIdx.z.
// part layout: [B][C][kNS][nchunk] (a column's chunks contiguous for the combine kernel).
__global__ __launch_bounds__(256) void eval_partial_kernel(EvalIn a, int32_t G, int32_t C, double* __restrict__ part) {
  __shared__ double red[kNS][256];
  const int tid = threadIdx.x;
  const int cl = tid % kColTile, lane_r = tid / kColTile;
  const int c = blockIdx.y * kColTile + cl;
  const int ch = blockIdx.x;
  const int64_t b = blockIdx.z;
  const int crow = chunk_rows(G), nchunk = num_chunks(G);
  const int i0 = ch * crow, i1 = min(G, i0 + crow);
  const bool live = c < C;
  double acc[kNS];
#pragma unroll
  for (int s = 0; s < kNS; ++s) acc[s] = 0.0;
  if (live) {
    const int kind = a.chan_kind ? a.chan_kind[c] : 0;
    const float* yb = a.y + b * a.bsy + c;
    const float y0f = yb[0];
    const double y0 = (double)y0f;
    const double o0 = (double)predict(a, kind, b, 0, c, y0f);
    // Positions i0 + lane_r + kRowLanes * j, j ascending: fixed per (G, position) whatever C is.
    for (int g = i0 + lane_r; g < i1; g += kRowLanes) {
      const float yv = yb[(int64_t)g * a.ldy];
      const float ov = predict(a, kind, b, g, c, yv);
      if (a.out) a.out[b * a.bso + (int64_t)g * a.ldo + c] = ov;
      const double d = (double)ov - (double)yv;
      const double dd = d * d;
      const double op = (double)ov - o0, yp = (double)yv - y0;
      acc[0] += dd;
      acc[1] += a.node_w ? (double)a.node_w[g] * dd : dd;
      acc[2] += op;
      acc[3] = fma(op, op, acc[3]);
      acc[4] += yp;
      acc[5] = fma(yp, yp, acc[5]);
      acc[6] = fma(op, yp, acc[6]);
    }
  }
  gcl::lanes_to_part(red, acc, tid, kRowLanes, kColTile, lane_r == 0 && live, part + (b * C + c) * kNS * nchunk + ch,
                     nchunk);
}

// One wave per (column blockIdx.x, sample blockIdx.y): lane l sums chunks l, l + 64, .. in ascending order, then the
// fixed butterfly over the lanes.  stats[(b * C + c) * 7 + s].
__global__ __launch_bounds__(64) void eval_combine_kernel(const double* __restrict__ part, int32_t G, int32_t C,
                                                          double* __restrict__ stats) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int nchunk = num_chunks(G);
  const double* src = part + (b * C + c) * kNS * nchunk;
  double v[kNS];
  gcl::wave_strided_sum(src, nchunk, lane, v);
  if (lane < kNS) {
    double pick = v[0];
#pragma unroll
    for (int s = 1; s < kNS; ++s) pick = lane == s ? v[s] : pick;
    stats[(b * C + c) * kNS + lane] = pick;
  }
}

// One block.  Thread t takes the (b, c) pairs t, t + 256, .. in ascending order, the block sums its threads in a
// fixed tree, thread 0 adds the batch's three scores and 1 to the state.
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const double* __restrict__ stats,
                                                              const float* __restrict__ chan_w,
                                                              const int32_t* __restrict__ chan_kind, double inv_wsum,
                                                              int32_t B, int32_t G, int32_t C, double* __restrict__ state) {
  __shared__ double red[3][256];
  const int tid = threadIdx.x;
  int nkept = 0;
  if (chan_kind)
    for (int c = 0; c < C; ++c) nkept += chan_kind[c] == 0;
  const bool keep_all = nkept == 0;  // src/train.py:126-130: an exclusion that leaves nothing is ignored
  if (keep_all) nkept = C;
  const double n = (double)G;
  double loss = 0.0, acc = 0.0, raw = 0.0;
  const int64_t total = (int64_t)B * C;
  for (int64_t i = tid; i < total; i += 256) {
    const int c = (int)(i % C);
    const double* s = stats + i * kNS;
    raw += s[0];
    loss += chan_w ? (double)chan_w[c] * s[1] : s[1];
    if (keep_all || chan_kind[c] == 0) {
      const double cov = (s[6] - s[2] * (s[4] / n)) / n;
      const double so = sqrt(fmax(s[3] - s[2] * (s[2] / n), 0.0) / (n - 1.0));
      const double sy = sqrt(fmax(s[5] - s[4] * (s[4] / n), 0.0) / (n - 1.0));
      acc += cov / ((so + 1e-8) * (sy + 1e-8));
    }
  }
  red[0][tid] = loss, red[1][tid] = acc, red[2][tid] = raw;
  gcl::block_tree_sum(red, tid);
  if (tid == 0) {
    state[0] += inv_wsum * red[0][0];
    state[1] += red[1][0] / ((double)B * (double)nkept);
    state[2] += red[2][0] / ((double)B * n * (double)C);
    state[3] += 1.0;
  }
}

}  // namespace

extern "C" size_t gcl_eval_colstats_ws_bytes(int32_t B, int32_t G, int32_t C) {
  if (B <= 0 || G <= 0 || C <= 0) return 0;
  return (size_t)B * C * kNS * num_chunks(G) * sizeof(double);
}

extern "C" int gcl_eval_colstats(const float* delta, int64_t ldd, int64_t bsd, const float* x_last, int64_t ldx,
                                 int64_t bsx, const float* y, int64_t ldy, int64_t bsy, const float* node_w,
                                 const int32_t* chan_kind, int32_t residual, float* out, int64_t ldo, int64_t bso,
                                 double* stats, int32_t B, int32_t G, int32_t C, void* ws, size_t ws_bytes,
                                 gcl_stream_t stream) {
  GCL_CHECK_ARG(delta && x_last && y && stats, "eval_colstats: null argument");
  GCL_CHECK_ARG(B > 0 && G > 0 && C > 0, "eval_colstats: bad shape (B=%d, G=%d, C=%d)", B, G, C);
  GCL_CHECK_ARG(G >= 2, "eval_colstats: G=%d, the unbiased standard deviation needs at least 2 nodes", G);
  GCL_CHECK_ARG(ldd >= C && ldx >= C && ldy >= C && (!out || ldo >= C), "eval_colstats: a row stride is smaller than C=%d", C);
  GCL_CHECK_ARG(B <= 65535 && C <= 65535, "eval_colstats: B=%d or C=%d above 65535", B, C);
  const size_t need = gcl_eval_colstats_ws_bytes(B, G, C);
  GCL_CHECK_ARG(ws && ws_bytes >= need, "eval_colstats: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  EvalIn a{delta, x_last, y, node_w, ldd, bsd, ldx, bsx, ldy, bsy, chan_kind, residual, out, ldo, bso};
  double* part = (double*)ws;
  hipLaunchKernelGGL(eval_partial_kernel, dim3(num_chunks(G), (unsigned)gcl::cdiv(C, kColTile), B), dim3(256), 0, st, a, G,
                     C, part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(eval_combine_kernel, dim3(C, B), dim3(64), 0, st, (const double*)part, G, C, stats);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_eval_accumulate(const double* stats, const float* chan_w, const int32_t* chan_kind, double inv_wsum,
                                   int32_t B, int32_t G, int32_t C, double* state, gcl_stream_t stream) {
  GCL_CHECK_ARG(stats && state, "eval_accumulate: null argument");
  GCL_CHECK_ARG(B > 0 && C > 0, "eval_accumulate: bad shape (B=%d, C=%d)", B, C);
  GCL_CHECK_ARG(G >= 2, "eval_accumulate: G=%d, the unbiased standard deviation needs at least 2 nodes", G);
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, chan_w, chan_kind,
                     inv_wsum, B, G, C, state);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
