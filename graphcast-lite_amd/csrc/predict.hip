// Station observations (scripts/create_obs.py:79-144, scripts/predict.py:394-421) and the regional scoring of a saved
// global forecast (scripts/interpolate_to_region.py:168-249).
//
// Observation pack.  obs[b, g, k] = y[b, g, k] where node g is a station and channel k % C is observed, the quiet NaN
// (bits 0x7fc00000) elsewhere.  One launch; rows that are whole and 16-byte aligned move as float4, a row that is not a
// station is never read.
//
// Regional scores.  For every matched sample s, horizon p, regional node i and channel c the float64 bilinear value v
// of the global forecast (the arithmetic of gcl_regrid_blend: four products rounded one by one, added left to right),
// the normalised regional truth t and persistence b from the fp16 series, and per (p, c) the sums
//   se = sum (v - t)^2, ae = sum |v - t|, bse = sum (b - t)^2, n, and St, Stt, Sv, Svv, Stv of t' = t - tp, v' = v - vp,
// tp / vp the values at node 0 of the first matched sample (the pivot of that (p, c)), so a channel whose mean is 1e4
// standard deviations from 0 loses nothing to cancellation.  Two launches with a fixed order and no atomics: a block
// sums a fixed chunk of nodes of one (sample, horizon) with the channel as the fast thread index (a thread keeps one
// channel, so its nine sums stay in registers), reduces its node lanes through LDS and writes one partial; the combine
// kernel adds the partials of a (p, c) in a fixed tree.
#include <hip/hip_fp16.h>

#include "colsum.h"
#include "common.h"

namespace {

constexpr uint32_t kQuietNaN = 0x7fc00000u;

__global__ __launch_bounds__(256) void obs_pack_vec_kernel(const float* y, int64_t ldy, int64_t bsy,
                                                           const uint8_t* __restrict__ keep_row,
                                                           const uint8_t* __restrict__ keep_chan, int32_t G, int32_t K,
                                                           int32_t C, float* obs, int64_t ldo, int64_t bso, int64_t total) {
  const int K4 = K >> 2;
  const float nan = __uint_as_float(kQuietNaN);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int q = (int)(t % K4);
    const int64_t rem = t / K4;
    const int g = (int)(rem % G);
    const int64_t b = rem / G;
    float4 o = make_float4(nan, nan, nan, nan);
    if (keep_row[g]) {
      const float4 v = gcl::ld4(y + b * bsy + (int64_t)g * ldy + 4 * q);
      const int k = 4 * q;
      if (keep_chan[k % C]) o.x = v.x;
      if (keep_chan[(k + 1) % C]) o.y = v.y;
      if (keep_chan[(k + 2) % C]) o.z = v.z;
      if (keep_chan[(k + 3) % C]) o.w = v.w;
    }
    gcl::st4(obs + b * bso + (int64_t)g * ldo + 4 * q, o);
  }
}

__global__ __launch_bounds__(256) void obs_pack_kernel(const float* y, int64_t ldy, int64_t bsy,
                                                       const uint8_t* __restrict__ keep_row,
                                                       const uint8_t* __restrict__ keep_chan, int32_t G, int32_t K, int32_t C,
                                                       float* obs, int64_t ldo, int64_t bso, int64_t total) {
  const float nan = __uint_as_float(kQuietNaN);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % K);
    const int64_t rem = t / K;
    const int g = (int)(rem % G);
    const int64_t b = rem / G;
    float o = nan;
    if (keep_row[g] && keep_chan[k % C]) o = y[b * bsy + (int64_t)g * ldy + k];
    obs[b * bso + (int64_t)g * ldo + k] = o;
  }
}

// ---- regional scores -------------------------------------------------------------------------------------------------
constexpr int kNS = 9;         // se, ae, bse, n, St, Stt, Sv, Svv, Stv
constexpr int kNOut = kNS + 2; // ... and the two pivots tp, vp
constexpr int kNodeIters = 32; // nodes per node lane of a block

struct RegionIn {
  const float* pred;  // [N, Gg, >= P * C]
  int64_t ldp, bsp;
  const int32_t* cell;  // [nr, 2] (lon, lat) of regrid_tables
  const double* w;      // [nr, 4]
  const __half* series;  // [n_time, nr, n_feat]
  const int32_t* t0;    // [N] regional step of horizon 0; a sample outside [1, n_time - P] is skipped
  const double* mean;   // [C]
  const double* std;    // [C]
  int32_t Gg, nlat, n_feat, n_time, first, N, P, nr, C;
};

__device__ __forceinline__ bool matched(const RegionIn& a, int t) { return t >= 1 && t <= a.n_time - a.P; }

// the bilinear value of column col of sample s at regional node i (NaN for a cell outside the source rows)
__device__ __forceinline__ double interp(const RegionIn& a, int s, int i, int col) {
  const int64_t n00 = (int64_t)a.cell[2 * i] * a.nlat + a.cell[2 * i + 1];
  if (a.cell[2 * i] < 0 || a.cell[2 * i + 1] < 0 || a.cell[2 * i + 1] + 1 >= a.nlat || n00 + a.nlat + 1 >= a.Gg)
    return __longlong_as_double(0x7ff8000000000000ll);
  return gcl::cell_corner_sum(a.pred + (int64_t)s * a.bsp + col, a.ldp, n00, a.nlat, a.w + 4 * (int64_t)i);
}

__device__ __forceinline__ double truth(const RegionIn& a, int t, int i, int c, double m, double sd) {
  return ((double)__half2float(a.series[((int64_t)t * a.nr + i) * a.n_feat + c]) - m) / sd;
}

// pivots of (p, c): node 0 of the first matched sample; 0 when there is none
__device__ __forceinline__ void pivots(const RegionIn& a, int p, int c, double m, double sd, double& tp, double& vp) {
  tp = vp = 0.0;
  const int tf = a.t0[a.first];
  if (!matched(a, tf)) return;
  tp = truth(a, tf + p, 0, c, m, sd);
  vp = interp(a, a.first, 0, p * a.C + c);
}

// Block (chunk blockIdx.x, horizon blockIdx.y, sample blockIdx.z); thread tid: channel tid % C, node lane tid / C of
// R = 256 / C lanes.  part layout: [P * C][kNS][N * nchunk] (the partials of a sum contiguous for the combine kernel).
__global__ __launch_bounds__(256) void region_partial_kernel(RegionIn a, double* __restrict__ part, float* __restrict__ vout,
                                                             float* __restrict__ tout) {
  __shared__ double red[kNS][256];
  const int tid = threadIdx.x;
  const int C = a.C, R = 256 / C;
  const int c = tid % C, lane = tid / C;
  const int chunk = blockIdx.x, p = blockIdx.y, s = blockIdx.z;
  const int nchunk = gridDim.x;
  const int ts = a.t0[s];
  double acc[kNS];
#pragma unroll
  for (int q = 0; q < kNS; ++q) acc[q] = 0.0;
  if (lane < R && matched(a, ts)) {
    const double m = a.mean[c], sd = a.std[c];
    double tp, vp;
    pivots(a, p, c, m, sd, tp, vp);
    const int i0 = chunk * R * kNodeIters + lane;
    for (int k = 0; k < kNodeIters; ++k) {
      const int i = i0 + k * R;
      if (i >= a.nr) break;
      const double v = interp(a, s, i, p * C + c);
      const double t = truth(a, ts + p, i, c, m, sd);
      const double b = truth(a, ts - 1, i, c, m, sd);
      const double d = v - t, db = b - t, tc = t - tp, vc = v - vp;
      acc[0] = fma(d, d, acc[0]);
      acc[1] += fabs(d);
      acc[2] = fma(db, db, acc[2]);
      acc[3] += 1.0;
      acc[4] += tc;
      acc[5] = fma(tc, tc, acc[5]);
      acc[6] += vc;
      acc[7] = fma(vc, vc, acc[7]);
      acc[8] = fma(tc, vc, acc[8]);
      if (vout) {
        const int64_t o = (((int64_t)s * a.P + p) * a.nr + i) * C + c;
        vout[o] = (float)v;
        tout[o] = (float)t;
      }
    }
  }
  const int64_t nparts = (int64_t)a.N * nchunk;
  gcl::lanes_to_part(red, acc, tid, R, C, tid < C,
                     part + (int64_t)(p * C + tid) * kNS * nparts + (int64_t)s * nchunk + chunk, nparts);
}

// One block per (p, c): the partials of each sum in a fixed tree; sums[(p * C + c) * kNOut + {0..8: the sums, 9: tp, 10: vp}]
__global__ __launch_bounds__(256) void region_combine_kernel(RegionIn a, const double* __restrict__ part, int64_t nparts,
                                                             double* __restrict__ sums) {
  __shared__ double red[kNS][256];
  const int pc = blockIdx.x, tid = threadIdx.x;
  const double* src = part + (int64_t)pc * kNS * nparts;
  for (int q = 0; q < kNS; ++q) red[q][tid] = gcl::strided_sum(src + (int64_t)q * nparts, nparts, tid);
  gcl::block_tree_sum(red, tid);
  double* o = sums + (int64_t)pc * kNOut;
  if (tid < kNS) o[tid] = red[tid][0];
  if (tid == 0) {
    const int p = pc / a.C, c = pc % a.C;
    double tp, vp;
    pivots(a, p, c, a.mean[c], a.std[c], tp, vp);
    o[kNS] = tp;
    o[kNS + 1] = vp;
  }
}

inline int region_nchunk(int32_t nr, int32_t C) { return (int)gcl::cdiv(nr, (int64_t)(256 / C) * kNodeIters); }

}  // namespace

extern "C" int gcl_obs_pack(const float* y, int64_t ldy, int64_t bsy, const uint8_t* keep_row, const uint8_t* keep_chan,
                            int32_t B, int32_t G, int32_t K, int32_t C, float* obs, int64_t ldo, int64_t bso,
                            gcl_stream_t stream) {
  GCL_CHECK_ARG(y && keep_row && keep_chan && obs, "obs_pack: null argument");
  GCL_CHECK_ARG(B >= 0 && G >= 0 && K > 0 && C > 0, "obs_pack: bad shape (B=%d, G=%d, K=%d, C=%d)", B, G, K, C);
  GCL_CHECK_ARG(ldy >= K && ldo >= K, "obs_pack: a leading dimension below K=%d", K);
  if ((int64_t)B * G == 0) return GCL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = K % 4 == 0 && ldy % 4 == 0 && bsy % 4 == 0 && ldo % 4 == 0 && bso % 4 == 0 && gcl::aligned16(y) &&
                   gcl::aligned16(obs);
  if (vec) {
    const int64_t total = (int64_t)B * G * (K / 4);
    hipLaunchKernelGGL(obs_pack_vec_kernel, dim3(gcl::grid_for(total, 2048)), dim3(256), 0, st, y, ldy, bsy, keep_row,
                       keep_chan, G, K, C, obs, ldo, bso, total);
  } else {
    const int64_t total = (int64_t)B * G * K;
    hipLaunchKernelGGL(obs_pack_kernel, dim3(gcl::grid_for(total, 2048)), dim3(256), 0, st, y, ldy, bsy, keep_row,
                       keep_chan, G, K, C, obs, ldo, bso, total);
  }
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" size_t gcl_region_interp_scores_ws_bytes(int32_t N, int32_t P, int32_t nr, int32_t C) {
  if (N <= 0 || P <= 0 || nr <= 0 || C <= 0 || C > 256) return 0;
  return (size_t)N * region_nchunk(nr, C) * P * C * kNS * sizeof(double);
}

extern "C" int gcl_region_interp_scores(const float* pred, int64_t ldp, int64_t bsp, int32_t Gg, int32_t nlat,
                                        const int32_t* cell, const double* w, const void* series, int32_t n_feat,
                                        int32_t n_time, const int32_t* t0, int32_t first, const double* mean,
                                        const double* std, int32_t N, int32_t P, int32_t nr, int32_t C, double* sums,
                                        float* vout, float* tout, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(pred && cell && w && series && t0 && mean && std && sums, "region_interp_scores: null argument");
  GCL_CHECK_ARG(N > 0 && P > 0 && nr > 0 && C > 0 && C <= 256, "region_interp_scores: bad shape (N=%d, P=%d, nr=%d, C=%d)",
                N, P, nr, C);
  GCL_CHECK_ARG(P <= 65535 && N <= 65535, "region_interp_scores: P=%d or N=%d above 65535", P, N);
  GCL_CHECK_ARG(n_feat >= C && n_time > 0 && nlat >= 2 && Gg >= 2 * nlat, "region_interp_scores: bad grid or series shape");
  GCL_CHECK_ARG(ldp >= (int64_t)P * C, "region_interp_scores: ldp=%lld below P * C", (long long)ldp);
  GCL_CHECK_ARG(first >= 0 && first < N, "region_interp_scores: first=%d outside [0, %d)", first, N);
  GCL_CHECK_ARG((vout == nullptr) == (tout == nullptr), "region_interp_scores: vout and tout go together");
  const size_t need = gcl_region_interp_scores_ws_bytes(N, P, nr, C);
  GCL_CHECK_ARG(ws && ws_bytes >= need, "region_interp_scores: workspace of %zu bytes, %zu needed", ws_bytes, need);
  RegionIn a{pred, ldp, bsp, cell, w, (const __half*)series, t0, mean, std, Gg, nlat, n_feat, n_time, first, N, P, nr, C};
  const hipStream_t st = (hipStream_t)stream;
  const int nchunk = region_nchunk(nr, C);
  hipLaunchKernelGGL(region_partial_kernel, dim3(nchunk, P, N), dim3(256), 0, st, a, (double*)ws, vout, tout);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(region_combine_kernel, dim3(P * C), dim3(256), 0, st, a, (const double*)ws, (int64_t)N * nchunk, sums);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
