// Glue of the full-pipeline evaluation (scripts/evaluate_full_pipeline.py:449-666) between the rollout, MOS and OI
// kernels (gfx950): ROI rows in physical units with the lapse-rate copy, simulated station observations, and the
// per-variant squared-error sums.  Every operation whose rounding numpy fixes goes through gcl::rounded.
#include "common.h"

using gcl::rounded;

namespace {

constexpr double kLapseRate = 6.5e-3;  // K/m, scripts/evaluate_full_pipeline.py:50

// t2m + (z_surf - elevation) * LAPSE_RATE as numpy 2 evaluates it (:193-199).  f64 == 0: the elevation is a Python
// float (a weak scalar), every step is float32.  f64 == 1: it is a float64 (a strong scalar), the difference and the
// product are float64 and the in-place add rounds (double)t + delta to float32 once.
__device__ __forceinline__ float lapse_t(float t, float z, double elev, int f64) {
  if (f64) {
    const double dt = rounded(rounded((double)z - elev) * kLapseRate);
    return (float)((double)t + dt);
  }
  const float dt = rounded(rounded(z - (float)elev) * (float)kLapseRate);
  return t + dt;
}

// raw[g, c] = v * std[c] + mean[c] (float32, product and sum rounded separately) with v = pred[rows[g], c]
// (+ x_last[rows[g], c] when residual); lapse = raw with the t2m column corrected by the row's own z_surf.
__global__ __launch_bounds__(256) void roi_phys_kernel(const float* __restrict__ pred, int64_t ldp,
                                                       const float* __restrict__ x_last, int64_t ldx,
                                                       const int32_t* __restrict__ rows, int32_t row0, int32_t G,
                                                       int32_t C, const float* __restrict__ mean,
                                                       const float* __restrict__ stdv, int32_t t_idx, int32_t z_idx,
                                                       double elev, int32_t f64, float* __restrict__ raw,
                                                       float* __restrict__ lapse) {
  const int64_t total = (int64_t)G * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int32_t g = (int32_t)(i / C), c = (int32_t)(i - (int64_t)g * C);
    const int64_t src = rows ? rows[g] : row0 + g;
    auto phys = [&](int32_t cc) {
      float v = pred[src * ldp + cc];
      if (x_last) v = x_last[src * ldx + cc] + v;
      return rounded(v * stdv[cc]) + mean[cc];
    };
    const float p = phys(c);
    raw[i] = p;
    if (lapse) lapse[i] = (c == t_idx && z_idx >= 0) ? lapse_t(p, phys(z_idx), elev, f64) : p;
  }
}

// out = in [G, S, C] with the t2m column of every step corrected by z_surf of step 0 (:192-199)
__global__ __launch_bounds__(256) void lapse_kernel(const float* __restrict__ in, float* __restrict__ out, int32_t G,
                                                    int32_t S, int32_t C, int32_t t_idx, int32_t z_idx, double elev,
                                                    int32_t f64) {
  const int64_t total = (int64_t)G * S * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int32_t c = (int32_t)(i % C);
    const int64_t g = i / ((int64_t)S * C);
    const float v = in[i];
    out[i] = c == t_idx ? lapse_t(v, in[g * S * C + z_idx], elev, f64) : v;
  }
}

// out = in [G, S, C] with the t2m column of every step corrected by the lapse formula of scripts/mos_idw_sweep_v2.py
// (apply_lapse_correction, :73-84): z_surf of step 0 is a geopotential, every operand a float32 array or a weak Python
// float, so every step is float32: t2m + f32(6.5e-3 * f32(f32(z / 9.80665) - elev)).
__global__ __launch_bounds__(256) void lapse_geopotential_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                 int32_t G, int32_t S, int32_t C, int32_t t_idx,
                                                                 int32_t z_idx, float elev) {
  const int64_t total = (int64_t)G * S * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int32_t c = (int32_t)(i % C);
    const int64_t g = i / ((int64_t)S * C);
    const float v = in[i];
    if (c == t_idx) {
      const float dh = rounded(in[g * S * C + z_idx] / 9.80665f) - elev;
      out[i] = v + rounded((float)kLapseRate * dh);
    } else {
      out[i] = v;
    }
  }
}

// obs[g, :] = truth[g, :] where g is a station's grid point, NaN elsewhere (:210-220)
__global__ __launch_bounds__(256) void station_obs_kernel(const float* __restrict__ truth, int64_t ldt,
                                                          const int32_t* __restrict__ stn, int32_t S, int32_t G,
                                                          int32_t C, float* __restrict__ obs) {
  const int64_t total = (int64_t)G * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int32_t g = (int32_t)(i / C), c = (int32_t)(i - (int64_t)g * C);
    bool hit = false;
    for (int32_t s = 0; s < S; ++s) hit |= stn[s] == g;
    obs[i] = hit ? truth[(int64_t)g * ldt + c] : __builtin_nanf("");
  }
}

// One block per variant v: acc_grid[v, h, c] += sum_g (p - t)^2 and acc_stn[v, h, c] += the same over the station
// rows (in list order, duplicates counted as often as listed).  The difference and the square are float32 as in
// numpy (:647-652), the sums float64 in a fixed order: thread (lane, c) walks the rows lane, lane + L, ..., then
// the L lane sums of a column are added in lane order.  No atomics, so a repeated evaluation repeats its bits.
__global__ __launch_bounds__(256) void sqerr_kernel(const float* __restrict__ preds, int64_t vs, int64_t ldp,
                                                    const float* __restrict__ truth, int64_t ldt,
                                                    const int32_t* __restrict__ stn, int32_t S, int32_t G, int32_t C,
                                                    int32_t H, int32_t h, double* __restrict__ acc_grid,
                                                    double* __restrict__ acc_stn) {
  __shared__ double part[256];
  const int32_t v = blockIdx.x;
  const float* p = preds + (int64_t)v * vs;
  const int32_t L = 256 / C;
  const int32_t lane = threadIdx.x / C, c = threadIdx.x - lane * C;
  double s = 0.0;
  if (lane < L)
    for (int32_t g = lane; g < G; g += L) {
      const float d = p[(int64_t)g * ldp + c] - truth[(int64_t)g * ldt + c];
      s += (double)rounded(d * d);
    }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < C) {
    const int32_t cc = threadIdx.x;
    double tot = 0.0;
    for (int32_t l = 0; l < L; ++l) tot += part[l * C + cc];
    const int64_t at = ((int64_t)v * H + h) * C + cc;
    acc_grid[at] += tot;
    if (acc_stn) {
      double ts = 0.0;
      for (int32_t k = 0; k < S; ++k) {
        const int64_t g = stn[k];
        const float d = p[g * ldp + cc] - truth[g * ldt + cc];
        ts += (double)rounded(d * d);
      }
      acc_stn[at] += ts;
    }
  }
}

}  // namespace

extern "C" int gcl_pipeline_roi_phys(const float* pred, int64_t ldp, const float* x_last, int64_t ldx,
                                     const int32_t* rows, int32_t row0, int32_t G, int32_t C, const float* mean,
                                     const float* stdv, int32_t t_idx, int32_t z_idx, double elev, int32_t lapse_f64,
                                     float* raw, float* lapse, gcl_stream_t stream) {
  GCL_CHECK_ARG(pred && mean && stdv && raw, "pipeline_roi_phys: null argument");
  GCL_CHECK_ARG(G > 0 && C > 0 && ldp >= C && (!x_last || ldx >= C) && row0 >= 0, "pipeline_roi_phys: bad shape");
  GCL_CHECK_ARG(!lapse || (t_idx < C && z_idx < C && (t_idx >= 0) == (z_idx >= 0)),
                "pipeline_roi_phys: t2m / z_surf columns %d / %d outside the %d channels", t_idx, z_idx, C);
  hipLaunchKernelGGL(roi_phys_kernel, dim3(gcl::grid_for((int64_t)G * C)), dim3(256), 0, (hipStream_t)stream, pred, ldp,
                     x_last, ldx, rows, row0, G, C, mean, stdv, t_idx, z_idx, elev, lapse_f64, raw, lapse);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_pipeline_lapse(const float* in, float* out, int32_t G, int32_t S, int32_t C, int32_t t_idx,
                                  int32_t z_idx, double elev, int32_t lapse_f64, gcl_stream_t stream) {
  GCL_CHECK_ARG(in && out && in != out, "pipeline_lapse: null or aliased argument");
  GCL_CHECK_ARG(G > 0 && S > 0 && C > 0 && t_idx >= 0 && t_idx < C && z_idx >= 0 && z_idx < C,
                "pipeline_lapse: bad shape");
  hipLaunchKernelGGL(lapse_kernel, dim3(gcl::grid_for((int64_t)G * S * C)), dim3(256), 0, (hipStream_t)stream, in, out,
                     G, S, C, t_idx, z_idx, elev, lapse_f64);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_pipeline_lapse_geopotential(const float* in, float* out, int32_t G, int32_t S, int32_t C,
                                               int32_t t_idx, int32_t z_idx, double elev, gcl_stream_t stream) {
  GCL_CHECK_ARG(in && out && in != out, "pipeline_lapse_geopotential: null or aliased argument");
  GCL_CHECK_ARG(G > 0 && S > 0 && C > 0 && t_idx >= 0 && t_idx < C && z_idx >= 0 && z_idx < C && t_idx != z_idx,
                "pipeline_lapse_geopotential: bad shape (G=%d S=%d C=%d t2m=%d z_surf=%d)", G, S, C, t_idx, z_idx);
  hipLaunchKernelGGL(lapse_geopotential_kernel, dim3(gcl::grid_for((int64_t)G * S * C)), dim3(256), 0,
                     (hipStream_t)stream, in, out, G, S, C, t_idx, z_idx, (float)elev);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_pipeline_station_obs(const float* truth, int64_t ldt, const int32_t* stn, int32_t S, int32_t G,
                                        int32_t C, float* obs, gcl_stream_t stream) {
  GCL_CHECK_ARG(truth && obs && (S == 0 || stn), "pipeline_station_obs: null argument");
  GCL_CHECK_ARG(G > 0 && C > 0 && S >= 0 && ldt >= C, "pipeline_station_obs: bad shape");
  hipLaunchKernelGGL(station_obs_kernel, dim3(gcl::grid_for((int64_t)G * C)), dim3(256), 0, (hipStream_t)stream, truth,
                     ldt, stn, S, G, C, obs);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_pipeline_sqerr(const float* preds, int64_t vs, int64_t ldp, int32_t V, const float* truth,
                                  int64_t ldt, const int32_t* stn, int32_t S, int32_t G, int32_t C, int32_t H,
                                  int32_t h, double* acc_grid, double* acc_stn, gcl_stream_t stream) {
  GCL_CHECK_ARG(preds && truth && acc_grid, "pipeline_sqerr: null argument");
  GCL_CHECK_ARG(V > 0 && G > 0 && C > 0 && C <= 256 && ldp >= C && ldt >= C && H > 0 && h >= 0 && h < H && S >= 0,
                "pipeline_sqerr: bad shape (V=%d G=%d C=%d horizon %d of %d)", V, G, C, h, H);
  GCL_CHECK_ARG(!acc_stn || S == 0 || stn, "pipeline_sqerr: station sums need the station rows");
  hipLaunchKernelGGL(sqerr_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, preds, vs, ldp, truth, ldt, stn, S, G, C,
                     H, h, acc_grid, acc_stn);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
