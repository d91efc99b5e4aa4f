// The WRF benchmark (gfx950): a regular-grid field onto the curvilinear WRF points with NaN outside the source axes
// (scripts/compare_wrf_era5.py:127-152), the NaN-masked paired scores behind compute_metrics (:155-164) and the
// WRF-box mean of a denormalised forecast in numpy's float32 order (scripts/compare_wrf.py:160-170, :202-203,
// :385-386).  No floating-point atomics; every reduction has a fixed order.
#include <hip/hip_fp16.h>

#include "common.h"

using gcl::rounded;

namespace {

constexpr int kSrcMask = 3;   // side kind: 0 float32 point field, 1 / 2 grid field of source 0 / 1, 3 float64 point field
constexpr int kConvert = 4;   // side kind bit: apply the float32 conversion (point: * mul; grid: * mul, then + add)
constexpr int kJobI = 6;      // int64 per job: kind a, offset a, kind b, offset b, gated, delta
constexpr int kJobF = 4;      // float per job: mul a, add a, mul b, add b
constexpr int kStats = 6;     // n, sum d, sum d^2, sum |d|, sum a, sum b

struct Source {
  const void* v;       // float32 or fp16 values
  const int32_t* pos;  // [P, 4]
  const double* w;     // [P, 4]
  int64_t stride;      // elements between two nodes of a field
  int32_t half;
};

__device__ __forceinline__ float load_value(const void* base, int32_t half, int64_t i) {
  return half ? __half2float(static_cast<const __half*>(base)[i]) : static_cast<const float*>(base)[i];
}

// One WRF point of one field: the four corners (lon, lat), (lon, lat+1), (lon+1, lat), (lon+1, lat+1), every product
// rounded on its own and added in that order onto 0.0 (scipy's RegularGridInterpolator on float32 values); NaN when the
// table marks the point as outside the source axes (bounds_error=False, fill_value=nan).
__device__ __forceinline__ double sample_point(const Source& s, int64_t off, int32_t i, bool conv, float mul, float add) {
  const int32_t* pi = s.pos + (int64_t)i * 4;
  if (pi[0] < 0) return __longlong_as_double(0x7ff8000000000000ll);
  const double* wi = s.w + (int64_t)i * 4;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = load_value(s.v, s.half, off + (int64_t)pi[k] * s.stride);
    if (conv) {
      v = rounded(v * mul);
      v = rounded(v + add);
    }
    acc = acc + rounded((double)v * wi[k]);
  }
  return acc;
}

// out[f, i]: one thread per (field, point), the point the fastest index
__global__ __launch_bounds__(256) void wrf_sample_kernel(Source s, const int64_t* __restrict__ field_off,
                                                         const float* __restrict__ mul, const float* __restrict__ add,
                                                         int32_t nf, int32_t P, double* __restrict__ out) {
  const int64_t total = (int64_t)nf * P;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int32_t f = (int32_t)(e / P), i = (int32_t)(e - (int64_t)f * P);
    const bool conv = mul != nullptr;
    out[e] = sample_point(s, field_off[f], i, conv, conv ? mul[f] : 1.f, conv ? add[f] : 0.f);
  }
}

struct ScoreArgs {
  Source src[2];
  const float* pts;        // point fields (WRF values on the WRF grid), float32
  const double* pts64;     // point fields already in float64 (a sampled field)
  const int64_t* jobs;     // [J, kJobI]
  const float* conv;       // [J, kJobF]
  const int64_t* offsets;  // [J / S] sample offsets of the gated jobs, or nullptr
  int64_t target;
  double* part;            // [J, nchunk, kStats]
  int32_t J, S, P, nchunk;
};

__device__ __forceinline__ bool job_runs(const ScoreArgs& a, int32_t j) {
  const int64_t* job = a.jobs + (int64_t)j * kJobI;
  return job[4] == 0 || (a.offsets != nullptr && a.offsets[j / a.S] == a.target + job[5]);
}

__device__ __forceinline__ double side_value(const ScoreArgs& a, int64_t kind, int64_t off, float mul, float add,
                                             int32_t i) {
  const bool conv = (kind & kConvert) != 0;
  const int which = (int)(kind & kSrcMask);
  if (which == 0) {
    float v = a.pts[off + i];
    if (conv) v = rounded(v * mul);
    return (double)v;
  }
  if (which == 3) return a.pts64[off + i];
  return sample_point(a.src[which - 1], off, i, conv, mul, add);
}

// Stage 1: block (job, chunk) takes the points chunk * 256 .. of its job, one per thread; the 64 lanes of a wave are
// combined by a fixed butterfly and the four waves in wave order.
__global__ __launch_bounds__(256) void wrf_scores_kernel(ScoreArgs a) {
  __shared__ double s_part[4][kStats];
  const int32_t j = blockIdx.x / a.nchunk, c = blockIdx.x - j * a.nchunk;
  if (!job_runs(a, j)) return;  // (the whole block takes this branch)
  const int64_t* job = a.jobs + (int64_t)j * kJobI;
  const float* cv = a.conv + (int64_t)j * kJobF;
  const int32_t i = c * 256 + threadIdx.x;
  double v[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < a.P) {
    const double x = side_value(a, job[0], job[1], cv[0], cv[1], i);
    const double y = side_value(a, job[2], job[3], cv[2], cv[3], i);
    if (!(x != x || y != y)) {
      const double d = x - y;
      v[0] = 1.0;
      v[1] = d;
      v[2] = rounded(d * d);
      v[3] = fabs(d);
      v[4] = x;
      v[5] = y;
    }
  }
#pragma unroll
  for (int q = 0; q < kStats; ++q) v[q] = gcl::wave_sum(v[q]);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < kStats; ++q) s_part[wv][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < kStats) {
    const int q = threadIdx.x;
    double t = s_part[0][q];
    for (int k = 1; k < 4; ++k) t += s_part[k][q];
    a.part[((int64_t)j * a.nchunk + c) * kStats + q] = t;
  }
}

// Stage 2: one thread per (slot, statistic), the six threads of a slot in one block (42 slots per block).  The jobs of
// slot s are s, s + S, s + 2 S, .. (one per sample), taken in that order; a job's own sum is its chunks in chunk order.
// A gated job counts only when its sample's offset is the target + its delta and its slot is still empty (the first
// such sample, as the reference picks it).
constexpr int kSlotsPerBlock = 42;

__global__ __launch_bounds__(256) void wrf_scores_finish_kernel(ScoreArgs a, int32_t* __restrict__ filled,
                                                                int32_t accumulate, double* __restrict__ stats) {
  const int32_t s = blockIdx.x * kSlotsPerBlock + (int32_t)threadIdx.x / kStats, q = (int32_t)threadIdx.x % kStats;
  const bool active = threadIdx.x < kSlotsPerBlock * kStats && s < a.S;
  bool took = false;
  if (active) {
    const int64_t e = (int64_t)s * kStats + q;
    double acc = accumulate ? stats[e] : 0.0;
    const bool full = filled != nullptr && filled[s] != 0;
    for (int32_t j = s; j < a.J; j += a.S) {
      const bool gated = a.jobs[(int64_t)j * kJobI + 4] != 0;
      if (!job_runs(a, j) || (gated && (full || took))) continue;
      double t = 0.0;
      for (int32_t c = 0; c < a.nchunk; ++c) t += a.part[((int64_t)j * a.nchunk + c) * kStats + q];
      acc += t;
      took = took || gated;
    }
    stats[e] = acc;
  }
  __syncthreads();  // the six threads of a slot have all read `filled` before one of them writes it
  if (active && took && q == 0 && filled != nullptr) filled[s] = 1;
}

// out[(count) + s, k]: numpy's float32 mean over a non-last axis - the first listed row, then the others added in
// their listed order, every product and sum rounded on its own, divided by (float)R.
__global__ __launch_bounds__(256) void wrf_box_means_kernel(const float* __restrict__ x, int64_t bs, int64_t gs,
                                                            const int32_t* __restrict__ rows, int32_t R,
                                                            const float* __restrict__ stdv, const float* __restrict__ mean,
                                                            int32_t C, int32_t K, int32_t B, float* __restrict__ out,
                                                            int64_t ldo, const int64_t* __restrict__ count, int64_t cap) {
  const int64_t total = (int64_t)B * K;
  const int64_t first = count ? count[0] : 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t s = e / K;
    const int32_t k = (int32_t)(e - s * K);
    if (first + s >= cap) continue;
    const float sd = stdv[k % C], mu = mean[k % C];
    const float* p = x + s * bs + k;
    float acc = 0.f;
    for (int32_t r = 0; r < R; ++r) {
      float t = rounded(p[(int64_t)rows[r] * gs] * sd);
      t = rounded(t + mu);
      acc = r == 0 ? t : rounded(acc + t);
    }
    out[(first + s) * ldo + k] = acc / (float)R;
  }
}

int fill_source(Source& s, const void* v, int32_t half, int64_t stride, const int32_t* pos, const double* w) {
  s.v = v; s.half = half; s.stride = stride; s.pos = pos; s.w = w;
  return 0;
}

}  // namespace

extern "C" int gcl_wrf_sample(const void* src, int32_t half, int64_t node_stride, const int64_t* field_off,
                              const float* mul, const float* add, int32_t nf, const int32_t* pos, const double* w,
                              int32_t P, double* out, gcl_stream_t stream) {
  GCL_CHECK_ARG(src && field_off && pos && w && out, "wrf_sample: null argument");
  GCL_CHECK_ARG((mul == nullptr) == (add == nullptr), "wrf_sample: mul and add go together");
  GCL_CHECK_ARG(nf > 0 && P > 0 && node_stride > 0 && (half == 0 || half == 1),
                "wrf_sample: bad shape (nf=%d P=%d node stride %lld half=%d)", nf, P, (long long)node_stride, half);
  Source s;
  fill_source(s, src, half, node_stride, pos, w);
  hipLaunchKernelGGL(wrf_sample_kernel, dim3(gcl::grid_for((int64_t)nf * P)), dim3(256), 0, (hipStream_t)stream, s,
                     field_off, mul, add, nf, P, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" size_t gcl_wrf_scores_ws_bytes(int32_t J, int32_t P) {
  if (J <= 0 || P <= 0) return 0;
  return (size_t)J * (size_t)gcl::cdiv(P, 256) * kStats * sizeof(double);
}

extern "C" int gcl_wrf_scores(const void* src0, int32_t half0, int64_t stride0, const int32_t* pos0, const double* w0,
                              const void* src1, int32_t half1, int64_t stride1, const int32_t* pos1, const double* w1,
                              const float* pts, const double* pts64, const int64_t* jobs, const float* conv, int32_t J,
                              int32_t S, int32_t P, const int64_t* offsets, int64_t target, int32_t* filled, int32_t accumulate,
                              double* stats, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(jobs && conv && stats && ws, "wrf_scores: null argument");
  GCL_CHECK_ARG(J > 0 && P > 0 && S > 0 && J % S == 0, "wrf_scores: bad shape (J=%d S=%d P=%d; J must be a multiple of S)",
                J, S, P);
  GCL_CHECK_ARG((src0 == nullptr) == (pos0 == nullptr) && (pos0 == nullptr) == (w0 == nullptr) &&
                    (src1 == nullptr) == (pos1 == nullptr) && (pos1 == nullptr) == (w1 == nullptr),
                "wrf_scores: a source and its point tables go together");
  GCL_CHECK_ARG((half0 == 0 || half0 == 1) && (half1 == 0 || half1 == 1) && (!src0 || stride0 > 0) &&
                    (!src1 || stride1 > 0), "wrf_scores: bad source description");
  const int64_t nchunk = gcl::cdiv(P, 256);
  GCL_CHECK_ARG((int64_t)J * nchunk < (1ll << 31), "wrf_scores: too many blocks (J=%d P=%d)", J, P);
  GCL_CHECK_ARG(ws_bytes >= gcl_wrf_scores_ws_bytes(J, P), "wrf_scores: workspace of %zu bytes, need %zu", ws_bytes,
                gcl_wrf_scores_ws_bytes(J, P));
  ScoreArgs a;
  fill_source(a.src[0], src0, half0, stride0, pos0, w0);
  fill_source(a.src[1], src1, half1, stride1, pos1, w1);
  a.pts = pts; a.pts64 = pts64; a.jobs = jobs; a.conv = conv; a.offsets = offsets; a.target = target;
  a.part = static_cast<double*>(ws);
  a.J = J; a.S = S; a.P = P; a.nchunk = (int32_t)nchunk;
  hipLaunchKernelGGL(wrf_scores_kernel, dim3((unsigned)(J * nchunk)), dim3(256), 0, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(wrf_scores_finish_kernel, dim3((unsigned)gcl::cdiv(S, kSlotsPerBlock)), dim3(256), 0,
                     (hipStream_t)stream, a, filled, accumulate, stats);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_wrf_box_means(const float* x, int64_t bs, int64_t gs, const int32_t* rows, int32_t R,
                                 const float* stdv, const float* mean, int32_t C, int32_t K, int32_t B, float* out,
                                 int64_t ldo, const int64_t* count, int64_t cap, gcl_stream_t stream) {
  GCL_CHECK_ARG(x && rows && stdv && mean && out, "wrf_box_means: null argument");
  GCL_CHECK_ARG(R > 0, "wrf_box_means: empty row list (the mean of no rows is undefined)");
  GCL_CHECK_ARG(C > 0 && K > 0 && K % C == 0 && B > 0 && ldo >= K && cap > 0,
                "wrf_box_means: bad shape (C=%d K=%d B=%d ldo=%lld cap=%lld)", C, K, B, (long long)ldo, (long long)cap);
  hipLaunchKernelGGL(wrf_box_means_kernel, dim3(gcl::grid_for((int64_t)B * K)), dim3(256), 0, (hipStream_t)stream, x, bs,
                     gs, rows, R, stdv, mean, C, K, B, out, ldo, count, cap);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
