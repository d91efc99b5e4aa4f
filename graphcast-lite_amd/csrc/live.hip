// Live forecast glue (gfx950): analysis fields on somebody else's regular lat/lon grid -> one normalised window slot
// (scripts/live_gdas_forecast.py:378-407, :460-483, :486-487, :617-620), and the city-box summary of the corrected
// forecast (:543-559).
#include "common.h"

using gcl::rounded;

namespace {

constexpr int kMaxDest = 16;  // window slots one launch can fill (gcl_live_max_dest)

struct PackArgs {
  const float* arena;       // the cycle's source fields, back to back, each in its own orientation
  const float* statics;     // [n_static, G] template rows
  const int64_t* chan;      // [C, 3]: kind (0 zero, 1 field, 2 static), arena offset / static row, point table
  const float* chan_div;    // [C] unit divisor of a field channel
  const int32_t* pos;       // [n_tab, G, 4] positions into the unsorted, unextended field
  const double* w;          // [n_tab, G, 4]
  const float* mean;
  const float* stdv;
  float* out;
  int64_t dest[kMaxDest];
  int64_t ldo;
  int32_t nd, G, C;
};

// One thread per (node, channel), the channel fastest: the C stores of a node are one contiguous run of its row.
// Field channels: scipy's RegularGridInterpolator in float64 - corners (lat, lon), (lat, lon+1), (lat+1, lon),
// (lat+1, lon+1) added in that order onto 0.0, every product rounded on its own - then float32, the unit divisor in
// float32, and the z-score with the subtraction and the division rounded separately.
__global__ __launch_bounds__(256) void live_frame_pack_kernel(PackArgs a) {
  const int64_t total = (int64_t)a.G * a.C;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t g = e / a.C;
    const int32_t c = (int32_t)(e - g * a.C);
    const int64_t kind = a.chan[3 * c], off = a.chan[3 * c + 1], tab = a.chan[3 * c + 2];
    float x = 0.f;
    if (kind == 1) {
      const float* s = a.arena + off;
      const int32_t* pi = a.pos + (tab * a.G + g) * 4;
      const double* wi = a.w + (tab * a.G + g) * 4;
      double acc = 0.0;
      for (int j = 0; j < 4; ++j) acc = acc + rounded((double)s[pi[j]] * wi[j]);
      x = rounded((float)acc) / a.chan_div[c];
    } else if (kind == 2) {
      x = a.statics[off * a.G + g];
    }
    const float z = rounded(x - a.mean[c]) / a.stdv[c];
    for (int d = 0; d < a.nd; ++d) a.out[a.dest[d] + g * a.ldo + c] = z;
  }
}

// NaN-propagating min / max, as numpy's reductions
__device__ __forceinline__ float nmin(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nmax(float a, float b) { return (b > a || b != b) ? b : a; }

// One block per (sample, step, listed channel).  Thread t takes the rows t, t + 256, .. in order, the 64 lanes of a
// wave are combined by a fixed butterfly and the four waves in wave order: the same bits on every run.
__global__ __launch_bounds__(256) void live_region_stats_kernel(const float* __restrict__ pred, int64_t bs, int64_t gs,
                                                                int64_t ss, const int32_t* __restrict__ rows, int32_t n,
                                                                const int32_t* __restrict__ chans,
                                                                const float* __restrict__ offs, int32_t nc, int32_t S,
                                                                double* __restrict__ out) {
  __shared__ double s_sum[4];
  __shared__ float s_min[4], s_max[4];
  const int32_t k = blockIdx.x % nc, s = (blockIdx.x / nc) % S, b = blockIdx.x / (nc * S);
  const float* p = pred + b * bs + s * ss + chans[k];
  const float off = offs[k];
  // every lane starts from row 0's value (it belongs to the set, so it changes neither extreme)
  float v0 = p[(int64_t)rows[0] * gs];
  if (off != 0.f) v0 = v0 + off;
  double sum = 0.0;
  float mn = v0, mx = v0;
  for (int32_t i = threadIdx.x; i < n; i += 256) {
    float v = p[(int64_t)rows[i] * gs];
    if (off != 0.f) v = v + off;
    sum += (double)v;
    mn = nmin(mn, v);
    mx = nmax(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    mn = nmin(mn, __shfl_xor(mn, o, 64));
    mx = nmax(mx, __shfl_xor(mx, o, 64));
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_sum[wv] = sum; s_min[wv] = mn; s_max[wv] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_sum[0];
    float lo = s_min[0], hi = s_max[0];
    for (int q = 1; q < 4; ++q) { t += s_sum[q]; lo = nmin(lo, s_min[q]); hi = nmax(hi, s_max[q]); }
    double* o = out + (int64_t)blockIdx.x * 3;
    o[0] = t / (double)n;
    o[1] = (double)lo;
    o[2] = (double)hi;
  }
}

}  // namespace

extern "C" int gcl_live_max_dest(void) { return kMaxDest; }

extern "C" int gcl_live_frame_pack(const float* arena, const float* statics, const int64_t* chan, const float* chan_div,
                                   const int32_t* pos, const double* w, const float* mean, const float* stdv,
                                   float* out, const int64_t* dest_off, int32_t nd, int64_t ldo, int32_t G, int32_t C,
                                   gcl_stream_t stream) {
  GCL_CHECK_ARG(chan && chan_div && mean && stdv && out && dest_off, "live_frame_pack: null argument");
  GCL_CHECK_ARG(G > 0 && C > 0 && ldo >= C && nd >= 1 && nd <= kMaxDest,
                "live_frame_pack: bad shape (G=%d C=%d ldo=%lld nd=%d, at most %d destinations)", G, C, (long long)ldo,
                nd, kMaxDest);
  GCL_CHECK_ARG((arena == nullptr) == (pos == nullptr) && (pos == nullptr) == (w == nullptr),
                "live_frame_pack: the field arena and the point tables go together");
  PackArgs a;
  a.arena = arena; a.statics = statics; a.chan = chan; a.chan_div = chan_div; a.pos = pos; a.w = w;
  a.mean = mean; a.stdv = stdv; a.out = out; a.ldo = ldo; a.nd = nd; a.G = G; a.C = C;
  for (int d = 0; d < kMaxDest; ++d) {
    a.dest[d] = d < nd ? dest_off[d] : 0;
    GCL_CHECK_ARG(a.dest[d] >= 0, "live_frame_pack: negative destination offset");
  }
  hipLaunchKernelGGL(live_frame_pack_kernel, dim3(gcl::grid_for((int64_t)G * C)), dim3(256), 0, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_live_region_stats(const float* pred, int64_t bs, int64_t gs, int64_t ss, const int32_t* rows,
                                     int32_t n, const int32_t* chans, const float* offs, int32_t nc, int32_t S,
                                     double* out, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(pred && rows && chans && offs && out, "live_region_stats: null argument");
  GCL_CHECK_ARG(n > 0, "live_region_stats: empty row list (the reference writes no city block then)");
  GCL_CHECK_ARG(nc > 0 && S > 0 && B > 0 && (int64_t)B * S * nc < (1ll << 31),
                "live_region_stats: bad shape (B=%d S=%d channels=%d)", B, S, nc);
  hipLaunchKernelGGL(live_region_stats_kernel, dim3((unsigned)(B * S * nc)), dim3(256), 0, (hipStream_t)stream, pred, bs,
                     gs, ss, rows, n, chans, offs, nc, S, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
