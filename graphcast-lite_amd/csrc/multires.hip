// Multi-resolution input windows straight from the device-resident series (gfx950): the flat node set of
// scripts/build_multires_dataset.py (kept global points, then the regional grid) is never materialised; a batch of
// windows is one launch over the global fp16 series (T, lon, lat, Ct) and, in merge mode, the regional one.
#include "common.h"

using gcl::rounded;

namespace {

constexpr int kRegRows = 64;  // regional rows of one block in interpolate mode

struct MrArgs {
  const _Float16* gs;  // global series (Tg, n_lon, n_lat, Ctg)
  int64_t Tg;
  int32_t n_lon, n_lat, Ctg;
  const _Float16* rs;  // regional series (Tr, rn_lon, rn_lat, Ctr), merge mode only
  int64_t Tr;
  int32_t rn_lon, rn_lat, Ctr;
  const int32_t* rank;    // [n_lat * n_lon] lat-major: output row of a global point, -1 when the box removed it
  const int32_t* corner;  // [n_reg, 4] positions lon * n_lat + lat of the four corners (interpolate mode)
  const double* w;        // [n_reg, 4] their float64 weights
  int32_t n_kept, n_reg;
  const int64_t* t0;
  int64_t off_g, off_r;
  const float* mean;  // NULL: no z-score
  const float* stdv;
  int32_t C, obs, pred, quantize, out_f16;
  void* X;
  void* Y;
  int32_t tile;     // points per tile side
  int32_t gt_lon;   // tiles along the longitude of the global grid
  int32_t n_gt;     // global tiles
  int32_t rt_lon;   // tiles along the longitude of the regional grid (merge mode)
};

__device__ __forceinline__ void put(void* out, int32_t out_f16, int64_t at, float v) {
  if (out_f16) reinterpret_cast<_Float16*>(out)[at] = (_Float16)v;
  else reinterpret_cast<float*>(out)[at] = v;
}

__device__ __forceinline__ float zscore(float x, const float* mean, const float* stdv, int c) {
  return mean ? (x - mean[c]) / stdv[c] : x;
}

// One tile of `tile` x `tile` (lon, lat) points of a (T, nlon, nlat, Ct) series, all `frames` frames of the window
// at once.  Load: runs of tile * Ct halves (latitude and channel are contiguous in the series) into LDS as
// [frame][lon][lat][c].  Store: for every latitude of the tile the rows of consecutive longitudes are consecutive
// output rows (the rank table skips the removed box), each a whole [frames * C] row - coalesced both ways.
__device__ void pack_tile(const _Float16* __restrict__ series, int64_t T, int32_t nlon, int32_t nlat, int32_t Ct,
                          const int32_t* __restrict__ rank, int32_t row_base, int32_t lon0, int32_t lat0, int64_t tb,
                          int32_t frames, const MrArgs& a, void* out, int64_t out_b, _Float16* lds) {
  const int32_t tile = a.tile, C = a.C;
  const int32_t nlo = min(tile, nlon - lon0), nla = min(tile, nlat - lat0);
  const int32_t run = nla * C, per_frame = nlo * run, total = frames * per_frame;
  const _Float16 nan16 = (_Float16)__builtin_nanf("");
  for (int32_t e = threadIdx.x; e < total; e += 256) {
    const int32_t f = e / per_frame, r = e - f * per_frame;
    const int32_t lo = r / run, q = r - lo * run;
    const int32_t la = q / C, c = q - la * C;
    const int64_t t = tb + f;
    _Float16 v = nan16;  // a window that leaves the series is an error made visible
    if (t >= 0 && t < T) v = series[((t * nlon + lon0 + lo) * nlat + lat0 + la) * Ct + c];
    lds[e] = v;
  }
  __syncthreads();
  const int32_t row = frames * C, per_lat = nlo * row;
  for (int32_t o = threadIdx.x; o < total; o += 256) {
    const int32_t la = o / per_lat, r = o - la * per_lat;
    const int32_t lo = r / row, k = r - lo * row;
    const int32_t f = k / C, c = k - f * C;
    const int32_t g = (lat0 + la) * nlon + lon0 + lo;
    const int32_t dst = rank ? rank[g] : row_base + g;
    if (dst < 0) continue;
    const float x = (float)lds[f * per_frame + lo * run + la * C + c];
    put(out, a.out_f16, out_b + (int64_t)dst * row + k, zscore(x, a.mean, a.stdv, c));
  }
}

// Regional rows of interpolate mode: the bilinear value of scipy's RegularGridInterpolator((lats, lons)) in float64,
// corners added in the order (lat, lon), (lat, lon+1), (lat+1, lon), (lat+1, lon+1) onto 0.0, every product rounded
// on its own, then float64 -> float32 (the reference's float32 buffer) and, when the dataset on disk is reproduced,
// -> float16 -> float32.
__device__ void interp_rows(int32_t r0, int64_t tb, int32_t frames, const MrArgs& a, void* out, int64_t out_b) {
  const int32_t C = a.C, row = frames * C;
  const int32_t nr = min(kRegRows, a.n_reg - r0);
  const int64_t frame_sz = (int64_t)a.n_lon * a.n_lat * a.Ctg;
  for (int32_t o = threadIdx.x; o < nr * row; o += 256) {
    const int32_t i = o / row, k = o - i * row;
    const int32_t f = k / C, c = k - f * C;
    const int64_t t = tb + f;
    float v = __builtin_nanf("");
    if (t >= 0 && t < a.Tg) {
      const _Float16* s = a.gs + t * frame_sz + c;
      const int32_t* ci = a.corner + 4 * (int64_t)(r0 + i);
      const double* wi = a.w + 4 * (int64_t)(r0 + i);
      double acc = 0.0;
      for (int j = 0; j < 4; ++j) acc = acc + rounded((double)(float)s[(int64_t)ci[j] * a.Ctg] * wi[j]);
      // two roundings, as numpy does them: opaque in between, or the compiler narrows float64 -> float16 in one step
      float x = rounded((float)acc);
      if (a.quantize) x = (float)(_Float16)x;
      v = zscore(x, a.mean, a.stdv, c);
    }
    put(out, a.out_f16, out_b + (int64_t)(a.n_kept + r0 + i) * row + k, v);
  }
}

// grid: x = global tiles, then the regional tiles (merge) or row chunks (interpolate); y = window of the batch;
// z = 0: the obs frames into X, 1: the pred frames into Y.
__global__ __launch_bounds__(256) void multires_window_pack_kernel(MrArgs a) {
  extern __shared__ _Float16 lds[];
  const int32_t b = blockIdx.y;
  const bool isY = blockIdx.z == 1;
  const int32_t frames = isY ? a.pred : a.obs;
  const int64_t first = isY ? a.obs : 0;
  void* out = isY ? a.Y : a.X;
  const int64_t out_b = (int64_t)b * (a.n_kept + a.n_reg) * frames * a.C;
  const int32_t bx = blockIdx.x;
  if (bx < a.n_gt) {
    const int32_t ty = bx / a.gt_lon, tx = bx - ty * a.gt_lon;
    pack_tile(a.gs, a.Tg, a.n_lon, a.n_lat, a.Ctg, a.rank, 0, tx * a.tile, ty * a.tile, a.t0[b] + a.off_g + first,
              frames, a, out, out_b, lds);
  } else if (a.rs) {
    const int32_t rb = bx - a.n_gt;
    const int32_t ty = rb / a.rt_lon, tx = rb - ty * a.rt_lon;
    pack_tile(a.rs, a.Tr, a.rn_lon, a.rn_lat, a.Ctr, nullptr, a.n_kept, tx * a.tile, ty * a.tile,
              a.t0[b] + a.off_r + first, frames, a, out, out_b, lds);
  } else {
    interp_rows((bx - a.n_gt) * kRegRows, a.t0[b] + a.off_g + first, frames, a, out, out_b);
  }
}

}  // namespace

extern "C" int gcl_multires_window_pack(const uint16_t* gseries, int64_t Tg, int32_t n_lon, int32_t n_lat, int32_t Ctg,
                                        const uint16_t* rseries, int64_t Tr, int32_t rn_lon, int32_t rn_lat,
                                        int32_t Ctr, const int32_t* rank, int32_t n_kept, int32_t n_reg,
                                        const int32_t* corner, const double* w, const int64_t* t0, int64_t off_g,
                                        int64_t off_r, const float* mean, const float* stdv, int32_t C, int32_t obs,
                                        int32_t pred, int32_t quantize, int32_t out_f16, void* X, void* Y, int32_t B,
                                        gcl_stream_t stream) {
  GCL_CHECK_ARG(gseries && rank && t0 && X, "multires_window_pack: null argument");
  GCL_CHECK_ARG(Tg > 0 && n_lon > 0 && n_lat > 0 && Ctg > 0 && C > 0 && C <= Ctg && obs > 0 && pred >= 0 && B > 0 &&
                    B <= 65535 && n_kept >= 0 && n_reg >= 0 && (int64_t)n_lon * n_lat < (1ll << 31) / 4 &&
                    n_kept <= (int64_t)n_lon * n_lat,
                "multires_window_pack: bad shape (T=%lld grid %dx%d C=%d of %d obs=%d pred=%d B=%d kept=%d reg=%d)",
                (long long)Tg, n_lon, n_lat, C, Ctg, obs, pred, B, n_kept, n_reg);
  GCL_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "multires_window_pack: mean and std go together");
  GCL_CHECK_ARG(pred == 0 || Y, "multires_window_pack: pred > 0 needs the Y buffer");
  if (rseries) {
    GCL_CHECK_ARG(Tr > 0 && rn_lon > 0 && rn_lat > 0 && C <= Ctr && (int64_t)rn_lon * rn_lat == n_reg,
                  "multires_window_pack: regional series %dx%d (C=%d) does not give the %d regional rows", rn_lon,
                  rn_lat, Ctr, n_reg);
  } else {
    GCL_CHECK_ARG(n_reg == 0 || (corner && w), "multires_window_pack: interpolate mode needs the corner tables");
  }
  const int maxf = obs > pred ? obs : pred;
  int tile = 16;  // LDS of a tile: tile^2 * frames * C halves, kept within 64 KiB
  while (tile > 1 && (int64_t)tile * tile * maxf * C * 2 > 65536) tile >>= 1;
  GCL_CHECK_ARG((int64_t)tile * tile * maxf * C * 2 <= 65536, "multires_window_pack: window of %d x %d values per point is too wide",
                maxf, C);
  MrArgs a;
  a.gs = (const _Float16*)gseries; a.Tg = Tg; a.n_lon = n_lon; a.n_lat = n_lat; a.Ctg = Ctg;
  a.rs = (const _Float16*)rseries; a.Tr = Tr; a.rn_lon = rn_lon; a.rn_lat = rn_lat; a.Ctr = Ctr;
  a.rank = rank; a.corner = corner; a.w = w; a.n_kept = n_kept; a.n_reg = n_reg;
  a.t0 = t0; a.off_g = off_g; a.off_r = off_r; a.mean = mean; a.stdv = stdv;
  a.C = C; a.obs = obs; a.pred = pred; a.quantize = quantize; a.out_f16 = out_f16; a.X = X; a.Y = Y;
  a.tile = tile;
  a.gt_lon = (int32_t)gcl::cdiv(n_lon, tile);
  a.n_gt = a.gt_lon * (int32_t)gcl::cdiv(n_lat, tile);
  a.rt_lon = rseries ? (int32_t)gcl::cdiv(rn_lon, tile) : 0;
  const int64_t n_rb = rseries ? (int64_t)a.rt_lon * gcl::cdiv(rn_lat, tile) : gcl::cdiv(n_reg, kRegRows);
  const size_t lds = (size_t)tile * tile * maxf * C * sizeof(_Float16);
  hipLaunchKernelGGL(multires_window_pack_kernel, dim3((unsigned)(a.n_gt + n_rb), (unsigned)B, pred > 0 ? 2 : 1),
                     dim3(256), lds, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
