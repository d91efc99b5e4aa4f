// The regional U-Net forecaster around its network (src/unet/predict.py and predict_v2.py, which differ in the model they
// build only): the window read from the fp16 series as a planar 2-D grid (src/data/dataloader_chunked.py:202-218 followed
// by Grid2DDataset.__getitem__, predict_v2.py:36-40) and one autoregressive step's carry-forward, window shift and scores
// (predict_v2.py:138-180), for B samples per launch.
//
// The series is [T, n_lon, n_lat, Ct] fp16 and the network's tensors are planar [.., H = n_lat, W = n_lon], so every read
// of a frame is a transpose: a pixel's channels are Ct adjacent halves, its right-hand neighbour is n_lat * Ct halves on.
// A block therefore owns a tile of kTW columns x kTH rows.  For one column the tile's (row, channel) values are ONE run of
// th * Ct contiguous halves of the frame; the block copies the tile's runs to LDS in 16-byte pieces wherever a whole piece
// lies inside the run (the first and last piece of a run one half at a time, a run starts at any 2-byte address) and then
// reads LDS in the output's order, so the planar side is written and read in full 128-byte rows.
//
// Planar accesses are float4 where W % 4 == 0 (every row of every plane then starts on a 16-byte boundary when the tensor
// does) and one float per lane otherwise; the choice, and with it the order of every sum, is a function of W alone.
//
// Scores: a block owns a chunk of consecutive tiles of one sample and four channels, one per wave (the tile of the series
// is staged per block: the frames are read once per four channels, from the L2 after the first).  Per channel the wave's
// lanes add their pixels in ascending order, the lanes are added by the fixed butterfly (gcl::wave_sum) and the tiles of
// the chunk in ascending order.  The chunk count is at most 64 and a function of (H, W) alone, so the second stage
// (gcl::wave_strided_sum) is one value per lane.  No atomics; a block reads and writes one sample only.
#include <atomic>

#include "colsum.h"
#include "common.h"

namespace {

std::atomic<int64_t> g_launches{0};

constexpr int kTW = 32;          // columns (w, the series' lon) of a tile: one 128-byte row of a plane
constexpr int kTH = 8;           // rows (h, the series' lat) of a tile
constexpr int kTileChunks = 64;  // chunks of tiles per sample: one per lane of the second stage
constexpr int kChanPerBlock = 4;  // channels of a block of the step kernels: one per wave
constexpr int kStepSums = 6;     // pass 1: se_phys, se_base_phys, se_norm, se_base_norm, sum out', sum g
constexpr int kAccSums = 3;      // pass 2: centred sum p^2, sum t^2, sum p t

// Halves between two columns' runs in LDS: even, and an odd number of dwords, so that the lanes of a row - consecutive
// columns - read different banks.
__host__ __device__ inline int span_pitch(int Ct) {
  const int p = (kTH * Ct + 1) & ~1;
  return (p >> 1) & 1 ? p : p + 2;
}

struct Tiling {
  int tiles_w, ntiles, tpc, nchunk;  // tiles per row of tiles, tiles, tiles per chunk, chunks
};
inline Tiling tiling_of(int H, int W) {
  Tiling t;
  t.tiles_w = (int)gcl::cdiv(W, kTW);
  t.ntiles = t.tiles_w * (int)gcl::cdiv(H, kTH);
  t.tpc = (int)gcl::cdiv(t.ntiles, kTileChunks);
  t.nchunk = (int)gcl::cdiv(t.ntiles, t.tpc);
  return t;
}

__device__ __forceinline__ float half_bits_to_float(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }

// (float(series value) - mean) / std: the loader's numpy operations (dataloader_chunked.py:210-214), each rounded once
__device__ __forceinline__ float zscore(uint16_t u, float m, float sd) { return (half_bits_to_float(u) - m) / sd; }

// The tile (columns w0 .. w0 + tw, rows h0 .. h0 + th) of one frame [W][H][Ct] -> lds[s * pitch + hl * Ct + ct] for
// column s of the tile.  Every thread of the 256-thread block calls it; the caller's barrier follows.
__device__ __forceinline__ void stage_tile(const uint16_t* __restrict__ frame, int H, int Ct, int w0, int tw, int h0, int th,
                                           int pitch, uint16_t* __restrict__ lds) {
  const int n = th * Ct;            // halves of a run
  const int nwin = (n + 14) >> 3;   // 16-byte windows a run can touch (it starts up to 7 halves into the first)
  for (int i = threadIdx.x; i < tw * nwin; i += 256) {
    const int s = i / nwin, j = i - s * nwin;
    const uint16_t* src = frame + ((int64_t)(w0 + s) * H + h0) * Ct;
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) & 15) >> 1);
    const int k0 = 8 * j - mis;  // the window's first half, counted from the run's start
    uint16_t* dst = lds + s * pitch;
    if (k0 >= 0 && k0 + 8 <= n) {
      union { uint4 q; uint16_t h[8]; } u;
      u.q = *reinterpret_cast<const uint4*>(src + k0);
#pragma unroll
      for (int m = 0; m < 8; ++m) dst[k0 + m] = u.h[m];
    } else {
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int k = k0 + m;
        if (k >= 0 && k < n) dst[k] = src[k];
      }
    }
  }
}

struct TileGeom {
  int w0, h0, tw, th, nq, per_c;  // nq: V-wide items per row of the tile; per_c: items per channel
};
template <int V>
__device__ __forceinline__ TileGeom tile_geom(int tile, int tiles_w, int H, int W) {
  TileGeom g;
  const int ty = tile / tiles_w, tx = tile - ty * tiles_w;
  g.w0 = tx * kTW, g.h0 = ty * kTH;
  g.tw = W - g.w0 < kTW ? W - g.w0 : kTW;
  g.th = H - g.h0 < kTH ? H - g.h0 : kTH;
  g.nq = (g.tw + V - 1) / V;  // V == 4: W % 4 == 0, so tw % 4 == 0
  g.per_c = g.th * g.nq;
  return g;
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = gcl::ld4(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
  if constexpr (V == 4) gcl::st4(p, make_float4(v[0], v[1], v[2], v[3]));
  else *p = v[0];
}

// X[b, o * C + c, h, w] of one (tile, frame o, sample b) per block
template <int V>
__global__ __launch_bounds__(256) void grid_window_pack_kernel(const uint16_t* __restrict__ series, int64_t T, int W, int H, int Ct,
                                                               const int64_t* __restrict__ t0, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, int C, int obs,
                                                               float* __restrict__ X, int tiles_w) {
  extern __shared__ __align__(16) uint16_t lds[];
  const int64_t b = blockIdx.z, o = blockIdx.y, HW = (int64_t)H * W;
  const TileGeom g = tile_geom<V>(blockIdx.x, tiles_w, H, W);
  const int64_t t = t0[b];
  const bool ok = t >= 0 && t + obs <= T;  // block-uniform; a window that leaves the series is an error made visible
  const int pitch = span_pitch(Ct);
  if (ok) stage_tile(series + (t + o) * HW * Ct, H, Ct, g.w0, g.tw, g.h0, g.th, pitch, lds);
  __syncthreads();
  float* planes = X + (b * obs + o) * C * HW + (int64_t)g.h0 * W + g.w0;
  for (int i = threadIdx.x; i < C * g.per_c; i += 256) {
    const int c = i / g.per_c, r = i - c * g.per_c, hl = r / g.nq, q = r - hl * g.nq;
    const float m = mean[c], sd = stdv[c];
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = ok ? zscore(lds[(q * V + e) * pitch + hl * Ct + c], m, sd) : __builtin_nanf("");
    store_v<V>(planes + c * HW + (int64_t)hl * W + q * V, v);
  }
}

struct StepArgs {
  const float* out;        // [B,C,H,W]
  const float* X;          // [B,obs*C,H,W]
  const uint16_t* series;  // [T,W,H,Ct]
  const int64_t* t0;
  const uint8_t* kind;     // [C]: 0 dynamic, 1 static, 2 forcing
  const float *mean, *stdv;
  float* Xn;               // [B,obs*C,H,W]
  float* pred;             // [B,C,H,W] or NULL
  double* part1;           // [B][C][kStepSums][nchunk]
  double* part2;           // [B][C][kAccSums][nchunk]
  int64_t T;
  int32_t W, H, Ct, C, obs, step;
  Tiling tl;
};

// The truth frame of sample b at this step, or -1 when the sample is skipped (block-uniform)
__device__ __forceinline__ int64_t truth_frame(const StepArgs& a, int64_t b) {
  const int64_t t = a.t0[b], tg = t + a.obs + a.step;
  return t >= 0 && tg < a.T ? tg : -1;
}

// Pass 1: carry-forward, shift, the four squared-error sums and the two field sums.  Block (chunk of tiles, sample, group
// of four channels): wave w owns channel 4 * group + w.
template <int V>
__global__ __launch_bounds__(256) void forecast_step_kernel(StepArgs a) {
  extern __shared__ __align__(16) uint16_t lds[];  // the truth tile, then the persistence tile
  const int64_t b = blockIdx.y, HW = (int64_t)a.H * a.W;
  const int64_t tg = truth_frame(a, b);
  if (tg < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, C = a.C, W = a.W;
  const int c = blockIdx.z * kChanPerBlock + (tid >> 6);  // wave-uniform
  const int pitch = span_pitch(a.Ct);
  uint16_t* lds_b = lds + kTW * pitch;
  const uint16_t* frame_g = a.series + tg * HW * a.Ct;
  const uint16_t* frame_b = a.series + (a.t0[b] + a.obs - 1) * HW * a.Ct;
  const float* Xb = a.X + b * a.obs * C * HW;
  float* Xnb = a.Xn + b * a.obs * C * HW;
  float m = 0.f, sd = 1.f;
  int kind = 0;
  const float* src = nullptr;
  if (c < C) {
    m = a.mean[c], sd = a.stdv[c], kind = a.kind[c];
    src = kind == 1 ? Xb + ((int64_t)(a.obs - 1) * C + c) * HW : a.out + (b * C + c) * HW;
  }
  double keep[kStepSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the channel over the block's tiles so far (every lane)
  const int tile_end = (blockIdx.x + 1) * a.tl.tpc < a.tl.ntiles ? (blockIdx.x + 1) * a.tl.tpc : a.tl.ntiles;
  for (int tile = blockIdx.x * a.tl.tpc; tile < tile_end; ++tile) {
    const TileGeom g = tile_geom<V>(tile, a.tl.tiles_w, a.H, W);
    stage_tile(frame_g, a.H, a.Ct, g.w0, g.tw, g.h0, g.th, pitch, lds);
    stage_tile(frame_b, a.H, a.Ct, g.w0, g.tw, g.h0, g.th, pitch, lds_b);
    __syncthreads();
    const int64_t origin = (int64_t)g.h0 * W + g.w0;
    // the shift (predict_v2.py:180): frames 1 .. obs-1 of X become frames 0 .. obs-2 of X_next; the channel groups deal
    // the shifted channels between them
    for (int ch = blockIdx.z; ch < (a.obs - 1) * C; ch += gridDim.z) {
      for (int i = tid; i < g.per_c; i += 256) {
        const int hl = i / g.nq, q = i - hl * g.nq;
        const int64_t at = ch * HW + origin + (int64_t)hl * W + q * V;
        float v[V];
        load_v<V>(Xb + C * HW + at, v);
        store_v<V>(Xnb + at, v);
      }
    }
    if (c < C) {
      double acc[kStepSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = lane; i < g.per_c; i += 64) {
        const int hl = i / g.nq, q = i - hl * g.nq;
        const int64_t at = origin + (int64_t)hl * W + q * V;
        float p[V];
        if (kind != 2) load_v<V>(src + at, p);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int k = (q * V + e) * pitch + hl * a.Ct + c;
          const float gt = zscore(lds[k], m, sd), bl = zscore(lds_b[k], m, sd);
          if (kind == 2) p[e] = gt;  // forcing: the truth's own value (predict_v2.py:145-148)
          // predict_v2.py:156-163: products, sums, differences and squares in float32, one by one
          const float pp = gcl::rounded(p[e] * sd) + m, gp = gcl::rounded(gt * sd) + m, bp = gcl::rounded(bl * sd) + m;
          const float d0 = pp - gp, d1 = bp - gp, d2 = p[e] - gt, d3 = bl - gt;
          acc[0] += (double)gcl::rounded(d0 * d0);
          acc[1] += (double)gcl::rounded(d1 * d1);
          acc[2] += (double)gcl::rounded(d2 * d2);
          acc[3] += (double)gcl::rounded(d3 * d3);
          acc[4] += (double)p[e];
          acc[5] += (double)gt;
        }
        store_v<V>(Xnb + ((int64_t)(a.obs - 1) * C + c) * HW + at, p);
        if (a.pred) store_v<V>(a.pred + (b * C + c) * HW + at, p);
      }
#pragma unroll
      for (int k = 0; k < kStepSums; ++k) keep[k] += gcl::wave_sum(acc[k]);
    }
    __syncthreads();  // the next tile overwrites LDS
  }
  if (c < C && lane == 0) {
#pragma unroll
    for (int k = 0; k < kStepSums; ++k) a.part1[((b * C + c) * kStepSums + k) * a.tl.nchunk + blockIdx.x] = keep[k];
  }
}

// Pass 2: the sums about the field means (predict_v2.py:166-171), out' read back from X_next's last frame; the blocks
// and waves of pass 1
template <int V>
__global__ __launch_bounds__(256) void forecast_acc_kernel(StepArgs a) {
  extern __shared__ __align__(16) uint16_t lds[];
  const int64_t b = blockIdx.y, HW = (int64_t)a.H * a.W;
  const int64_t tg = truth_frame(a, b);
  if (tg < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, C = a.C, W = a.W;
  const int c = blockIdx.z * kChanPerBlock + (tid >> 6);  // wave-uniform
  const int pitch = span_pitch(a.Ct);
  const uint16_t* frame_g = a.series + tg * HW * a.Ct;
  const float* last = a.Xn + ((b * a.obs + (a.obs - 1)) * C + (c < C ? c : 0)) * HW;
  float m = 0.f, sd = 1.f;
  double mean_p = 0.0, mean_g = 0.0;
  if (c < C) {  // every block of a (sample, channel) adds the chunks' field sums in the same order
    m = a.mean[c], sd = a.stdv[c];
    double S[2];
    gcl::wave_strided_sum<2>(a.part1 + ((b * C + c) * kStepSums + 4) * a.tl.nchunk, a.tl.nchunk, lane, S);
    mean_p = S[0] / (double)HW, mean_g = S[1] / (double)HW;
  }
  double keep[kAccSums] = {0.0, 0.0, 0.0};
  const int tile_end = (blockIdx.x + 1) * a.tl.tpc < a.tl.ntiles ? (blockIdx.x + 1) * a.tl.tpc : a.tl.ntiles;
  for (int tile = blockIdx.x * a.tl.tpc; tile < tile_end; ++tile) {
    const TileGeom g = tile_geom<V>(tile, a.tl.tiles_w, a.H, W);
    stage_tile(frame_g, a.H, a.Ct, g.w0, g.tw, g.h0, g.th, pitch, lds);
    __syncthreads();
    if (c < C) {
      const int64_t origin = (int64_t)g.h0 * W + g.w0;
      double acc[kAccSums] = {0.0, 0.0, 0.0};
      for (int i = lane; i < g.per_c; i += 64) {
        const int hl = i / g.nq, q = i - hl * g.nq;
        float p[V];
        load_v<V>(last + origin + (int64_t)hl * W + q * V, p);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double dp = (double)p[e] - mean_p;
          const double dg = (double)zscore(lds[(q * V + e) * pitch + hl * a.Ct + c], m, sd) - mean_g;
          acc[0] += gcl::rounded(dp * dp);
          acc[1] += gcl::rounded(dg * dg);
          acc[2] += gcl::rounded(dp * dg);
        }
      }
#pragma unroll
      for (int k = 0; k < kAccSums; ++k) keep[k] += gcl::wave_sum(acc[k]);
    }
    __syncthreads();
  }
  if (c < C && lane == 0) {
#pragma unroll
    for (int k = 0; k < kAccSums; ++k) a.part2[((b * C + c) * kAccSums + k) * a.tl.nchunk + blockIdx.x] = keep[k];
  }
}

// The state: one block per channel.  Its four waves reduce four samples' chunks at a time; thread 0 then adds the four
// samples to the state one after the other, so the batch is walked in order whatever B is.
__global__ __launch_bounds__(256) void forecast_state_kernel(StepArgs a, double* __restrict__ state, int64_t* __restrict__ acc_count,
                                                             int64_t* __restrict__ count, int B) {
  __shared__ double sums[4][5];  // per wave: the four squared-error sums and the correlation of its sample
  __shared__ int flags[4];       // bit 0: scored, bit 1: the correlation counts
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, C = a.C, nchunk = a.tl.nchunk;
  double* st = state + ((int64_t)a.step * C + c) * 5;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = st[k];
  }
  int64_t scored = 0, counted = 0;
  for (int64_t b0 = 0; b0 < B; b0 += 4) {
    const int64_t b = b0 + wave;
    int flag = 0;
    if (b < B && truth_frame(a, b) >= 0) {  // wave-uniform
      double S[4], Q[kAccSums];
      gcl::wave_strided_sum<4>(a.part1 + (b * C + c) * kStepSums * nchunk, nchunk, lane, S);
      gcl::wave_strided_sum<kAccSums>(a.part2 + (b * C + c) * kAccSums * nchunk, nchunk, lane, Q);
      const double pn = sqrt(Q[0]), tn = sqrt(Q[1]);
      const bool counts = pn > 1e-8 && tn > 1e-8;  // predict_v2.py:172; a NaN norm is not counted either
      flag = counts ? 3 : 1;
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sums[wave][k] = S[k];
        sums[wave][4] = counts ? Q[2] / gcl::rounded(pn * tn) : 0.0;
      }
    }
    if (lane == 0) flags[wave] = flag;
    __syncthreads();
    if (tid == 0) {
      for (int w = 0; w < 4; ++w) {
        if (!(flags[w] & 1)) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += sums[w][k];
        if (flags[w] & 2) v[4] += sums[w][4], ++counted;
        ++scored;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) st[k] = v[k];
    acc_count[(int64_t)a.step * C + c] += counted;
    if (c == 0) count[a.step] += scored * (int64_t)a.H * a.W;
  }
}

// dynamic LDS of `frames` staged tiles; 0 when it does not fit a CU
size_t tile_lds_bytes(int Ct, int frames) {
  const size_t bytes = (size_t)frames * kTW * span_pitch(Ct) * sizeof(uint16_t);
  return bytes <= (size_t)gcl::kLdsBytes ? bytes : 0;
}

}  // namespace

extern "C" {

int64_t gcl_unet_forecast_launches(void) { return g_launches.load(); }

int gcl_grid_window_pack(const uint16_t* series, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct, const int64_t* t0,
                         const float* mean, const float* stdv, int32_t C, int32_t obs, float* X, int32_t B,
                         gcl_stream_t stream) {
  GCL_CHECK_ARG(series && t0 && mean && stdv && X, "gcl_grid_window_pack: null pointer");
  GCL_CHECK_ARG(T >= 1 && n_lon >= 1 && n_lat >= 1 && C >= 1 && C <= Ct && obs >= 1 && obs <= 65535 && B >= 1 && B <= 65535 &&
                    (int64_t)n_lon * n_lat <= 0x7fffffff / 4,
                "gcl_grid_window_pack: T %lld, grid %d x %d, C %d of %d, obs %d, B %d", (long long)T, n_lon, n_lat, C, Ct, obs, B);
  const size_t lds = tile_lds_bytes(Ct, 1);
  GCL_CHECK_ARG(lds > 0, "gcl_grid_window_pack: %d stored channels do not fit a tile in LDS", Ct);
  const Tiling tl = tiling_of(n_lat, n_lon);
  const dim3 grid((unsigned)tl.ntiles, (unsigned)obs, (unsigned)B);
  const hipStream_t st = (hipStream_t)stream;
  if (n_lon % 4 == 0 && gcl::aligned16(X)) {
    if (lds > 64 * 1024) GCL_ENSURE_DYN_LDS(grid_window_pack_kernel<4>, lds);
    hipLaunchKernelGGL(grid_window_pack_kernel<4>, grid, dim3(256), lds, st, series, T, n_lon, n_lat, Ct, t0, mean, stdv, C, obs, X,
                       tl.tiles_w);
  } else {
    if (lds > 64 * 1024) GCL_ENSURE_DYN_LDS(grid_window_pack_kernel<1>, lds);
    hipLaunchKernelGGL(grid_window_pack_kernel<1>, grid, dim3(256), lds, st, series, T, n_lon, n_lat, Ct, t0, mean, stdv, C, obs, X,
                       tl.tiles_w);
  }
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

size_t gcl_grid_forecast_step_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || (int64_t)H * W > 0x7fffffff / 4) return 0;
  return (size_t)B * C * (kStepSums + kAccSums) * tiling_of(H, W).nchunk * sizeof(double);
}

int gcl_grid_forecast_step(const float* out, const float* X, const uint16_t* series, int64_t T, int32_t n_lon, int32_t n_lat,
                           int32_t Ct, const int64_t* t0, const uint8_t* chan_kind, const float* mean, const float* stdv,
                           int32_t C, int32_t obs, int32_t step, int32_t AR, float* X_next, float* pred, double* state,
                           int64_t* acc_count, int64_t* count, int32_t B, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(out && X && series && t0 && chan_kind && mean && stdv && X_next && state && acc_count && count && ws,
                "gcl_grid_forecast_step: null pointer");
  GCL_CHECK_ARG(T >= 1 && n_lon >= 1 && n_lat >= 1 && C >= 1 && C <= Ct && obs >= 1 && obs <= 4096 && B >= 1 && B <= 65535 &&
                    (int64_t)n_lon * n_lat <= 0x7fffffff / 4,
                "gcl_grid_forecast_step: T %lld, grid %d x %d, C %d of %d, obs %d, B %d", (long long)T, n_lon,
                n_lat, C, Ct, obs, B);
  GCL_CHECK_ARG(step >= 0 && step < AR, "gcl_grid_forecast_step: step %d of %d", step, AR);
  GCL_CHECK_ARG(X_next != X, "gcl_grid_forecast_step: X_next must not be X (ping-pong two buffers)");
  GCL_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gcl_grid_forecast_step: ws must be 8-byte aligned");
  const bool vec = n_lon % 4 == 0;
  GCL_CHECK_ARG(!vec || (gcl::aligned16(out) && gcl::aligned16(X) && gcl::aligned16(X_next) && (!pred || gcl::aligned16(pred))),
                "gcl_grid_forecast_step: with n_lon %% 4 == 0 out, X, X_next and pred must be 16-byte aligned");
  const size_t need = gcl_grid_forecast_step_ws_bytes(B, n_lat, n_lon, C);
  if (ws_bytes < need) {
    gcl::set_error("gcl_grid_forecast_step: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return GCL_ENOMEM;
  }
  const size_t lds2 = tile_lds_bytes(Ct, 2), lds1 = tile_lds_bytes(Ct, 1);
  GCL_CHECK_ARG(lds2 > 0, "gcl_grid_forecast_step: %d stored channels do not fit two tiles in LDS", Ct);
  StepArgs a{};
  a.out = out, a.X = X, a.series = series, a.t0 = t0, a.kind = chan_kind, a.mean = mean, a.stdv = stdv, a.Xn = X_next, a.pred = pred;
  a.T = T, a.W = n_lon, a.H = n_lat, a.Ct = Ct, a.C = C, a.obs = obs, a.step = step;
  a.tl = tiling_of(n_lat, n_lon);
  a.part1 = static_cast<double*>(ws);
  a.part2 = a.part1 + (size_t)B * C * kStepSums * a.tl.nchunk;
  const dim3 grid((unsigned)a.tl.nchunk, (unsigned)B, (unsigned)gcl::cdiv(C, kChanPerBlock));
  const hipStream_t st = (hipStream_t)stream;
  if (vec) {
    if (lds2 > 64 * 1024) GCL_ENSURE_DYN_LDS(forecast_step_kernel<4>, lds2);
    if (lds1 > 64 * 1024) GCL_ENSURE_DYN_LDS(forecast_acc_kernel<4>, lds1);
    hipLaunchKernelGGL(forecast_step_kernel<4>, grid, dim3(256), lds2, st, a);
    GCL_CHECK_LAUNCH();
    hipLaunchKernelGGL(forecast_acc_kernel<4>, grid, dim3(256), lds1, st, a);
  } else {
    if (lds2 > 64 * 1024) GCL_ENSURE_DYN_LDS(forecast_step_kernel<1>, lds2);
    if (lds1 > 64 * 1024) GCL_ENSURE_DYN_LDS(forecast_acc_kernel<1>, lds1);
    hipLaunchKernelGGL(forecast_step_kernel<1>, grid, dim3(256), lds2, st, a);
    GCL_CHECK_LAUNCH();
    hipLaunchKernelGGL(forecast_acc_kernel<1>, grid, dim3(256), lds1, st, a);
  }
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(forecast_state_kernel, dim3(C), dim3(256), 0, st, a, state, acc_count, count, B);
  GCL_CHECK_LAUNCH();
  g_launches += 3;
  return GCL_OK;
}

}  // extern "C"
