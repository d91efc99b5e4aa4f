// The data layer of the U-Net downscaler (gfx950): the (coarse, fine) pairs of scripts/build_downscaler_dataset.py, the
// archive of GNN predictions on the fine grid of scripts/generate_gnn_predictions.py, the batches of DownscalerDataset
// and the coarse baseline of compute_metrics (scripts/train_downscaler.py), all from the fp16 series in HBM.  No entry
// point allocates or synchronises; offsets are int64; no floating-point atomics; every reduction has a fixed order.
#include "common.h"

using gcl::load_span;
using gcl::rounded;
using gcl::store_span;
using gcl::wave_sum;

namespace {

constexpr int kStageBytes = 32768;  // LDS of one staged tile
constexpr int kBlocks = 2048;       // most blocks of a tiled or reducing kernel
constexpr int kTW = 32, kTH = 8;    // the (w, h) tile of the batch transpose
constexpr int kUnroll = 4;           // points a thread of the interpolating kernels has in flight
constexpr float kEps = 1e-8f;       // _normalize: (x - mean) / (std + 1e-8)

__device__ __forceinline__ float widen(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t half_bits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }

// float64 -> binary16 in ONE rounding (to nearest even, overflow to +-inf, subnormals kept), as
// ndarray.astype(np.float16) rounds a float64.  Rounding to float32 first rounds twice.  The float32 step here rounds to
// odd instead: the nearest-even float32 is moved one step towards zero when it lies beyond d, and its last bit is set
// whenever it is inexact; 24 bits against the 11 of binary16 leave the two guard bits that make the second rounding
// the only one that counts.
__device__ __forceinline__ uint16_t double_to_half(double d) {
  float f = (float)d;
  if (d == d) {
    const double back = (double)f;
    if (back != d) {
      uint32_t b = __builtin_bit_cast(uint32_t, f);
      if (__builtin_fabs(back) > __builtin_fabs(d)) b -= 1;  // f != 0 here; inf steps down to the largest float
      b |= 1u;
      f = __builtin_bit_cast(float, b);
    }
  }
  return half_bits(f);
}

// points of one staged tile: tile * C halves within kStageBytes, and small enough that `spans` spans of P points make
// a few hundred blocks (a batch of 8 predictions is 40 tiles of 512 points, a sixth of the CUs: a single call of 51 us
// against 17 us)
int tile_points(int32_t C, int64_t P, int64_t spans) {
  int tile = 512;
  while (tile > 32 && ((int64_t)tile * C * 2 > kStageBytes || gcl::cdiv(P, tile) * spans < 512)) tile >>= 1;
  return tile;
}

unsigned blocks_for(int64_t items) { return (unsigned)(items < kBlocks ? (items > 0 ? items : 1) : kBlocks); }

// ---- coarse: scripts/build_downscaler_dataset.py:137-157 (interpolation), :125-127 (the copy of fine.npy) ------------
struct CoarseArgs {
  const uint16_t* series;
  const int32_t* pos;
  const double* w;
  uint16_t* out;
  int64_t N, P, t0, to0, tiles_per_t, ntiles;
  int32_t C, tile;
};

// A block walks tiles of `tile` output points of one frame (tile = blockIdx.x, + gridDim.x, ..).  Thread tid forms
// channel tid % C of the points tid / C, + 256 / C, .. of the tile: consecutive threads read consecutive channels of
// the same four corner nodes.  The span goes through LDS and out by store_span (16-byte stores over the aligned
// body).  Without a table the frame's own halves are staged and stored: bits are moved, never converted.
__global__ __launch_bounds__(256) void downscale_coarse_kernel(CoarseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  // a thread keeps one channel: 256 / C whole points per pass, no division per value
  const int pstep = 256 / a.C, c = tid % a.C, pl0 = tid < pstep * a.C ? tid / a.C : a.tile;
  for (int64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const int64_t t = tl / a.tiles_per_t;
    const int64_t p0 = (tl - t * a.tiles_per_t) * a.tile;
    const int np = (int)((a.P - p0) < a.tile ? (a.P - p0) : a.tile);
    const int n = np * a.C;
    const uint16_t* __restrict__ frame = a.series + (a.t0 + t) * a.N * a.C;
    const uint16_t* __restrict__ fc = frame + c;
    if (a.pos == nullptr) {
      load_span<256>(frame + p0 * a.C, n, stage);
    } else {
      // kUnroll points per pass, every load of the pass issued before the first sum: the loop is a chain of two
      // dependent loads (table row, then corner values) and runs at their latency otherwise
      for (int pl = pl0; pl < np; pl += kUnroll * pstep) {  // (threads past the last whole point idle: pl0 >= tile)
        uint16_t h[kUnroll][4];
        double wv[kUnroll][4];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int q = pl + u * pstep;
          if (q < np) {
            const int32_t* pi = a.pos + (p0 + q) * 4;
            const double* wi = a.w + (p0 + q) * 4;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              h[u][m] = fc[(uint32_t)pi[m] * (uint32_t)a.C];
              wv[u][m] = wi[m];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int q = pl + u * pstep;
          if (q < np) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) acc = acc + rounded((double)widen(h[u][m]) * wv[u][m]);
            stage[q * a.C + c] = double_to_half(acc);
          }
        }
      }
    }
    __syncthreads();
    store_span<256>(a.out + ((a.to0 + t) * a.P + p0) * a.C, n, [&](int k) { return stage[k]; });
    __syncthreads();
  }
}

// ---- pred: scripts/generate_gnn_predictions.py:226-254 (residual, crop_and_upsample_roi :100-111, denormalise, store) -
struct PredArgs {
  const float* pred;
  const float* last;
  const int32_t* pos;
  const double* w;
  const float* stdv;
  const float* mean;
  const int64_t* dest;
  uint16_t* out;
  int64_t bs, gs, lbs, lgs, P, T_out, tiles_per_b, ntiles;
  int32_t C, tile;
};

// The tiling of downscale_coarse_kernel over (sample, tile); a sample whose destination lies outside the archive is
// skipped by the whole block.
__global__ __launch_bounds__(256) void downscale_pred_kernel(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  const int pstep = 256 / a.C, c = tid % a.C, pl0 = tid < pstep * a.C ? tid / a.C : a.tile;  // as in the coarse kernel
  const float sd = a.stdv[c], mu = a.mean[c];
  for (int64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const int64_t b = tl / a.tiles_per_b;
    const int64_t d = a.dest[b];
    if (d < 0 || d >= a.T_out) continue;
    const int64_t p0 = (tl - b * a.tiles_per_b) * a.tile;
    const int np = (int)((a.P - p0) < a.tile ? (a.P - p0) : a.tile);
    const int n = np * a.C;
    const float* __restrict__ x = a.pred + b * a.bs;
    const float* __restrict__ xl = a.last ? a.last + b * a.lbs : nullptr;
    for (int pl = pl0; pl < np; pl += kUnroll * pstep) {  // (loads first, as in the coarse kernel)
      float v[kUnroll][4], vl[kUnroll][4];
      double wv[kUnroll][4];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int q = pl + u * pstep;
        if (q < np) {
          const int32_t* pi = a.pos + (p0 + q) * 4;
          const double* wi = a.w + (p0 + q) * 4;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            v[u][m] = x[(int64_t)pi[m] * a.gs + c];
            vl[u][m] = xl ? xl[(int64_t)pi[m] * a.lgs + c] : 0.f;
            wv[u][m] = wi[m];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int q = pl + u * pstep;
        if (q < np) {
          double acc = 0.0;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float y = xl ? rounded(vl[u][m] + v[u][m]) : v[u][m];
            acc = acc + rounded((double)y * wv[u][m]);
          }
          float f = (float)acc;
          f = rounded(f * sd);
          f = rounded(f + mu);
          stage[q * a.C + c] = half_bits(f);
        }
      }
    }
    __syncthreads();
    store_span<256>(a.out + (d * a.P + p0) * a.C, n, [&](int k) { return stage[k]; });
    __syncthreads();
  }
}

// ---- batch: DownscalerDataset.__getitem__, scripts/train_downscaler.py:137-183 ---------------------------------------
struct BatchArgs {
  const uint16_t* coarse;
  const uint16_t* fine;
  const int64_t* t;
  const float* mean;
  const float* stdv;
  const float* stat;
  const int32_t* flip;
  const int32_t* neg;
  const float* noise;
  float* X;
  float* Y;
  int64_t T, nitems;
  int32_t W, H, C, obs, Ns, nf, ntw, nth;
  float sigma;
};

// An item is (sample, frame, h tile, w tile): frames 0 .. obs-1 the coarse frames t - obs + 1 .. t into X, frame obs the
// fine frame t into Y, frame obs + 1 the statics.  The archive is (w, h, c) with c fastest, the output (c, h, w) with w
// fastest: per w of the tile the thn * C halves of its h rows are one contiguous span, staged as they lie (rows
// kTH * C + 2 halves apart: an odd number of words, so the transposed read meets every bank once), then written w
// fastest - 128 contiguous bytes per (c, h).  The statics are small and come straight from L2.
__global__ __launch_bounds__(256) void downscale_batch_kernel(BatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  const int rs = kTH * a.C + 2;
  const int64_t HW = (int64_t)a.H * a.W;
  const int CX = a.obs * a.C + a.Ns;
  for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    int64_t q = item;
    const int wt = (int)(q % a.ntw); q /= a.ntw;
    const int ht = (int)(q % a.nth); q /= a.nth;
    const int f = (int)(q % a.nf);
    const int64_t b = q / a.nf;
    const int64_t tb = a.t[b];
    if (tb - a.obs + 1 < 0 || tb >= a.T) continue;  // (the whole block)
    const int w0 = wt * kTW, h0 = ht * kTH;
    const int twn = a.W - w0 < kTW ? a.W - w0 : kTW, thn = a.H - h0 < kTH ? a.H - h0 : kTH;
    const bool fl = a.flip != nullptr && a.flip[b] != 0;
    if (f > a.obs) {
      float* dst = a.X + (b * CX + (int64_t)a.obs * a.C) * HW;
      for (int e = tid; e < a.Ns * thn * twn; e += 256) {
        const int wl = e % twn, r = e / twn, hl = r % thn, s = r / thn;
        const int w = w0 + wl, h = h0 + hl;
        dst[(int64_t)s * HW + (int64_t)h * a.W + (fl ? a.W - 1 - w : w)] = a.stat[((int64_t)w * a.H + h) * a.Ns + s];
      }
      continue;
    }
    const bool isx = f < a.obs;
    const uint16_t* __restrict__ src = isx ? a.coarse + (tb - a.obs + 1 + f) * HW * a.C : a.fine + tb * HW * a.C;
    const int span = thn * a.C;
    for (int e = tid; e < twn * span; e += 256) {
      const int wl = e / span, r = e - wl * span;
      stage[wl * rs + r] = src[((int64_t)(w0 + wl) * a.H + h0) * a.C + r];
    }
    __syncthreads();
    float* dst = isx ? a.X + (b * CX + (int64_t)f * a.C) * HW : a.Y + b * a.C * HW;
    const float* nz = isx && a.noise ? a.noise + (b * a.obs + f) * a.C * HW : nullptr;
    for (int e = tid; e < a.C * thn * twn; e += 256) {
      const int wl = e % twn, r = e / twn, hl = r % thn, c = r / thn;
      float v = rounded(widen(stage[wl * rs + hl * a.C + c]) - a.mean[c]) / rounded(a.stdv[c] + kEps);
      if (fl && a.neg != nullptr && a.neg[c] != 0) v = -v;
      const int w = w0 + wl;
      const int64_t o = (int64_t)c * HW + (int64_t)(h0 + hl) * a.W + (fl ? a.W - 1 - w : w);
      if (nz) v = rounded(v + rounded(nz[o] * a.sigma));
      dst[o] = v;
    }
    __syncthreads();
  }
}

// ---- pair mse: the coarse baseline of compute_metrics, scripts/train_downscaler.py:288-305 ---------------------------
// Stage 1: an item is (listed frame, chunk of A elements), A the largest multiple of C within 256, so thread tid < A
// meets channel tid % C in every chunk and keeps one sum.  Items are dealt blockIdx.x, + gridDim.x, ..; at the end
// thread c < C folds the sums of its channel in thread order.  Stage 2: one wave per channel over the blocks' records,
// lane l taking l, l + 64, .., then the fixed butterfly.
__global__ __launch_bounds__(256) void downscale_pair_mse_kernel(const uint16_t* __restrict__ xa,
                                                                 const uint16_t* __restrict__ xb, int64_t T, int64_t FE,
                                                                 int32_t C, int32_t A, const int64_t* __restrict__ tl,
                                                                 int64_t chunks, int64_t nitems,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, double* part) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0, cnt = 0.0;
  if (tid < A) {
    const int c = tid % C;
    const float mu = mean[c], sd = rounded(stdv[c] + kEps);
    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
      const int64_t i = item / chunks, e = (item - i * chunks) * A + tid;
      const int64_t t = tl[i];
      if (t < 0 || t >= T || e >= FE) continue;
      const float va = rounded(widen(xa[t * FE + e]) - mu) / sd;
      const float vb = rounded(widen(xb[t * FE + e]) - mu) / sd;
      const float d = rounded(va - vb);
      s += rounded((double)d * (double)d);  // (exact: 24 x 24 bits)
      cnt += 1.0;
    }
  }
  for (int qty = 0; qty < 2; ++qty) {
    __syncthreads();
    red[tid] = qty == 0 ? cnt : s;
    __syncthreads();
    if (tid < C) {
      double r = red[tid];
      for (int i = tid + C; i < A; i += C) r += red[i];
      part[((int64_t)blockIdx.x * C + tid) * 2 + qty] = r;
    }
  }
}

__global__ __launch_bounds__(64) void downscale_pair_mse_reduce_kernel(const double* __restrict__ part, int nparts, int C,
                                                                       double* stats) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double n = 0.0, s = 0.0;
  for (int b = lane; b < nparts; b += 64) {
    n += part[((int64_t)b * C + c) * 2];
    s += part[((int64_t)b * C + c) * 2 + 1];
  }
  n = wave_sum(n);
  s = wave_sum(s);
  if (lane == 0) {
    stats[c * 2] = n;
    stats[c * 2 + 1] = s;
  }
}

bool even_address(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1) == 0; }

}  // namespace

extern "C" size_t gcl_downscale_ws_bytes(int32_t C) {
  return (size_t)kBlocks * (size_t)(C > 0 ? C : 1) * 2 * sizeof(double);
}

extern "C" int gcl_downscale_coarse(const uint16_t* series, int64_t T, int64_t N, int32_t C, const int32_t* pos,
                                    const double* w, int64_t P, int64_t t0, int64_t nt, uint16_t* out, int64_t T_out,
                                    int64_t to0, gcl_stream_t stream) {
  GCL_CHECK_ARG(series && out, "downscale_coarse: null argument");
  GCL_CHECK_ARG((pos == nullptr) == (w == nullptr), "downscale_coarse: the positions and the weights of a point table go together");
  GCL_CHECK_ARG(T > 0 && N > 0 && N < (1ll << 31) && C > 0 && C <= 256 && P > 0 && nt > 0 && t0 >= 0 && t0 + nt <= T &&
                    T_out > 0 && to0 >= 0 && to0 + nt <= T_out,
                "downscale_coarse: bad shape (N=%lld C=%d P=%lld frames [%lld, %lld) of %lld into [%lld, %lld) of %lld)",
                (long long)N, C, (long long)P, (long long)t0, (long long)(t0 + nt), (long long)T, (long long)to0,
                (long long)(to0 + nt), (long long)T_out);
  GCL_CHECK_ARG(N * C < (1ll << 32), "downscale_coarse: a frame of %lld halves (the kernel's offsets inside a frame are 32-bit)",
                (long long)(N * C));
  GCL_CHECK_ARG(pos != nullptr || P == N, "downscale_coarse: a copy takes whole frames (P=%lld, N=%lld)", (long long)P,
                (long long)N);
  GCL_CHECK_ARG(even_address(series) && even_address(out), "downscale_coarse: a buffer is not 2-byte aligned");
  GCL_CHECK_ARG(series != out, "downscale_coarse: in place is not possible");
  CoarseArgs a;
  a.series = series; a.pos = pos; a.w = w; a.out = out;
  a.N = N; a.P = P; a.t0 = t0; a.to0 = to0; a.C = C; a.tile = tile_points(C, P, nt);
  a.tiles_per_t = gcl::cdiv(P, a.tile);
  a.ntiles = a.tiles_per_t * nt;
  hipLaunchKernelGGL(downscale_coarse_kernel, dim3(blocks_for(a.ntiles)), dim3(256), (size_t)a.tile * C * sizeof(uint16_t),
                     (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_downscale_pred(const float* pred, int64_t bs, int64_t gs, const float* last, int64_t lbs, int64_t lgs,
                                  const int32_t* pos, const double* w, int64_t P, int32_t C, int32_t B, const float* stdv,
                                  const float* mean, const int64_t* dest, uint16_t* out, int64_t T_out,
                                  gcl_stream_t stream) {
  GCL_CHECK_ARG(pred && stdv && mean && dest && out, "downscale_pred: null argument");
  GCL_CHECK_ARG(pos && w, "downscale_pred: null point table (P=%lld)", (long long)P);
  GCL_CHECK_ARG(P > 0 && C > 0 && C <= 256 && B > 0 && T_out > 0 && gs >= C && bs >= 0 &&
                    (last == nullptr || (lgs >= C && lbs >= 0)),
                "downscale_pred: bad shape (P=%lld C=%d B=%d T_out=%lld strides %lld/%lld, %lld/%lld)", (long long)P, C, B,
                (long long)T_out, (long long)bs, (long long)gs, (long long)lbs, (long long)lgs);
  GCL_CHECK_ARG(even_address(out), "downscale_pred: the archive is not 2-byte aligned");
  PredArgs a;
  a.pred = pred; a.last = last; a.pos = pos; a.w = w; a.stdv = stdv; a.mean = mean; a.dest = dest; a.out = out;
  a.bs = bs; a.gs = gs; a.lbs = lbs; a.lgs = lgs; a.P = P; a.T_out = T_out; a.C = C; a.tile = tile_points(C, P, B);
  a.tiles_per_b = gcl::cdiv(P, a.tile);
  a.ntiles = a.tiles_per_b * B;
  hipLaunchKernelGGL(downscale_pred_kernel, dim3(blocks_for(a.ntiles)), dim3(256), (size_t)a.tile * C * sizeof(uint16_t),
                     (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_downscale_batch(const uint16_t* coarse, const uint16_t* fine, int64_t T, int32_t W, int32_t H, int32_t C,
                                   const int64_t* t, int32_t B, int32_t obs, const float* mean, const float* stdv,
                                   const float* stat, int32_t Ns, const int32_t* flip, const int32_t* neg,
                                   const float* noise, float sigma, float* X, float* Y, gcl_stream_t stream) {
  GCL_CHECK_ARG(coarse && fine && t && mean && stdv && X && Y, "downscale_batch: null argument");
  GCL_CHECK_ARG(T > 0 && W > 0 && H > 0 && C > 0 && C <= 64 && B > 0 && obs > 0 && obs <= T && Ns >= 0,
                "downscale_batch: bad shape (T=%lld grid %dx%d C=%d (1 .. 64) B=%d obs=%d Ns=%d)", (long long)T, W, H, C, B,
                obs, Ns);
  GCL_CHECK_ARG((Ns > 0) == (stat != nullptr), "downscale_batch: %d static channels and %s static field", Ns,
                stat ? "a" : "no");
  GCL_CHECK_ARG(even_address(coarse) && even_address(fine), "downscale_batch: an archive is not 2-byte aligned");
  BatchArgs a;
  a.coarse = coarse; a.fine = fine; a.t = t; a.mean = mean; a.stdv = stdv; a.stat = stat; a.flip = flip; a.neg = neg;
  a.noise = noise; a.X = X; a.Y = Y; a.T = T; a.W = W; a.H = H; a.C = C; a.obs = obs; a.Ns = Ns; a.sigma = sigma;
  a.nf = obs + 1 + (Ns > 0 ? 1 : 0);
  a.ntw = (int32_t)gcl::cdiv(W, kTW);
  a.nth = (int32_t)gcl::cdiv(H, kTH);
  a.nitems = (int64_t)B * a.nf * a.ntw * a.nth;
  const unsigned nb = (unsigned)(a.nitems < (1 << 16) ? a.nitems : (1 << 16));
  hipLaunchKernelGGL(downscale_batch_kernel, dim3(nb), dim3(256), (size_t)kTW * (kTH * C + 2) * sizeof(uint16_t),
                     (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_downscale_pair_mse(const uint16_t* xa, const uint16_t* xb, int64_t T, int64_t P, int32_t C,
                                      const int64_t* t, int32_t n, const float* mean, const float* stdv, double* stats,
                                      void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(xa && xb && t && mean && stdv && stats && ws, "downscale_pair_mse: null argument");
  GCL_CHECK_ARG(T > 0 && P > 0 && C > 0 && C <= 256 && n > 0, "downscale_pair_mse: bad shape (T=%lld P=%lld C=%d n=%d)",
                (long long)T, (long long)P, C, n);
  GCL_CHECK_ARG(even_address(xa) && even_address(xb), "downscale_pair_mse: an archive is not 2-byte aligned");
  const int A = 256 / C * C;
  const int64_t FE = P * C, chunks = gcl::cdiv(FE, A), nitems = chunks * n;
  const unsigned nb = blocks_for(nitems);
  GCL_CHECK_ARG(ws_bytes >= (size_t)nb * C * 2 * sizeof(double),
                "downscale_pair_mse: workspace of %zu bytes is too small (need %zu)", ws_bytes,
                (size_t)nb * C * 2 * sizeof(double));
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(downscale_pair_mse_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, xa, xb, T, FE, C, A, t, chunks,
                     nitems, mean, stdv, part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(downscale_pair_mse_reduce_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, part, (int)nb, C, stats);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
