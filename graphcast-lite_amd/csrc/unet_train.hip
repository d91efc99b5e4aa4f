// WeatherUNet training (src/unet/model.py:11-98 in .train()): BatchNorm on batch statistics, and the backward pass.
//
// Activations are channels-last [B,H,W,C] float32, so every per-channel sum is a column sum over n = B*H*W rows: they
// all run in float64 in the two-stage order of colsum.h (fixed chunks of rows, a function of n alone; then the chunks of
// a column in a fixed order).  No atomics; every sum's order is a function of the shapes alone.
//
// unet_wgrad_kernel: dW[co][ci][t] = sum over pixels of dZ[pixel][co] * in[pixel + tap t][ci], an implicit GEMM on
// v_mfma_f32_32x32x2_f32 with M = 32 output channels, N = 32 input channels and K = pixels.
//   block = 1 wave; it owns one (32 co, 32 ci) tile of dW for all nine taps - nine accumulator tiles, 144 registers - and
//   a chunk of consecutive 4 x 8 pixel tiles (numbered sample-major over the batch);
//   per pixel tile the 32 x 32 dZ tile and the 6 x 10 pixels (tile + one-pixel halo) of the 32 input channels are
//   staged in LDS, the input by the forward's own unet_src.h::stage_halo (zero outside the image, past Cin and past
//   Cout), then 16 k-steps of two pixels (lane half h supplies pixel 2 s + h) x 9 taps: the A operand is one
//   LDS word of the dZ tile, the B operand one word of the shifted input image - lanes 0 .. 31 read 32 consecutive
//   words, the two halves never conflict;
//   the chunk's partial tiles go to the workspace [chunk][Cout][Cin][9]; unet_wgrad_sum_kernel adds the chunks of an
//   element in ascending order in float64 and writes dW in torch's [Cout,Cin,3,3] layout.
// The chunking (wgrad_plan) is a function of (B, H, W, Cin, Cout) alone.
#include <atomic>

#include "colsum.h"
#include "common.h"
#include "mfma_io.h"
#include "unet_src.h"

namespace {

using gcl::mfma_io::d_row;
using gcl::mfma_io::f32x16;
using gcl::unet_src::gelu_erf;
using gcl::unet_src::kHP;
using gcl::unet_src::kHW;
using gcl::unet_src::kTH;
using gcl::unet_src::kTW;
using gcl::unet_src::lerp_of;
using gcl::unet_src::Lerp;
using gcl::unet_src::pool_take;
using gcl::unet_src::pool_takes;
using gcl::unet_src::Src;
using gcl::unet_src::stage_halo;

std::atomic<int64_t> g_launches{0};

constexpr int kTC = 32;                      // channels of a dW tile, each way
constexpr int kWgradBlocks = 1024;           // blocks a weight gradient aims at: one wave each, 4 SIMDs x 256 CUs
constexpr int kWgradMaxChunks = 256;         // bounds the workspace: at most 256 partial copies of dW

// d gelu(u) / du, erf form
__device__ __forceinline__ float dgelu_erf(float u) {
  return 0.5f * (1.f + erff(u * 0.70710678118654752440f)) + u * 0.39894228040143267794f * expf(-0.5f * u * u);
}

// ---------------------------------------------------------------------------------------------------------------------
// Column sums: part[(col * NS + s) * nchunk + chunk]
// ---------------------------------------------------------------------------------------------------------------------
// Stage 2 for a block of 256 = 32 columns x 8 row lanes (every thread calls it): row lane rl adds the chunks rl, rl + 8,
// .. of column col in ascending order, then every thread adds the eight lanes of its column in ascending order.
template <int NS>
__device__ __forceinline__ void chunks_to_sums(const double* __restrict__ part, int nchunk, bool live, int64_t col,
                                               double (&red)[NS][256], double (&S)[NS]) {
  const int tid = threadIdx.x, c = tid & (gcl::kColTile - 1), rl = tid / gcl::kColTile;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    double v = 0.0;
    if (live) {
      const double* p = part + (col * NS + s) * nchunk;
      for (int j = rl; j < nchunk; j += gcl::kRowLanes) v += p[j];
    }
    red[s][tid] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    double v = red[s][c];
    for (int l = 1; l < gcl::kRowLanes; ++l) v += red[s][c + l * gcl::kColTile];
    S[s] = v;
  }
}

// Stage 1 of the batch statistics: sum z and sum z^2 of a chunk of rows, 32 channels a block
__global__ __launch_bounds__(256) void bn_stats_part_kernel(const float* __restrict__ z, double* __restrict__ part, int n,
                                                            int C, int rows_per, int nchunk) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x, col = tid & (gcl::kColTile - 1), rl = tid / gcl::kColTile;
  const int c = blockIdx.y * gcl::kColTile + col;
  const int r0 = blockIdx.x * rows_per, r1 = (r0 + rows_per) < n ? (r0 + rows_per) : n;
  double acc[2] = {0.0, 0.0};
  if (c < C) {
    for (int r = r0 + rl; r < r1; r += gcl::kRowLanes) {
      const double v = (double)z[(int64_t)r * C + c];
      acc[0] += v;
      acc[1] += v * v;
    }
  }
  const bool writer = rl == 0 && c < C;
  double* dst = part + ((int64_t)(c < C ? c : 0) * 2) * nchunk + blockIdx.x;
  gcl::lanes_to_part<2, 256>(red, acc, tid, gcl::kRowLanes, gcl::kColTile, writer, dst, nchunk);
}

__global__ __launch_bounds__(256) void bn_stats_final_kernel(const double* __restrict__ part, int n, int C, int nchunk,
                                                             float eps, float momentum, float* __restrict__ mean,
                                                             float* __restrict__ invstd, float* running_mean,
                                                             float* running_var, int64_t* num_batches) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * gcl::kColTile + (tid & (gcl::kColTile - 1));
  double S[2];
  chunks_to_sums<2>(part, nchunk, c < C, c, red, S);
  if (tid < gcl::kColTile && c < C) {
    const double m = S[0] / (double)n;
    double var = S[1] / (double)n - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    const double mom = (double)momentum;
    if (running_mean) running_mean[c] = (float)((1.0 - mom) * (double)running_mean[c] + mom * m);
    if (running_var) running_var[c] = (float)((1.0 - mom) * (double)running_var[c] + mom * (var * (double)n / (double)(n - 1)));
  }
  if (blockIdx.x == 0 && tid == 0 && num_batches) *num_batches += 1;
}

// a = gelu(gamma * (z - mean) * invstd + beta), four channels an item
__global__ __launch_bounds__(256) void bn_gelu_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float* __restrict__ a, int C,
                                                      int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i * 4) % C);
    const float4 zv = gcl::ld4(z + i * 4), g = gcl::ld4(gamma + c), bt = gcl::ld4(beta + c), m = gcl::ld4(mean + c),
                 is = gcl::ld4(invstd + c);
    float4 o;
    o.x = gelu_erf(g.x * ((zv.x - m.x) * is.x) + bt.x);
    o.y = gelu_erf(g.y * ((zv.y - m.y) * is.y) + bt.y);
    o.z = gelu_erf(g.z * ((zv.z - m.z) * is.z) + bt.z);
    o.w = gelu_erf(g.w * ((zv.w - m.w) * is.w) + bt.w);
    gcl::st4(a + i * 4, o);
  }
}

// Stage 1 of the BatchNorm + GELU backward: S1 = sum g, S2 = sum g * xhat, g = dA * gelu'(gamma * xhat + beta)
__global__ __launch_bounds__(256) void bn_gelu_bwd_part_kernel(const float* __restrict__ z, const float* __restrict__ dA,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               double* __restrict__ part, int n, int C, int rows_per,
                                                               int nchunk) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x, col = tid & (gcl::kColTile - 1), rl = tid / gcl::kColTile;
  const int c = blockIdx.y * gcl::kColTile + col;
  const int r0 = blockIdx.x * rows_per, r1 = (r0 + rows_per) < n ? (r0 + rows_per) : n;
  double acc[2] = {0.0, 0.0};
  if (c < C) {
    const float g_ = gamma[c], bt = beta[c], m = mean[c], is = invstd[c];
    for (int r = r0 + rl; r < r1; r += gcl::kRowLanes) {
      const float xhat = (z[(int64_t)r * C + c] - m) * is;
      const float g = dA[(int64_t)r * C + c] * dgelu_erf(g_ * xhat + bt);
      acc[0] += (double)g;
      acc[1] += (double)g * (double)xhat;
    }
  }
  const bool writer = rl == 0 && c < C;
  double* dst = part + ((int64_t)(c < C ? c : 0) * 2) * nchunk + blockIdx.x;
  gcl::lanes_to_part<2, 256>(red, acc, tid, gcl::kRowLanes, gcl::kColTile, writer, dst, nchunk);
}

// Stage 2: dbeta = S1, dgamma = S2
__global__ __launch_bounds__(256) void bn_gelu_bwd_final_kernel(const double* __restrict__ part, int C, int nchunk,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * gcl::kColTile + (tid & (gcl::kColTile - 1));
  double S[2];
  chunks_to_sums<2>(part, nchunk, c < C, c, red, S);
  if (tid < gcl::kColTile && c < C) {
    dbeta[c] = (float)S[0];
    dgamma[c] = (float)S[1];
  }
}

// dZ = gamma * invstd * (g - S1 / n - xhat * S2 / n); dZ may be dA
__global__ __launch_bounds__(256) void bn_gelu_bwd_apply_kernel(const float* __restrict__ z, const float* dA,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                                float* dZ, float inv_n, int C, int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i * 4) % C);
    const float4 zv = gcl::ld4(z + i * 4), dv = gcl::ld4(dA + i * 4);
    const float4 g4 = gcl::ld4(gamma + c), b4 = gcl::ld4(beta + c), m4 = gcl::ld4(mean + c), i4 = gcl::ld4(invstd + c),
                 s1 = gcl::ld4(dbeta + c), s2 = gcl::ld4(dgamma + c);
    const float zz[4] = {zv.x, zv.y, zv.z, zv.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w},
                bb[4] = {b4.x, b4.y, b4.z, b4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w},
                a1[4] = {s1.x, s1.y, s1.z, s1.w}, a2[4] = {s2.x, s2.y, s2.z, s2.w};
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xhat = (zz[k] - mm[k]) * ii[k];
      const float g = dd[k] * dgelu_erf(gg[k] * xhat + bb[k]);
      o[k] = gg[k] * ii[k] * (g - a1[k] * inv_n - xhat * (a2[k] * inv_n));
    }
    gcl::st4(dZ + i * 4, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The output convolution's backward
// ---------------------------------------------------------------------------------------------------------------------
// dA[b,pix,f] = sum over c, ascending, of dY[b,c,pix] * w[c,f]: an item is a pixel and four features
__global__ __launch_bounds__(256) void out_bwd_data_kernel(const float* __restrict__ dY, const float* __restrict__ w,
                                                           float* __restrict__ dA, int64_t HW, int F, int Cout,
                                                           int64_t total4) {
  const int F4 = F / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int f = (int)(i % F4) * 4;
    const int64_t r = i / F4, b = r / HW, pix = r % HW;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < Cout; ++c) {
      const float d = dY[(b * Cout + c) * HW + pix];
      const float4 wv = gcl::ld4(w + (int64_t)c * F + f);
      acc.x = __builtin_fmaf(d, wv.x, acc.x);
      acc.y = __builtin_fmaf(d, wv.y, acc.y);
      acc.z = __builtin_fmaf(d, wv.z, acc.z);
      acc.w = __builtin_fmaf(d, wv.w, acc.w);
    }
    gcl::st4(dA + r * F + f, acc);
  }
}

// Stage 1: column j < Cout * F is dW[c = j / F][f = j % F] = sum dY[c] * a[f]; column Cout * F + c is db[c] = sum dY[c]
__global__ __launch_bounds__(256) void out_bwd_part_kernel(const float* __restrict__ dY, const float* __restrict__ a,
                                                           double* __restrict__ part, int n, int64_t HW, int F, int Cout,
                                                           int rows_per, int nchunk) {
  __shared__ double red[1][256];
  const int tid = threadIdx.x, col = tid & (gcl::kColTile - 1), rl = tid / gcl::kColTile;
  const int j = blockIdx.y * gcl::kColTile + col, ncols = Cout * F + Cout;
  const int r0 = blockIdx.x * rows_per, r1 = (r0 + rows_per) < n ? (r0 + rows_per) : n;
  double acc[1] = {0.0};
  if (j < ncols) {
    const bool bias = j >= Cout * F;
    const int c = bias ? j - Cout * F : j / F, f = bias ? 0 : j % F;
    for (int r = r0 + rl; r < r1; r += gcl::kRowLanes) {
      const int64_t b = r / HW, pix = r % HW;
      const double d = (double)dY[(b * Cout + c) * HW + pix];
      acc[0] += bias ? d : d * (double)a[(int64_t)r * F + f];
    }
  }
  const bool writer = rl == 0 && j < ncols;
  double* dst = part + (int64_t)(j < ncols ? j : 0) * nchunk + blockIdx.x;
  gcl::lanes_to_part<1, 256>(red, acc, tid, gcl::kRowLanes, gcl::kColTile, writer, dst, nchunk);
}

__global__ __launch_bounds__(256) void out_bwd_final_kernel(const double* __restrict__ part, int nchunk, int nw, int nb,
                                                            float* __restrict__ dW, float* __restrict__ db) {
  __shared__ double red[1][256];
  const int tid = threadIdx.x;
  const int j = blockIdx.x * gcl::kColTile + (tid & (gcl::kColTile - 1));
  double S[1];
  chunks_to_sums<1>(part, nchunk, j < nw + nb, j, red, S);
  if (tid < gcl::kColTile && j < nw + nb) {
    if (j < nw) dW[j] = (float)S[0];
    else db[j - nw] = (float)S[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Routing a data gradient back through the source kind: every output element is written exactly once
// ---------------------------------------------------------------------------------------------------------------------
// dA[b,y,x,c] = skip[b,y,x,c] + (pixel is its window's argmax ? dP[b,y/2,x/2,c] : 0); the argmax is recomputed from the
// saved activation by torch's scan (row-major, pool_take)
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ act, const float* __restrict__ dP,
                                                       const float* __restrict__ skip, int64_t skip_ld,
                                                       float* __restrict__ dA, int Hs, int Ws, int C, int64_t total4) {
  const int C4 = C / 4, Hp = Hs / 2, Wp = Ws / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const int64_t r = i / C4;  // (b, y, x)
    const int x = (int)(r % Ws), y = (int)((r / Ws) % Hs);
    const int64_t b = r / ((int64_t)Ws * Hs);
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if ((y >> 1) < Hp && (x >> 1) < Wp) {
      const float* p = act + ((b * Hs + (y & ~1)) * Ws + (x & ~1)) * C + c;
      const int64_t row = (int64_t)Ws * C;
      const float4 v00 = gcl::ld4(p), v01 = gcl::ld4(p + C), v10 = gcl::ld4(p + row), v11 = gcl::ld4(p + row + C);
      const float4 d = gcl::ld4(dP + ((b * Hp + (y >> 1)) * Wp + (x >> 1)) * C + c);
      const float w0[4] = {v00.x, v00.y, v00.z, v00.w}, w1[4] = {v01.x, v01.y, v01.z, v01.w},
                  w2[4] = {v10.x, v10.y, v10.z, v10.w}, w3[4] = {v11.x, v11.y, v11.z, v11.w}, dd[4] = {d.x, d.y, d.z, d.w};
      const int own = (y & 1) * 2 + (x & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float win[4] = {w0[k], w1[k], w2[k], w3[k]};
        float m = -INFINITY;
        int arg = 0;  // (nothing taken, four -inf: torch keeps the first)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          arg = pool_takes(m, win[q]) ? q : arg;
          m = pool_take(m, win[q]);
        }
        t[k] = arg == own ? dd[k] : 0.f;
      }
    }
    if (skip) {
      const float4 s = gcl::ld4(skip + r * skip_ld + c);
      t[0] = s.x + t[0], t[1] = s.y + t[1], t[2] = s.z + t[2], t[3] = s.w + t[3];
    }
    gcl::st4(dA + r * C + c, make_float4(t[0], t[1], t[2], t[3]));
  }
}

// The adjoint of the bilinear align_corners=True read plus the zero pad, in gather form: a low-resolution element adds
// the contributions of the high-resolution pixels below (2 Hs, 2 Ws) that read it, in ascending (y, x) order
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ d, int64_t ld, int c_off,
                                                           float* __restrict__ dlow, int H, int W, int Hs, int Ws, int C2,
                                                           float sy, float sx, int64_t total4) {
  const int C4 = C2 / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const int64_t r = i / C4;
    const int xs = (int)(r % Ws), ys = (int)((r / Ws) % Hs);
    const int64_t b = r / ((int64_t)Ws * Hs);
    // candidates: floor(s * dst) in {ys - 1, ys}; the window is generous and every candidate is tested by the read's rule
    int ylo = 0, yhi = 2 * Hs - 1, xlo = 0, xhi = 2 * Ws - 1;
    if (sy > 0.f) {
      const int lo = (int)((float)(ys - 1) / sy) - 2, hi = (int)((float)(ys + 1) / sy) + 2;
      ylo = lo > ylo ? lo : ylo, yhi = hi < yhi ? hi : yhi;
    }
    if (sx > 0.f) {
      const int lo = (int)((float)(xs - 1) / sx) - 2, hi = (int)((float)(xs + 1) / sx) + 2;
      xlo = lo > xlo ? lo : xlo, xhi = hi < xhi ? hi : xhi;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int y = ylo; y <= yhi; ++y) {
      const Lerp ly = lerp_of(sy, y, Hs);
      const float wy = (ly.i0 == ys ? ly.h : 0.f) + (ly.i1 == ys ? ly.l : 0.f);
      if (ly.i0 != ys && ly.i1 != ys) continue;
      for (int x = xlo; x <= xhi; ++x) {
        const Lerp lx = lerp_of(sx, x, Ws);
        if (lx.i0 != xs && lx.i1 != xs) continue;
        const float wx = (lx.i0 == xs ? lx.h : 0.f) + (lx.i1 == xs ? lx.l : 0.f);
        const float wgt = wy * wx;
        const float4 g = gcl::ld4(d + ((b * H + y) * W + x) * ld + c_off + c);
        acc.x = __builtin_fmaf(wgt, g.x, acc.x);
        acc.y = __builtin_fmaf(wgt, g.y, acc.y);
        acc.z = __builtin_fmaf(wgt, g.z, acc.z);
        acc.w = __builtin_fmaf(wgt, g.w, acc.w);
      }
    }
    gcl::st4(dlow + r * C2 + c, acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient: the forward kernel on the transposed, tap-flipped weight
// ---------------------------------------------------------------------------------------------------------------------
// The record order of unet_pack_kernel for w'[ci][co][t] = w[co][ci][8 - t] (Cout' = Cin, Cin' = Cout):
// packed[(((nt * 9 + t) * G + g) * 64 + lane) * 4 + q] = w[co = 8 g + 4 (lane >> 5) + q][ci = 32 nt + (lane & 31)][8 - t]
__global__ __launch_bounds__(256) void pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ packed, int Cin,
                                                         int Cout, int G, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & 3), lane = (int)((i >> 2) & 63);
    int64_t r = i >> 8;
    const int g = (int)(r % G);
    r /= G;
    const int t = (int)(r % 9), nt = (int)(r / 9);
    const int ci = 32 * nt + (lane & 31), co = 8 * g + 4 * (lane >> 5) + q;
    packed[i] = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * 9 + (8 - t)] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient
// ---------------------------------------------------------------------------------------------------------------------
struct WgradPlan {
  int TX, T, NT, tpc, nchunk, NCo, NCi;  // tiles across, per sample, in all; tiles per chunk; chunks; channel tiles
  int64_t elems;                         // Cout * Cin * 9
};
// The one place that decides the pixel split; the size query and the launcher both read it.  A function of the shape.
bool wgrad_plan(int B, int H, int W, int Cin, int Cout, WgradPlan& p) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 4 || Cout % 4) return false;
  p.TX = (int)gcl::cdiv(W, kTW);
  p.T = (int)gcl::cdiv(H, kTH) * p.TX;
  const int64_t nt = (int64_t)B * p.T;
  if (nt > 0x7fffffff) return false;
  p.NT = (int)nt;
  p.NCo = (int)gcl::cdiv(Cout, kTC), p.NCi = (int)gcl::cdiv(Cin, kTC);
  int64_t want = gcl::cdiv(kWgradBlocks, (int64_t)p.NCo * p.NCi);
  want = want > kWgradMaxChunks ? kWgradMaxChunks : want;
  want = want > p.NT ? p.NT : want;
  p.tpc = (int)gcl::cdiv(p.NT, want);
  p.nchunk = (int)gcl::cdiv(p.NT, p.tpc);
  p.elems = (int64_t)Cout * Cin * 9;
  return (int64_t)p.NCo * p.NCi <= 0x7fffffff;
}

struct WgradArgs {
  Src src;
  const float* dz;
  float* part;
  int32_t Cout, TX, T, NT, tpc, NCi;
};

template <int KIND, int V>
__global__ __launch_bounds__(64) void unet_wgrad_kernel(const WgradArgs s) {
  __shared__ __align__(16) float Zs[32 * kTC];
  __shared__ __align__(16) float Xs[kHP * kTC];
  const int lane = threadIdx.x;
  const int cit = blockIdx.x % s.NCi, cot = blockIdx.x / s.NCi;
  const int chunk = blockIdx.y;
  const int j = lane & 31, h = lane >> 5;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  }

  const int g0 = chunk * s.tpc, g1 = (g0 + s.tpc) < s.NT ? (g0 + s.tpc) : s.NT;
  for (int g = g0; g < g1; ++g) {
    const int64_t b = g / s.T;
    const int tile = g % s.T;
    const int y0 = (tile / s.TX) * kTH, x0 = (tile % s.TX) * kTW;
    // the dZ tile: 32 pixels x 32 output channels (Cout % 4 == 0: four channels are inside or outside together)
    for (int idx = lane; idx < 32 * (kTC / 4); idx += 64) {
      const int p = idx >> 3, cc = (idx & 7) * 4;
      const int y = y0 + (p >> 3), x = x0 + (p & 7), co = cot * kTC + cc;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y < s.src.H && x < s.src.W && co < s.Cout) v = gcl::ld4(s.dz + ((b * s.src.H + y) * s.src.W + x) * s.Cout + co);
      gcl::st4(Zs + p * kTC + cc, v);
    }
    // the input image: 60 pixels x 32 input channels through the source kind
    stage_halo<KIND, V, 64>(Xs, kTC, s.src, b, y0, x0, cit * kTC, kTC, lane);
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int py = st >> 2, px = 2 * (st & 3);  // lane half h: pixel (py, px + h)
      const float av = Zs[(py * kTW + px + h) * kTC + j];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float bv = Xs[((py + t / 3) * kHW + px + h + t % 3) * kTC + j];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const int ci = cit * kTC + j;
  float* out = s.part + (int64_t)chunk * s.Cout * s.src.Cin * 9;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = cot * kTC + d_row(r, lane);
    if (co < s.Cout && ci < s.src.Cin) {
      float* o = out + ((int64_t)co * s.src.Cin + ci) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) o[t] = acc[t][r];
    }
  }
}

// dW[e] = the chunks' partial values of e, added in ascending chunk order in float64
__global__ __launch_bounds__(256) void unet_wgrad_sum_kernel(const float* __restrict__ part, float* __restrict__ dW,
                                                             int64_t elems, int nchunk) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < elems; e += (int64_t)gridDim.x * 256) {
    double v = 0.0;
    for (int k = 0; k < nchunk; ++k) v += (double)part[(int64_t)k * elems + e];
    dW[e] = (float)v;
  }
}

template <int KIND>
void launch_wgrad(const WgradArgs& a, bool vec, dim3 grid, hipStream_t st) {
  if constexpr (KIND != GCL_UNET_SRC_PLANAR) {
    if (vec) {
      hipLaunchKernelGGL((unet_wgrad_kernel<KIND, 4>), grid, dim3(64), 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((unet_wgrad_kernel<KIND, 1>), grid, dim3(64), 0, st, a);
}

bool rows_ok(int64_t n) { return n >= 1 && n <= 0x7fffffff; }
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" {

int64_t gcl_unet_train_launches(void) { return g_launches.load(); }

size_t gcl_unet_colsum_ws_bytes(int64_t n, int64_t ncols) {
  if (!rows_ok(n) || ncols < 1) return 0;
  return (size_t)ncols * gcl::num_chunks((int)n) * sizeof(double);
}

int gcl_unet_bn_stats(const float* z, int64_t n, int32_t C, float eps, float momentum, float* mean, float* invstd,
                      float* running_mean, float* running_var, int64_t* num_batches, void* ws, size_t ws_bytes,
                      gcl_stream_t stream) {
  GCL_CHECK_ARG(z && mean && invstd && ws, "gcl_unet_bn_stats: null pointer");
  GCL_CHECK_ARG(rows_ok(n) && C >= 1, "gcl_unet_bn_stats: n %lld, C %d", (long long)n, C);
  GCL_CHECK_ARG(n >= 2, "gcl_unet_bn_stats: more than 1 value per channel is needed in training, got n = %lld", (long long)n);
  GCL_CHECK_ARG(aligned8(ws), "gcl_unet_bn_stats: ws must be 8-byte aligned");
  const size_t need = gcl_unet_colsum_ws_bytes(n, 2 * (int64_t)C);
  if (ws_bytes < need) {
    gcl::set_error("gcl_unet_bn_stats: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return GCL_ENOMEM;
  }
  const int rows_per = gcl::chunk_rows((int)n), nchunk = gcl::num_chunks((int)n);
  const unsigned ct = (unsigned)gcl::cdiv(C, gcl::kColTile);
  const hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(bn_stats_part_kernel, dim3(nchunk, ct), dim3(256), 0, st, z, part, (int)n, C, rows_per, nchunk);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(ct), dim3(256), 0, st, part, (int)n, C, nchunk, eps, momentum, mean, invstd,
                     running_mean, running_var, num_batches);
  GCL_CHECK_LAUNCH();
  g_launches += 2;
  return GCL_OK;
}

int gcl_unet_bn_gelu(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd, float* a,
                     int64_t n, int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(z && gamma && beta && mean && invstd && a, "gcl_unet_bn_gelu: null pointer");
  GCL_CHECK_ARG(rows_ok(n) && C >= 4 && C % 4 == 0, "gcl_unet_bn_gelu: n %lld, C %d (a multiple of 4)", (long long)n, C);
  GCL_CHECK_ARG(gcl::aligned16(z) && gcl::aligned16(a) && gcl::aligned16(gamma) && gcl::aligned16(beta) &&
                    gcl::aligned16(mean) && gcl::aligned16(invstd),
                "gcl_unet_bn_gelu: every tensor must be 16-byte aligned");
  const int64_t total4 = n * C / 4;
  hipLaunchKernelGGL(bn_gelu_kernel, dim3(gcl::grid_for(total4, 1 << 16)), dim3(256), 0, (hipStream_t)stream, z, gamma, beta,
                     mean, invstd, a, C, total4);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_bn_gelu_bwd(const float* z, const float* dA, const float* gamma, const float* beta, const float* mean,
                         const float* invstd, float* dZ, float* dgamma, float* dbeta, int64_t n, int32_t C, void* ws,
                         size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(z && dA && gamma && beta && mean && invstd && dZ && dgamma && dbeta && ws, "gcl_unet_bn_gelu_bwd: null pointer");
  GCL_CHECK_ARG(rows_ok(n) && n >= 2 && C >= 4 && C % 4 == 0, "gcl_unet_bn_gelu_bwd: n %lld (at least 2), C %d (a multiple of 4)",
                (long long)n, C);
  GCL_CHECK_ARG(gcl::aligned16(z) && gcl::aligned16(dA) && gcl::aligned16(dZ) && gcl::aligned16(gamma) && gcl::aligned16(beta) &&
                    gcl::aligned16(mean) && gcl::aligned16(invstd) && gcl::aligned16(dgamma) && gcl::aligned16(dbeta),
                "gcl_unet_bn_gelu_bwd: every tensor must be 16-byte aligned");
  GCL_CHECK_ARG(aligned8(ws), "gcl_unet_bn_gelu_bwd: ws must be 8-byte aligned");
  const size_t need = gcl_unet_colsum_ws_bytes(n, 2 * (int64_t)C);
  if (ws_bytes < need) {
    gcl::set_error("gcl_unet_bn_gelu_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return GCL_ENOMEM;
  }
  const int rows_per = gcl::chunk_rows((int)n), nchunk = gcl::num_chunks((int)n);
  const unsigned ct = (unsigned)gcl::cdiv(C, gcl::kColTile);
  const hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(bn_gelu_bwd_part_kernel, dim3(nchunk, ct), dim3(256), 0, st, z, dA, gamma, beta, mean, invstd, part, (int)n,
                     C, rows_per, nchunk);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_gelu_bwd_final_kernel, dim3(ct), dim3(256), 0, st, part, C, nchunk, dgamma, dbeta);
  GCL_CHECK_LAUNCH();
  const int64_t total4 = n * C / 4;
  hipLaunchKernelGGL(bn_gelu_bwd_apply_kernel, dim3(gcl::grid_for(total4, 1 << 16)), dim3(256), 0, st, z, dA, gamma, beta, mean,
                     invstd, dgamma, dbeta, dZ, 1.f / (float)n, C, total4);
  GCL_CHECK_LAUNCH();
  g_launches += 3;
  return GCL_OK;
}

int32_t gcl_unet_wgrad_chunks(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
  WgradPlan p;
  return wgrad_plan(B, H, W, Cin, Cout, p) ? p.nchunk : 0;
}

size_t gcl_unet_wgrad_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
  WgradPlan p;
  return wgrad_plan(B, H, W, Cin, Cout, p) ? (size_t)p.nchunk * p.elems * sizeof(float) : 0;
}

int gcl_unet_conv3x3_wgrad(const gcl_unet_src_t* src, const float* dZ, float* dW, int32_t B, int32_t H, int32_t W,
                           int32_t Cin, int32_t Cout, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(dZ && dW && ws, "gcl_unet_conv3x3_wgrad: null pointer");
  WgradPlan p;
  GCL_CHECK_ARG(wgrad_plan(B, H, W, Cin, Cout, p),
                "gcl_unet_conv3x3_wgrad: B %d, H %d, W %d, Cin %d, Cout %d (Cout must be a multiple of 4)", B, H, W, Cin, Cout);
  GCL_CHECK_ARG(gcl::aligned16(dZ) && gcl::aligned16(ws), "gcl_unet_conv3x3_wgrad: dZ and ws must be 16-byte aligned");
  const size_t need = (size_t)p.nchunk * p.elems * sizeof(float);
  if (ws_bytes < need) {
    gcl::set_error("gcl_unet_conv3x3_wgrad: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return GCL_ENOMEM;
  }
  WgradArgs a{};
  bool vec;
  if (const int rc = gcl::unet_src::bind(src, H, W, Cin, "gcl_unet_conv3x3_wgrad", a.src, vec)) return rc;
  a.dz = dZ, a.part = static_cast<float*>(ws);
  a.Cout = Cout, a.TX = p.TX, a.T = p.T, a.NT = p.NT, a.tpc = p.tpc, a.NCi = p.NCi;
  const dim3 grid((unsigned)(p.NCo * p.NCi), (unsigned)p.nchunk);
  const hipStream_t st = (hipStream_t)stream;
  const int rc = gcl::unet_src::with_kind(src->kind, [&](auto K) {
    launch_wgrad<decltype(K)::value>(a, vec, grid, st);
    return GCL_OK;
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(unet_wgrad_sum_kernel, dim3(gcl::grid_for(p.elems)), dim3(256), 0, st, a.part, dW, p.elems, p.nchunk);
  GCL_CHECK_LAUNCH();
  g_launches += 2;
  return GCL_OK;
}

int gcl_unet_pack_weights_dgrad(const float* w, int32_t Cin, int32_t Cout, float* packed, gcl_stream_t stream) {
  GCL_CHECK_ARG(w && packed, "gcl_unet_pack_weights_dgrad: null pointer");
  GCL_CHECK_ARG(Cin >= 1 && Cout >= 1, "gcl_unet_pack_weights_dgrad: Cin %d, Cout %d", Cin, Cout);
  const int64_t total = gcl_unet_packed_floats(Cout, Cin);  // the transposed convolution: Cin' = Cout, Cout' = Cin
  hipLaunchKernelGGL(pack_dgrad_kernel, dim3(gcl::grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, packed, Cin, Cout,
                     (int)gcl::cdiv(Cout, 8), total);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_pool_bwd(const float* act, const float* dpooled, const float* skip, int64_t skip_ld, float* dA, int32_t B,
                      int32_t Hs, int32_t Ws, int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(act && dpooled && dA, "gcl_unet_pool_bwd: null pointer");
  GCL_CHECK_ARG(B >= 1 && Hs >= 2 && Ws >= 2 && C >= 4 && C % 4 == 0, "gcl_unet_pool_bwd: B %d, Hs %d, Ws %d, C %d (a multiple of 4)",
                B, Hs, Ws, C);
  GCL_CHECK_ARG(!skip || (skip_ld >= C && skip_ld % 4 == 0), "gcl_unet_pool_bwd: skip rows of %lld floats for %d channels",
                (long long)skip_ld, C);
  GCL_CHECK_ARG(gcl::aligned16(act) && gcl::aligned16(dpooled) && gcl::aligned16(dA) && gcl::aligned16(skip),
                "gcl_unet_pool_bwd: every tensor must be 16-byte aligned");
  const int64_t total4 = (int64_t)B * Hs * Ws * (C / 4);
  hipLaunchKernelGGL(pool_bwd_kernel, dim3(gcl::grid_for(total4, 1 << 16)), dim3(256), 0, (hipStream_t)stream, act, dpooled, skip,
                     skip_ld, dA, Hs, Ws, C, total4);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_upsample_bwd(const float* d, int64_t ld, int32_t c_off, float* dlow, int32_t B, int32_t H, int32_t W, int32_t Hs,
                          int32_t Ws, int32_t C2, gcl_stream_t stream) {
  GCL_CHECK_ARG(d && dlow, "gcl_unet_upsample_bwd: null pointer");
  GCL_CHECK_ARG(B >= 1 && Hs >= 1 && Ws >= 1 && 2 * Hs <= H && 2 * Ws <= W && C2 >= 4 && C2 % 4 == 0,
                "gcl_unet_upsample_bwd: B %d, low %d x %d in %d x %d, C2 %d (a multiple of 4)", B, Hs, Ws, H, W, C2);
  GCL_CHECK_ARG(c_off >= 0 && c_off % 4 == 0 && ld >= (int64_t)c_off + C2 && ld % 4 == 0,
                "gcl_unet_upsample_bwd: channels %d .. %d of rows of %lld floats", c_off, c_off + C2, (long long)ld);
  GCL_CHECK_ARG(gcl::aligned16(d) && gcl::aligned16(dlow), "gcl_unet_upsample_bwd: d and dlow must be 16-byte aligned");
  const int64_t total4 = (int64_t)B * Hs * Ws * (C2 / 4);
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3(gcl::grid_for(total4, 1 << 16)), dim3(256), 0, (hipStream_t)stream, d, ld, c_off,
                     dlow, H, W, Hs, Ws, C2, gcl::unet_src::upcat_scale(Hs), gcl::unet_src::upcat_scale(Ws), total4);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

size_t gcl_unet_conv1x1_out_bwd_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t F, int32_t Cout) {
  if (B < 1 || H < 1 || W < 1 || F < 1 || Cout < 1) return 0;
  return gcl_unet_colsum_ws_bytes((int64_t)B * H * W, (int64_t)Cout * F + Cout);
}

int gcl_unet_conv1x1_out_bwd(const float* dY, const float* a, const float* w, float* dA, float* dW, float* db, int32_t B,
                             int32_t H, int32_t W, int32_t F, int32_t Cout, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(dY && a && w && dA && dW && db && ws, "gcl_unet_conv1x1_out_bwd: null pointer");
  GCL_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && F >= 4 && F % 4 == 0 && Cout >= 1 && rows_ok((int64_t)B * H * W) &&
                    (int64_t)Cout * F + Cout <= 0x7fffffff,
                "gcl_unet_conv1x1_out_bwd: B %d, H %d, W %d, F %d (a multiple of 4), Cout %d", B, H, W, F, Cout);
  GCL_CHECK_ARG(gcl::aligned16(w) && gcl::aligned16(dA) && aligned8(ws),
                "gcl_unet_conv1x1_out_bwd: w and dA must be 16-byte aligned, ws 8-byte aligned");
  const size_t need = gcl_unet_conv1x1_out_bwd_ws_bytes(B, H, W, F, Cout);
  if (ws_bytes < need) {
    gcl::set_error("gcl_unet_conv1x1_out_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return GCL_ENOMEM;
  }
  const int64_t HW = (int64_t)H * W;
  const int n = (int)(B * HW), ncols = Cout * F + Cout;
  const int rows_per = gcl::chunk_rows(n), nchunk = gcl::num_chunks(n);
  const hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
  const int64_t total4 = (int64_t)n * (F / 4);
  hipLaunchKernelGGL(out_bwd_data_kernel, dim3(gcl::grid_for(total4, 1 << 16)), dim3(256), 0, st, dY, w, dA, HW, F, Cout, total4);
  GCL_CHECK_LAUNCH();
  const unsigned ct = (unsigned)gcl::cdiv(ncols, gcl::kColTile);
  hipLaunchKernelGGL(out_bwd_part_kernel, dim3(nchunk, ct), dim3(256), 0, st, dY, a, part, n, HW, F, Cout, rows_per, nchunk);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(out_bwd_final_kernel, dim3(ct), dim3(256), 0, st, part, nchunk, Cout * F, Cout, dW, db);
  GCL_CHECK_LAUNCH();
  g_launches += 3;
  return GCL_OK;
}

}  // extern "C"
