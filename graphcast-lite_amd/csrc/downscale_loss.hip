// The training objective and the scores of the U-Net downscaler (gfx950): masked_mse_loss, spectral_loss and
// gradient_loss (scripts/train_downscaler.py:189-220) with their gradients with respect to the network's output, and
// the per-batch means of compute_metrics (:280-298).  No entry point allocates or synchronises; offsets are int64; no
// floating-point atomics; every reduction has a fixed order, so results are bit-equal from run to run; scratch is
// passed in (gcl_downscale_loss_ws_bytes).  All sums run in float64 on float32 differences.
//
// Layout of the spectral term: a separable direct DFT of the half spectrum, rows then columns, twiddles from tables
// built in double by the caller.  A (H, W) map never has to fit in LDS: the row pass stages kTH rows, writes the
// half-spectrum rows of both fields to scratch as [map][kx][h] (a column is contiguous), the column pass takes
// 256 / H columns per block, forms |P|, |T|, the loss and the cotangent, applies the adjoint column transform in
// place, and the adjoint row pass stages kTH rows of that again and adds into dOut.
#include "common.h"

using gcl::rounded;
using gcl::wave_sum;

namespace {

constexpr int kMaxDim = 256;  // H, W of the spectral term (and of the tiles here)
constexpr int kMaxC = 64;     // the limit of gcl_downscale_batch
constexpr int kBlocks = 2048; // most blocks of a reducing kernel
constexpr int kTH = 8;        // rows of a tile
constexpr int kChunks = 64;   // most chunks per channel of the metrics
constexpr size_t kPartBytes = 65536;  // the partial records in front of the workspace

unsigned blocks_for(int64_t items) { return (unsigned)(items < kBlocks ? (items > 0 ? items : 1) : kBlocks); }

// the sum of one value per thread of a 256-thread block in a fixed order (butterfly per wave, then wave 0 .. 3);
// red: 4 doubles of LDS.  Every thread gets the sum.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double2 cplx(double re, double im) {
  double2 r;
  r.x = re;
  r.y = im;
  return r;
}

struct Fields {
  const float* out;
  const float* xl;  // the residual base (batch stride xbs, channel stride H * W) or nullptr
  const float* y;
  const float* mask;
  int64_t xbs;
  int32_t B, C, H, W;
};

// o - y of one element, o = out or x_last + out rounded once in float32
__device__ __forceinline__ float field_o(const Fields& f, int64_t b, int c, int64_t bc_off, int64_t idx) {
  float o = f.out[bc_off + idx];
  if (f.xl) o = rounded(f.xl[b * f.xbs + (int64_t)c * f.H * f.W + idx] + o);
  return o;
}

// ---- mse + finite differences: scripts/train_downscaler.py:189-193, :207-220 ----------------------------------------
struct LossArgs {
  Fields f;
  float* dout;
  double* part;  // [blocks][3]: sum m e^2, sum m dy^2, sum m dx^2
  int64_t nitems;
  int32_t nth, do_mse, do_grad;
  double cm, cy, cx;  // 2 * weight / count of the three sums, as they enter dOut
};

// An item is (map b * C + c, tile of kTH rows).  The tile's e = o - y is staged with one halo row either side, so every
// thread forms the differences of its elements from LDS and writes its dOut element once: no neighbour tile is
// written.  Element (h, w) owns the differences towards h + 1 and w + 1 in the sums.
__global__ __launch_bounds__(256) void downscale_loss_kernel(LossArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);
  float* e = reinterpret_cast<float*>(smem + 32);
  const int tid = threadIdx.x;
  const int H = a.f.H, W = a.f.W;
  const int64_t HW = (int64_t)H * W;
  double s_mse = 0.0, s_dy = 0.0, s_dx = 0.0;
  for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const int ht = (int)(item % a.nth);
    const int64_t bc = item / a.nth;
    const int c = (int)(bc % a.f.C);
    const int64_t b = bc / a.f.C;
    const int h0 = ht * kTH;
    const int thn = H - h0 < kTH ? H - h0 : kTH;
    const int r_lo = h0 > 0 ? h0 - 1 : 0, r_hi = h0 + thn + 1 < H ? h0 + thn + 1 : H;
    const double m = a.f.mask ? (double)a.f.mask[c] : 1.0;
    const int64_t off = bc * HW;
    float* stage = e + (r_lo - (h0 - 1)) * W;  // LDS row 0 is row h0 - 1
    for (int k = tid; k < (r_hi - r_lo) * W; k += 256) {
      const int64_t idx = (int64_t)r_lo * W + k;
      stage[k] = rounded(field_o(a.f, b, c, off, idx) - a.f.y[off + idx]);
    }
    __syncthreads();
    double t_mse = 0.0, t_dy = 0.0, t_dx = 0.0;
    for (int k = tid; k < thn * W; k += 256) {
      const int hl = k / W, w = k - hl * W, h = h0 + hl;
      const float* p = e + (hl + 1) * W + w;
      const double ec = (double)p[0];
      double gy = 0.0, gx = 0.0;
      if (a.do_grad) {
        if (h + 1 < H) {
          const double d = (double)p[W] - ec;
          t_dy += d * d;
          gy -= d;
        }
        if (h > 0) gy += ec - (double)p[-W];
        if (w + 1 < W) {
          const double d = (double)p[1] - ec;
          t_dx += d * d;
          gx -= d;
        }
        if (w > 0) gx += ec - (double)p[-1];
      }
      if (a.do_mse) t_mse += ec * ec;
      if (a.dout) a.dout[off + (int64_t)h * W + w] = (float)(m * (a.cm * ec + a.cy * gy + a.cx * gx));
    }
    s_mse += m * t_mse;
    s_dy += m * t_dy;
    s_dx += m * t_dx;
    __syncthreads();
  }
  s_mse = block_sum(s_mse, red);
  s_dy = block_sum(s_dy, red);
  s_dx = block_sum(s_dx, red);
  if (tid == 0) {
    a.part[(int64_t)blockIdx.x * 3] = s_mse;
    a.part[(int64_t)blockIdx.x * 3 + 1] = s_dy;
    a.part[(int64_t)blockIdx.x * 3 + 2] = s_dx;
  }
}

// rec[dst[q]] = sum over the q with that destination of coef[q] * (sum over the blocks' records of value q); a
// destination below 0 is left alone.  One block: thread t takes records t, t + 256, .., then block_sum.
struct FinishArgs {
  const double* part;
  double* rec;
  int32_t nparts, K;
  double coef[3];
  int32_t dst[3];
};

__global__ __launch_bounds__(256) void downscale_loss_finish_kernel(FinishArgs a) {
  __shared__ double red[4];
  double acc[3] = {0.0, 0.0, 0.0};
  bool hit[3] = {false, false, false};
  for (int q = 0; q < a.K; ++q) {
    double s = 0.0;
    for (int p = threadIdx.x; p < a.nparts; p += 256) s += a.part[(int64_t)p * a.K + q];
    s = block_sum(s, red);
    if (a.dst[q] >= 0) {
      acc[a.dst[q]] += a.coef[q] * s;
      hit[a.dst[q]] = true;
    }
  }
  if (threadIdx.x == 0)
    for (int d = 0; d < 3; ++d)
      if (hit[d]) a.rec[d] = acc[d];
}

// ---- spectral: scripts/train_downscaler.py:196-204 -------------------------------------------------------------------
struct SpecArgs {
  Fields f;
  const double2* twh;  // [H] (cos, sin)(2 pi k / H)
  const double2* tww;  // [W]
  double2* RP;         // [B * C][KX][H]: row transforms of m * o, then the adjoint column transform of the cotangent
  double2* RT;         // the same of m * y
  double* part;        // [blocks]
  float* dout;
  int64_t nitems;
  int32_t KX, nth, ncol, ngrp, accumulate;
  double scale, inv_count, sw;
};

// Row pass.  An item is (map, tile of kTH rows): both masked fields of the tile are staged, then one thread per
// (kx, row) sums the row of either field against e^{-2 pi i kx w / W}; rows are the fastest index, so the stores of a
// kx are contiguous.
__global__ __launch_bounds__(256) void downscale_spec_rows_kernel(SpecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2* tw = reinterpret_cast<double2*>(smem);
  const int H = a.f.H, W = a.f.W, KX = a.KX;
  float* xs = reinterpret_cast<float*>(smem + (size_t)W * sizeof(double2));
  float* ys = xs + kTH * W;
  const int tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  for (int k = tid; k < W; k += 256) tw[k] = a.tww[k];
  for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const int ht = (int)(item % a.nth);
    const int64_t bc = item / a.nth;
    const int c = (int)(bc % a.f.C);
    const int64_t b = bc / a.f.C;
    const int h0 = ht * kTH;
    const int thn = H - h0 < kTH ? H - h0 : kTH;
    const int64_t off = bc * HW;
    __syncthreads();
    for (int k = tid; k < thn * W; k += 256) {
      const int64_t idx = (int64_t)h0 * W + k;
      float o = field_o(a.f, b, c, off, idx), y = a.f.y[off + idx];
      if (a.f.mask) {
        o = rounded(o * a.f.mask[c]);
        y = rounded(y * a.f.mask[c]);
      }
      xs[k] = o;
      ys[k] = y;
    }
    __syncthreads();
    // one thread per (kx, row) forms both fields: the twiddle is read once for the two
    for (int e = tid; e < thn * KX; e += 256) {
      const int kx = e / thn, r = e - kx * thn;
      const float* sx = xs + r * W;
      const float* sy = ys + r * W;
      double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
      int idx = 0;
#pragma unroll 4
      for (int w = 0; w < W; ++w) {
        const double2 t = tw[idx];
        const double vx = (double)sx[w], vy = (double)sy[w];
        xr += vx * t.x;
        xi -= vx * t.y;
        yr += vy * t.x;
        yi -= vy * t.y;
        idx += kx;
        if (idx >= W) idx -= W;
      }
      const int64_t at = (bc * KX + kx) * H + h0 + r;
      a.RP[at] = cplx(xr, xi);
      a.RT[at] = cplx(yr, yi);
    }
  }
}

// Column pass.  An item is (map, group of ncol = 256 / H columns kx); thread j * H + ky forms P and T of its bin, the
// loss term and the cotangent G = sign(|P| - |T|) P / |P| / count (0 where |P| = 0 or |P| = |T|), then, as thread
// j * H + h, the adjoint column transform S[h] = sum_ky G[ky] e^{+2 pi i ky h / H}, which replaces the column in RP.
__global__ __launch_bounds__(256) void downscale_spec_cols_kernel(SpecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);
  double2* tw = reinterpret_cast<double2*>(smem + 32);
  const int H = a.f.H, KX = a.KX;
  double2* cp = tw + H;
  double2* ct = cp + 256;
  double2* cg = ct + 256;
  const int tid = threadIdx.x;
  const int j = tid / H, ky = tid - j * H;
  for (int k = tid; k < H; k += 256) tw[k] = a.twh[k];
  double s_spec = 0.0;
  for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const int grp = (int)(item % a.ngrp);
    const int64_t bc = item / a.ngrp;
    const int kx = grp * a.ncol + j;
    const bool valid = j < a.ncol && kx < KX;
    const int64_t col = (bc * KX + kx) * H;
    __syncthreads();
    if (valid) {
      cp[tid] = a.RP[col + ky];
      ct[tid] = a.RT[col + ky];
    }
    __syncthreads();
    double2 g = cplx(0.0, 0.0);
    if (valid) {
      const double2* pc = cp + j * H;
      const double2* tc = ct + j * H;
      double pr = 0.0, pi = 0.0, tr = 0.0, ti = 0.0;
      int idx = 0;
#pragma unroll 4
      for (int h = 0; h < H; ++h) {
        const double2 t = tw[idx], p = pc[h], q = tc[h];
        pr += p.x * t.x + p.y * t.y;  // (p.x + i p.y)(cos - i sin)
        pi += p.y * t.x - p.x * t.y;
        tr += q.x * t.x + q.y * t.y;
        ti += q.y * t.x - q.x * t.y;
        idx += ky;
        if (idx >= H) idx -= H;
      }
      pr *= a.scale; pi *= a.scale; tr *= a.scale; ti *= a.scale;
      const double ap = hypot(pr, pi), at = hypot(tr, ti), d = ap - at;
      s_spec += fabs(d);
      if (ap > 0.0 && d != 0.0) {
        const double k = (d > 0.0 ? a.inv_count : -a.inv_count) / ap;
        g = cplx(pr * k, pi * k);
      }
    }
    cg[tid] = g;
    __syncthreads();
    if (valid) {
      const double2* gc = cg + j * H;
      double sr = 0.0, si = 0.0;
      int idx = 0;
#pragma unroll 4
      for (int k = 0; k < H; ++k) {
        const double2 t = tw[idx], q = gc[k];
        sr += q.x * t.x - q.y * t.y;  // (q.x + i q.y)(cos + i sin)
        si += q.x * t.y + q.y * t.x;
        idx += ky;  // (ky is this thread's h here)
        if (idx >= H) idx -= H;
      }
      a.RP[col + ky] = cplx(sr, si);
    }
  }
  s_spec = block_sum(s_spec, red);
  if (tid == 0) a.part[blockIdx.x] = s_spec;
}

// Adjoint row pass.  An item is (map, tile of kTH rows): S of the tile is staged, one thread per (row, w) forms
// Re sum_kx S[h][kx] e^{+2 pi i kx w / W} / sqrt(H W), and dOut takes spectral_weight * m_c * that (added, or stored
// when nothing wrote dOut before).
__global__ __launch_bounds__(256) void downscale_spec_adj_kernel(SpecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2* tw = reinterpret_cast<double2*>(smem);
  const int H = a.f.H, W = a.f.W, KX = a.KX;
  double2* ss = tw + W;  // [kTH][KX]
  const int tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  for (int k = tid; k < W; k += 256) tw[k] = a.tww[k];
  for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const int ht = (int)(item % a.nth);
    const int64_t bc = item / a.nth;
    const int c = (int)(bc % a.f.C);
    const int h0 = ht * kTH;
    const int thn = H - h0 < kTH ? H - h0 : kTH;
    const double m = (a.f.mask ? (double)a.f.mask[c] : 1.0) * a.sw * a.scale;
    __syncthreads();
    for (int e = tid; e < thn * KX; e += 256) {
      const int kx = e / thn, r = e - kx * thn;
      ss[r * KX + kx] = a.RP[(bc * KX + kx) * H + h0 + r];
    }
    __syncthreads();
    for (int e = tid; e < thn * W; e += 256) {
      const int r = e / W, w = e - r * W;
      const double2* s = ss + r * KX;
      double acc = 0.0;
      int idx = 0;
#pragma unroll 4
      for (int kx = 0; kx < KX; ++kx) {
        const double2 t = tw[idx];
        acc += s[kx].x * t.x - s[kx].y * t.y;
        idx += w;
        if (idx >= W) idx -= W;
      }
      float* dst = a.dout + bc * HW + (int64_t)(h0 + r) * W + w;
      *dst = a.accumulate ? (float)((double)*dst + m * acc) : (float)(m * acc);
    }
  }
}

// ---- metrics: compute_metrics, scripts/train_downscaler.py:280-298 ---------------------------------------------------
// Stage 1: block (chunk, c) sums (o - y)^2 and (x_last - y)^2 over its share of the B * H * W elements of channel c.
// Stage 2: one wave per channel adds the chunks (lane = chunk, fixed butterfly), divides by the element count and adds
// the two means to the state; the first wave also advances the batch counter.
__global__ __launch_bounds__(256) void downscale_metrics_kernel(Fields f, int32_t residual, int32_t nchunk, double* part) {
  __shared__ double red[4];
  const int c = blockIdx.y, chunk = blockIdx.x;
  const int64_t HW = (int64_t)f.H * f.W, n = (int64_t)f.B * HW, span = (n + nchunk - 1) / nchunk;
  const int64_t i1 = (chunk + 1) * span < n ? (chunk + 1) * span : n;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = chunk * span + threadIdx.x; i < i1; i += 256) {
    const int64_t b = i / HW, p = i - b * HW;
    const int64_t o_off = (b * f.C + c) * HW + p;
    const float yv = f.y[o_off], xv = f.xl[b * f.xbs + (int64_t)c * HW + p];
    float ov = f.out[o_off];
    if (residual) ov = rounded(xv + ov);
    const double d1 = (double)rounded(ov - yv), d2 = (double)rounded(xv - yv);
    s1 += d1 * d1;
    s2 += d2 * d2;
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    part[((int64_t)c * nchunk + chunk) * 2] = s1;
    part[((int64_t)c * nchunk + chunk) * 2 + 1] = s2;
  }
}

__global__ __launch_bounds__(64) void downscale_metrics_add_kernel(const double* __restrict__ part, int32_t nchunk,
                                                                   double inv_n, double* state, int64_t* count) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (lane < nchunk) {
    s1 = part[((int64_t)c * nchunk + lane) * 2];
    s2 = part[((int64_t)c * nchunk + lane) * 2 + 1];
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    state[c * 2] += s1 * inv_n;
    state[c * 2 + 1] += s2 * inv_n;
    if (c == 0) count[0] += 1;
  }
}

__global__ __launch_bounds__(256) void downscale_loss_scale_kernel(const float* __restrict__ d, const float* __restrict__ g,
                                                                   int64_t n, float* __restrict__ out) {
  const float s = g[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = d[i] * s;
}

size_t spectrum_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  return (size_t)B * C * H * (W / 2 + 1) * sizeof(double2);
}

}  // namespace

#define GCL_CHECK_LOSS_SHAPE(who)                                                                                     \
  GCL_CHECK_ARG(B > 0 && C > 0 && C <= kMaxC && H >= 2 && H <= kMaxDim && W >= 2 && W <= kMaxDim,                     \
                who ": bad shape (B=%d C=%d (1 .. 64) H=%d W=%d (2 .. 256 each))", B, C, H, W);                      \
  GCL_CHECK_ARG(x_last == nullptr || xbs >= (int64_t)C * H * W, who ": a batch stride of %lld for %d x %d x %d", \
                (long long)xbs, C, H, W)

extern "C" size_t gcl_downscale_loss_ws_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return kPartBytes;
  return kPartBytes + 2 * spectrum_bytes(B, C, H, W);
}

extern "C" int gcl_downscale_loss_fwd_bwd(const float* out, const float* x_last, int64_t xbs, const float* Y,
                                          const float* mask, int32_t B, int32_t C, int32_t H, int32_t W,
                                          float mse_weight, float gradient_weight, double* rec, float* dOut, void* ws,
                                          size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(out && Y && rec && ws, "downscale_loss_fwd_bwd: null argument");
  GCL_CHECK_LOSS_SHAPE("downscale_loss_fwd_bwd");
  GCL_CHECK_ARG(ws_bytes >= kPartBytes, "downscale_loss_fwd_bwd: workspace of %zu bytes is too small (need %zu)", ws_bytes,
                kPartBytes);
  const bool do_mse = mse_weight > 0.f, do_grad = gradient_weight > 0.f;
  GCL_CHECK_ARG(do_mse || do_grad, "downscale_loss_fwd_bwd: neither term has a weight above 0");
  LossArgs a;
  a.f = Fields{out, x_last, Y, mask, xbs, B, C, H, W};
  a.dout = dOut;
  a.part = static_cast<double*>(ws);
  a.nth = (int32_t)gcl::cdiv(H, kTH);
  a.nitems = (int64_t)B * C * a.nth;
  a.do_mse = do_mse;
  a.do_grad = do_grad;
  const double n = (double)B * C * H * W, ny = (double)B * C * (H - 1) * W, nx = (double)B * C * H * (W - 1);
  a.cm = do_mse ? 2.0 * (double)mse_weight / n : 0.0;
  a.cy = do_grad ? 2.0 * (double)gradient_weight / ny : 0.0;
  a.cx = do_grad ? 2.0 * (double)gradient_weight / nx : 0.0;
  const unsigned nb = blocks_for(a.nitems);
  hipLaunchKernelGGL(downscale_loss_kernel, dim3(nb), dim3(256), 32 + (size_t)(kTH + 2) * W * sizeof(float),
                     (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  FinishArgs fa;
  fa.part = a.part; fa.rec = rec; fa.nparts = (int32_t)nb; fa.K = 3;
  fa.coef[0] = 1.0 / n; fa.coef[1] = 1.0 / ny; fa.coef[2] = 1.0 / nx;
  fa.dst[0] = do_mse ? 0 : -1; fa.dst[1] = fa.dst[2] = do_grad ? 1 : -1;
  hipLaunchKernelGGL(downscale_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, fa);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_downscale_spectral_fwd_bwd(const float* out, const float* x_last, int64_t xbs, const float* Y,
                                              const float* mask, const double* tw_h, const double* tw_w, int32_t B,
                                              int32_t C, int32_t H, int32_t W, float spectral_weight, int32_t accumulate,
                                              double* rec, float* dOut, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(out && Y && rec && ws && tw_h && tw_w, "downscale_spectral_fwd_bwd: null argument");
  GCL_CHECK_LOSS_SHAPE("downscale_spectral_fwd_bwd");
  GCL_CHECK_ARG(gcl::aligned16(ws) && gcl::aligned16(tw_h) && gcl::aligned16(tw_w),
                "downscale_spectral_fwd_bwd: the workspace and the twiddle tables are 16-byte aligned");
  const size_t need = gcl_downscale_loss_ws_bytes(B, C, H, W);
  GCL_CHECK_ARG(ws_bytes >= need, "downscale_spectral_fwd_bwd: workspace of %zu bytes is too small (need %zu)", ws_bytes, need);
  SpecArgs a;
  a.f = Fields{out, x_last, Y, mask, xbs, B, C, H, W};
  a.twh = reinterpret_cast<const double2*>(tw_h);
  a.tww = reinterpret_cast<const double2*>(tw_w);
  a.part = static_cast<double*>(ws);
  a.RP = reinterpret_cast<double2*>(static_cast<unsigned char*>(ws) + kPartBytes);
  a.RT = a.RP + (int64_t)B * C * H * (W / 2 + 1);
  a.dout = dOut;
  a.KX = W / 2 + 1;
  a.nth = (int32_t)gcl::cdiv(H, kTH);
  a.ncol = 256 / H;
  a.ngrp = (int32_t)gcl::cdiv(a.KX, a.ncol);
  a.accumulate = accumulate;
  a.scale = 1.0 / sqrt((double)H * W);
  const double count = (double)B * C * H * a.KX;
  a.inv_count = 1.0 / count;
  a.sw = (double)spectral_weight;
  hipStream_t st = (hipStream_t)stream;
  a.nitems = (int64_t)B * C * a.nth;
  hipLaunchKernelGGL(downscale_spec_rows_kernel, dim3(blocks_for(a.nitems)), dim3(256),
                     (size_t)W * sizeof(double2) + 2 * (size_t)kTH * W * sizeof(float), st, a);
  GCL_CHECK_LAUNCH();
  a.nitems = (int64_t)B * C * a.ngrp;
  const unsigned nb = blocks_for(a.nitems);
  hipLaunchKernelGGL(downscale_spec_cols_kernel, dim3(nb), dim3(256), 32 + (size_t)(H + 3 * 256) * sizeof(double2), st, a);
  GCL_CHECK_LAUNCH();
  FinishArgs fa;
  fa.part = a.part; fa.rec = rec; fa.nparts = (int32_t)nb; fa.K = 1;
  fa.coef[0] = a.inv_count; fa.coef[1] = fa.coef[2] = 0.0;
  fa.dst[0] = 2; fa.dst[1] = fa.dst[2] = -1;
  hipLaunchKernelGGL(downscale_loss_finish_kernel, dim3(1), dim3(256), 0, st, fa);
  GCL_CHECK_LAUNCH();
  if (dOut) {
    a.nitems = (int64_t)B * C * a.nth;
    hipLaunchKernelGGL(downscale_spec_adj_kernel, dim3(blocks_for(a.nitems)), dim3(256),
                       (size_t)(W + kTH * a.KX) * sizeof(double2), st, a);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}

extern "C" int gcl_downscale_metrics(const float* out, const float* x_last, int64_t xbs, const float* Y, int32_t residual,
                                     int32_t B, int32_t C, int32_t H, int32_t W, double* state, int64_t* count, void* ws,
                                     size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(out && x_last && Y && state && count && ws, "downscale_metrics: null argument");
  GCL_CHECK_ARG(B > 0 && C > 0 && C <= kMaxC && H > 0 && W > 0 && xbs >= (int64_t)C * H * W,
                "downscale_metrics: bad shape (B=%d C=%d (1 .. 64) H=%d W=%d batch stride %lld)", B, C, H, W, (long long)xbs);
  GCL_CHECK_ARG(ws_bytes >= kPartBytes, "downscale_metrics: workspace of %zu bytes is too small (need %zu)", ws_bytes,
                kPartBytes);
  const int64_t n = (int64_t)B * H * W;
  const int32_t nchunk = (int32_t)(gcl::cdiv(n, 1024) < kChunks ? gcl::cdiv(n, 1024) : kChunks);
  double* part = static_cast<double*>(ws);  // C * nchunk * 2 doubles <= 64 * 64 * 2 * 8 bytes = kPartBytes
  hipLaunchKernelGGL(downscale_metrics_kernel, dim3(nchunk, C), dim3(256), 0, (hipStream_t)stream,
                     Fields{out, x_last, Y, nullptr, xbs, B, C, H, W}, residual, nchunk, part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(downscale_metrics_add_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, part, nchunk, 1.0 / (double)n,
                     state, count);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_downscale_loss_scale(const float* dOut, const float* g, int64_t n, float* out, gcl_stream_t stream) {
  GCL_CHECK_ARG(dOut && g && out && n > 0, "downscale_loss_scale: null argument or no elements");
  hipLaunchKernelGGL(downscale_loss_scale_kernel, dim3(gcl::grid_for(n, kBlocks)), dim3(256), 0, (hipStream_t)stream, dOut, g,
                     n, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
