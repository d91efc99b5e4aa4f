// WeatherUNetV2 inference (src/unet/model_v2.py, eval mode): everything around the 3x3 implicit GEMM of unet.hip.
//
//   gn_stats_kernel      GroupNorm statistics of a raw convolution output, one block per (sample, group): the mean, then
//                        the centred second moment, both summed in float64 (thread-strided, then a fixed LDS tree).
//   gn_gelu_kernel       GroupNorm apply + erf GELU, element-wise.
//   pw_kernel            the bias-free 1x1 convolution over a gcl_unet_src_t of any kind (the block's skip), also the two
//                        linears of the attention (a token is a pixel): 16 pixels x 64 output channels per block, the
//                        input and the weights staged 32 channels at a time, every output an fmaf chain in ascending ci.
//   tail_a / tail_b      u = gelu(GN(z)) + skip with the per-(sample, channel) sums of a pixel chunk; then every block
//                        of the second launch adds the chunks in ascending order, forms the SE gate itself (two tiny
//                        matrix-vector products) and scales its chunk in place.
//   ln_kernel            LayerNorm over tokens, a wave per row.
//   attn_kernel          softmax(q k^T scale) v, a wave per (sample, head, query): lanes over keys for the scores, lanes
//                        over head dimensions for the values, probabilities passed lane to lane.
//   spec_fwd / spec_mix / spec_inv   the kept Fourier modes by direct sums; twiddles from the integer phase
//                        (kh h mod Hb, kw w mod Wb) through a float64 sincospi, rounded to float32.
//
// A block reads one sample only (spec_mix: one accumulator set per sample), and the order of every sum is a function of
// the layer's shape alone.  No atomics.
#include <atomic>

#include "common.h"
#include "unet_src.h"

namespace {

using gcl::unet_src::gelu_erf;
using gcl::unet_src::Src;
using gcl::unet_src::src_read;

std::atomic<int64_t> g_launches{0};

constexpr int kMaxC = 2048;     // widest block tail_b holds a gate for
constexpr int kMaxHid = 512;    // widest SE hidden layer
constexpr int kMaxModes = 1024; // kept Fourier modes spec_inv holds twiddles for
constexpr int kTwPix = 1024;    // pixels per twiddle table of spec_fwd

// sum over the block's 1024 threads in a fixed tree; every thread gets the result
__device__ __forceinline__ double block_sum_1024(double* red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(1024) void gn_stats_kernel(const float* __restrict__ z, float* __restrict__ mean,
                                                        float* __restrict__ invstd, int HW, int C, int G, float eps) {
  __shared__ double red[1024];
  const int tid = threadIdx.x, g = blockIdx.x, cpg = C / G;
  const int64_t b = blockIdx.y;
  const float* base = z + b * HW * C + g * cpg;
  const int n = HW * cpg;
  double acc = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const int pix = i / cpg, cc = i - pix * cpg;
    acc += (double)base[(int64_t)pix * C + cc];
  }
  const double m = block_sum_1024(red, acc) / (double)n;
  acc = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const int pix = i / cpg, cc = i - pix * cpg;
    const double d = (double)base[(int64_t)pix * C + cc] - m;
    acc += d * d;
  }
  const double var = block_sum_1024(red, acc) / (double)n;
  if (tid == 0) {
    mean[b * G + g] = (float)m;
    invstd[b * G + g] = 1.f / sqrtf((float)var + eps);
  }
}

// the one copy of GroupNorm apply + GELU of channels c .. c+3 of sample b
struct GnVec {
  float m[4], is[4], ga[4], be[4];
};
__device__ __forceinline__ GnVec gn_vec(const float* mean, const float* invstd, const float* gamma, const float* beta,
                                        int64_t b, int G, int cpg, int c) {
  GnVec r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int g = (c + k) / cpg;
    r.m[k] = mean[b * G + g], r.is[k] = invstd[b * G + g], r.ga[k] = gamma[c + k], r.be[k] = beta[c + k];
  }
  return r;
}
__device__ __forceinline__ float gn_gelu_one(const GnVec& n, int k, float z) {
  return gelu_erf(((z - n.m[k]) * n.is[k]) * n.ga[k] + n.be[k]);
}

__global__ __launch_bounds__(256) void gn_gelu_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, float* __restrict__ out, int HW,
                                                      int C, int G, int64_t total) {
  const int C4 = C / 4, cpg = C / G;
  const int64_t per = (int64_t)HW * C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per;
    const int c = (int)(i % C4) * 4;
    const GnVec n = gn_vec(mean, invstd, gamma, beta, b, G, cpg, c);
    const float4 v = gcl::ld4(z + i * 4);
    gcl::st4(out + i * 4, make_float4(gn_gelu_one(n, 0, v.x), gn_gelu_one(n, 1, v.y), gn_gelu_one(n, 2, v.z),
                                      gn_gelu_one(n, 3, v.w)));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The pointwise convolution over a source
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kPP = 16, kPC = 64, kPK = 32;  // pixels, output channels of a block; input channels of a stage
constexpr int kPWP = kPC + 4;                // pitch of the staged weights (16-byte aligned rows)

struct PwArgs {
  Src src;
  const float *w, *bias, *res;
  float* out;
  int64_t ldo;
  int32_t Cout, NT;
};

template <int KIND>
__global__ __launch_bounds__(256) void pw_kernel(const PwArgs s) {
  __shared__ float Xs[kPP][kPK + 1];
  __shared__ __align__(16) float Wt[kPK][kPWP];
  const int tid = threadIdx.x;
  const int ct = blockIdx.x % s.NT, pix0 = (blockIdx.x / s.NT) * kPP;
  const int64_t b = blockIdx.y;
  const int HW = s.src.H * s.src.W;
  const int p = tid >> 4, cq = tid & 15;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < s.src.Cin; k0 += kPK) {
    for (int idx = tid; idx < kPP * kPK; idx += 256) {
      const int px = idx >> 5, cc = idx & 31;
      const int pix = pix0 + px, c = k0 + cc;
      float v = 0.f;
      if (pix < HW && c < s.src.Cin) v = src_read<KIND, 1>(s.src, b, pix / s.src.W, pix % s.src.W, c).v[0];
      Xs[px][cc] = v;
    }
    for (int idx = tid; idx < kPC * kPK; idx += 256) {
      const int col = idx >> 5, cc = idx & 31;
      const int co = ct * kPC + col, c = k0 + cc;
      Wt[cc][col] = (co < s.Cout && c < s.src.Cin) ? s.w[(int64_t)co * s.src.Cin + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int cc = 0; cc < kPK; ++cc) {
      const float x = Xs[p][cc];
      const float4 w4 = *reinterpret_cast<const float4*>(&Wt[cc][cq * 4]);
      acc[0] = __builtin_fmaf(x, w4.x, acc[0]);
      acc[1] = __builtin_fmaf(x, w4.y, acc[1]);
      acc[2] = __builtin_fmaf(x, w4.z, acc[2]);
      acc[3] = __builtin_fmaf(x, w4.w, acc[3]);
    }
    __syncthreads();
  }
  const int pix = pix0 + p, co = ct * kPC + cq * 4;
  if (pix < HW && co < s.Cout) {  // Cout % 4 == 0
    const int64_t row = b * HW + pix;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (s.bias) acc[k] = acc[k] + s.bias[co + k];
      if (s.res) acc[k] = s.res[row * s.Cout + co + k] + acc[k];
    }
    gcl::st4(s.out + row * s.ldo + co, make_float4(acc[0], acc[1], acc[2], acc[3]));
  }
}

// w == NULL: the identity skip, out = the source's own channels
template <int KIND>
__global__ __launch_bounds__(256) void pw_copy_kernel(const PwArgs s, int64_t total) {
  const int HW = s.src.H * s.src.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % s.src.Cin);
    const int64_t row = i / s.src.Cin;
    const int pix = (int)(row % HW);
    s.out[row * s.ldo + c] = src_read<KIND, 1>(s.src, row / HW, pix / s.src.W, pix % s.src.W, c).v[0];
  }
}

template <int KIND>
void launch_pw(const PwArgs& a, int B, hipStream_t st) {
  const int HW = a.src.H * a.src.W;
  if (a.w) {
    hipLaunchKernelGGL((pw_kernel<KIND>), dim3((unsigned)(gcl::cdiv(HW, kPP) * a.NT), (unsigned)B), dim3(256), 0, st, a);
  } else {
    const int64_t total = (int64_t)B * HW * a.src.Cin;
    hipLaunchKernelGGL((pw_copy_kernel<KIND>), dim3(gcl::grid_for(total)), dim3(256), 0, st, a, total);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The block tail
// ---------------------------------------------------------------------------------------------------------------------
struct TailArgs {
  const float *z, *gamma, *beta, *mean, *invstd, *skip;
  const float *w1, *b1, *w2, *b2;
  float* out;
  double* part;  // [B][nchunk][C]
  int32_t HW, C, G, hid, chunk_px, nchunk;
};

__global__ __launch_bounds__(256) void tail_a_kernel(const TailArgs s) {
  __shared__ double red[256 * 4];
  const int tid = threadIdx.x, chunk = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int C4 = s.C / 4, cpg = s.C / s.G;
  const int cw = C4 < 256 ? C4 : 256, npl = 256 / cw;
  const bool active = tid < cw * npl;
  const int cql = tid % cw, pl = tid / cw;
  const int p0 = chunk * s.chunk_px, p1 = p0 + s.chunk_px < s.HW ? p0 + s.chunk_px : s.HW;
  for (int cq0 = 0; cq0 < C4; cq0 += cw) {
    const int cq = cq0 + cql;
    double a4[4] = {0.0, 0.0, 0.0, 0.0};
    if (active && cq < C4) {
      const int c = cq * 4;
      const GnVec n = gn_vec(s.mean, s.invstd, s.gamma, s.beta, b, s.G, cpg, c);
      for (int p = p0 + pl; p < p1; p += npl) {
        const int64_t off = (b * s.HW + p) * s.C + c;
        const float4 zv = gcl::ld4(s.z + off), sv = gcl::ld4(s.skip + off);
        const float4 u = make_float4(gn_gelu_one(n, 0, zv.x) + sv.x, gn_gelu_one(n, 1, zv.y) + sv.y,
                                     gn_gelu_one(n, 2, zv.z) + sv.z, gn_gelu_one(n, 3, zv.w) + sv.w);
        gcl::st4(s.out + off, u);
        a4[0] += (double)u.x, a4[1] += (double)u.y, a4[2] += (double)u.z, a4[3] += (double)u.w;
      }
    }
    if (active) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[(pl * cw + cql) * 4 + k] = a4[k];
    }
    __syncthreads();
    for (int t = tid; t < cw * 4; t += 256) {
      const int cl = t >> 2, k = t & 3;
      if (cq0 + cl < C4) {
        double sum = 0.0;
        for (int q = 0; q < npl; ++q) sum += red[(q * cw + cl) * 4 + k];
        s.part[(b * s.nchunk + chunk) * s.C + (cq0 + cl) * 4 + k] = sum;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void tail_b_kernel(const TailArgs s) {
  __shared__ float mean_s[kMaxC];
  __shared__ float gate_s[kMaxC];
  __shared__ float hid_s[kMaxHid];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, chunk = blockIdx.x;
  const int64_t b = blockIdx.y;
  for (int c = tid; c < s.C; c += 256) {
    double sum = 0.0;
    for (int q = 0; q < s.nchunk; ++q) sum += s.part[(b * s.nchunk + q) * s.C + c];
    mean_s[c] = (float)(sum / (double)s.HW);
  }
  __syncthreads();
  for (int j = wave; j < s.hid; j += 4) {
    float a = 0.f;
    for (int c = lane; c < s.C; c += 64) a = __builtin_fmaf(s.w1[(int64_t)j * s.C + c], mean_s[c], a);
    a = gcl::wave_sum(a);
    if (lane == 0) hid_s[j] = gelu_erf(a + s.b1[j]);
  }
  __syncthreads();
  for (int c = tid; c < s.C; c += 256) {
    float a = 0.f;
    for (int j = 0; j < s.hid; ++j) a = __builtin_fmaf(s.w2[(int64_t)c * s.hid + j], hid_s[j], a);
    gate_s[c] = 1.f / (1.f + expf(-(a + s.b2[c])));
  }
  __syncthreads();
  const int C4 = s.C / 4;
  const int p0 = chunk * s.chunk_px, p1 = p0 + s.chunk_px < s.HW ? p0 + s.chunk_px : s.HW;
  const int items = (p1 - p0) * C4;
  float* base = s.out + (b * s.HW + p0) * s.C;
  for (int i = tid; i < items; i += 256) {
    const int c = (i % C4) * 4;
    float4 u = gcl::ld4(base + (int64_t)i * 4);
    u.x *= gate_s[c], u.y *= gate_s[c + 1], u.z *= gate_s[c + 2], u.w *= gate_s[c + 3];
    gcl::st4(base + (int64_t)i * 4, u);
  }
}

inline int tail_chunk_px(int HW) {
  const int per = (int)gcl::cdiv(HW, 256);
  return per > 64 ? per : 64;
}

// ---------------------------------------------------------------------------------------------------------------------
// Attention
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float* __restrict__ out, int64_t rows,
                                                 int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * C;
  float a = 0.f;
  for (int c = lane; c < C; c += 64) a += xr[c];
  const float m = gcl::wave_sum(a) / (float)C;
  a = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - m;
    a = __builtin_fmaf(d, d, a);
  }
  const float is = 1.f / sqrtf(gcl::wave_sum(a) / (float)C + eps);
  for (int c = lane; c < C; c += 64) out[r * C + c] = ((xr[c] - m) * is) * gamma[c] + beta[c];
}

// q . k * scale.  D % 4 == 0: four interleaved partial sums (component d goes to sum d % 4, ascending), added as
// (s0 + s1) + (s2 + s3): fewer roundings at the magnitude of the total than one chain, and a fixed order all the same.
__device__ __forceinline__ float attn_score(const float* q, const float* k, int D, float scale) {
  if ((D & 3) == 0) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int d = 0; d < D; d += 4) {
      const float4 qv = gcl::ld4(q + d), kv = gcl::ld4(k + d);
      a0 = __builtin_fmaf(qv.x, kv.x, a0);
      a1 = __builtin_fmaf(qv.y, kv.y, a1);
      a2 = __builtin_fmaf(qv.z, kv.z, a2);
      a3 = __builtin_fmaf(qv.w, kv.w, a3);
    }
    return ((a0 + a1) + (a2 + a3)) * scale;
  }
  float a = 0.f;
  for (int d = 0; d < D; ++d) a = __builtin_fmaf(q[d], k[d], a);
  return a * scale;
}

// qkv [B][N][3][heads][D]; out [B][N][heads * D]
__global__ __launch_bounds__(256) void attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int heads,
                                                   int D, float scale) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), head = blockIdx.y;
  const int64_t b = blockIdx.z;
  if (i >= N) return;  // wave-uniform; the kernel has no block barrier
  const int C = heads * D;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + b * N * ld + head * D;
  const float* q = base + i * ld;
  const float* K = base + C;
  const float* V = base + 2 * C;
  float m = -INFINITY;
  for (int j = lane; j < N; j += 64) m = fmaxf(m, attn_score(q, K + j * ld, D, scale));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  for (int d0 = 0; d0 < D; d0 += 512) {
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    for (int j0 = 0; j0 < N; j0 += 64) {
      const int j = j0 + lane;
      const float p = j < N ? expf(attn_score(q, K + j * ld, D, scale) - m) : 0.f;
      lsum += p;
      const int cnt = N - j0 < 64 ? N - j0 : 64;
      for (int jj = 0; jj < cnt; ++jj) {
        const float pj = __shfl(p, jj, 64);
        const float* v = V + (j0 + jj) * ld + d0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int d = lane + 64 * t;
          if (d0 + d < D) o[t] = __builtin_fmaf(pj, v[d], o[t]);
        }
      }
    }
    const float l = gcl::wave_sum(lsum);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int d = d0 + lane + 64 * t;
      if (d < D) out[(b * N + i) * C + head * D + d] = o[t] / l;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The spectral convolution
// ---------------------------------------------------------------------------------------------------------------------
// (cos, sin)(2 pi (kh h / Hb + kw w / Wb)) * amp from the reduced integer phase
__device__ __forceinline__ float2 twiddle(int kh, int h, int Hb, int kw, int w, int Wb, double amp) {
  const int a = (kh * h) % Hb, c = (kw * w) % Wb;
  double sn, cs;
  sincospi(2.0 * ((double)a / (double)Hb + (double)c / (double)Wb), &sn, &cs);
  return make_float2((float)(cs * amp), (float)(sn * amp));
}

// packed[(mode * Cin + i) * Cout + o] = (re, im)[i][o][kh][kw], mode = kh * mw + kw
__global__ __launch_bounds__(256) void spec_pack_kernel(const float* __restrict__ wre, const float* __restrict__ wim,
                                                        float2* __restrict__ packed, int Cin, int Cout, int MH, int MW,
                                                        int mw, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int o = (int)(i % Cout);
    const int64_t r = i / Cout;
    const int ci = (int)(r % Cin), mode = (int)(r / Cin);
    const int64_t src = (((int64_t)ci * Cout + o) * MH + mode / mw) * MW + mode % mw;
    packed[i] = make_float2(wre[src], wim[src]);
  }
}

// X[b][mode][i] = (Hb Wb)^-1/2 sum over the pixels (ascending) of x[b][pix][i] exp(-i theta)
__global__ __launch_bounds__(256) void spec_fwd_kernel(const float* __restrict__ x, float2* __restrict__ X, int Hb, int Wb,
                                                       int C, int mw, int nmodes) {
  __shared__ float2 tw[kTwPix];
  const int tid = threadIdx.x, mode = blockIdx.x, i = blockIdx.y * 256 + tid;
  const int64_t b = blockIdx.z;
  const int kh = mode / mw, kw = mode % mw, HW = Hb * Wb;
  const double amp = 1.0 / sqrt((double)HW);
  float re = 0.f, im = 0.f;
  for (int p0 = 0; p0 < HW; p0 += kTwPix) {
    const int cnt = HW - p0 < kTwPix ? HW - p0 : kTwPix;
    __syncthreads();
    for (int t = tid; t < cnt; t += 256) tw[t] = twiddle(kh, (p0 + t) / Wb, Hb, kw, (p0 + t) % Wb, Wb, amp);
    __syncthreads();
    if (i < C) {
      const float* xp = x + (b * HW + p0) * C + i;
      for (int t = 0; t < cnt; ++t) {
        const float v = xp[(int64_t)t * C];
        re = __builtin_fmaf(v, tw[t].x, re);
        im = __builtin_fmaf(-v, tw[t].y, im);
      }
    }
  }
  if (i < C) X[(b * nmodes + mode) * C + i] = make_float2(re, im);
}

constexpr int kMixW = 8, kMixB = 4;  // waves that split Cin; samples per pass over the weights
// O[b][mode][o] = sum over i of X[b][mode][i] * packed[mode][i][o]: wave w adds its eighth of Cin in ascending i, the eight
// partial sums are added as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))
__global__ __launch_bounds__(64 * kMixW) void spec_mix_kernel(const float2* __restrict__ X, const float2* __restrict__ Wp,
                                                              float2* __restrict__ O, int B, int nmodes, int Cin, int Cout) {
  __shared__ float2 xs[kMixW][kMixB][64];
  __shared__ float2 red[kMixW][kMixB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mode = blockIdx.x;
  const int o = blockIdx.y * 64 + lane;
  const int per = (Cin + kMixW - 1) / kMixW;
  const int i_beg = wave * per, i_end = i_beg + per < Cin ? i_beg + per : Cin;
  const int nch = (per + 63) / 64;
  for (int b0 = 0; b0 < B; b0 += kMixB) {
    float2 acc[kMixB];
#pragma unroll
    for (int t = 0; t < kMixB; ++t) acc[t] = make_float2(0.f, 0.f);
    for (int ch = 0; ch < nch; ++ch) {
      const int i0 = i_beg + ch * 64;
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kMixB; ++t)
        xs[wave][t][lane] = (b0 + t < B && i0 + lane < i_end) ? X[((int64_t)(b0 + t) * nmodes + mode) * Cin + i0 + lane]
                                                               : make_float2(0.f, 0.f);
      __syncthreads();
      const int cnt = i_end - i0 < 64 ? i_end - i0 : 64;
      if (o < Cout) {
        const float2* wp = Wp + ((int64_t)mode * Cin + i0) * Cout + o;
#pragma unroll 4
        for (int ii = 0; ii < cnt; ++ii) {
          const float2 w = wp[(int64_t)ii * Cout];
#pragma unroll
          for (int t = 0; t < kMixB; ++t) {
            const float2 v = xs[wave][t][ii];
            acc[t].x = __builtin_fmaf(v.x, w.x, acc[t].x);
            acc[t].x = __builtin_fmaf(-v.y, w.y, acc[t].x);
            acc[t].y = __builtin_fmaf(v.x, w.y, acc[t].y);
            acc[t].y = __builtin_fmaf(v.y, w.x, acc[t].y);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kMixB; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave == 0 && o < Cout) {
      for (int t = 0; t < kMixB && b0 + t < B; ++t) {
        float2 r;
        r.x = ((red[0][t][lane].x + red[1][t][lane].x) + (red[2][t][lane].x + red[3][t][lane].x)) +
              ((red[4][t][lane].x + red[5][t][lane].x) + (red[6][t][lane].x + red[7][t][lane].x));
        r.y = ((red[0][t][lane].y + red[1][t][lane].y) + (red[2][t][lane].y + red[3][t][lane].y)) +
              ((red[4][t][lane].y + red[5][t][lane].y) + (red[6][t][lane].y + red[7][t][lane].y));
        O[((int64_t)(b0 + t) * nmodes + mode) * Cout + o] = r;
      }
    }
  }
}

// y[b][pix][o] = (Hb Wb)^-1/2 sum over the modes (ascending) of c_kw Re(O[b][mode][o] exp(+i theta))
__global__ __launch_bounds__(256) void spec_inv_kernel(const float2* __restrict__ O, float* __restrict__ out, int64_t ldo,
                                                       int Hb, int Wb, int Cout, int mw, int nmodes) {
  __shared__ float2 tw[kMaxModes];
  const int tid = threadIdx.x, pix = blockIdx.x, HW = Hb * Wb;
  const int64_t b = blockIdx.y;
  const double amp = 1.0 / sqrt((double)HW);
  for (int t = tid; t < nmodes; t += 256) {
    const int kw = t % mw;
    const double ck = (kw == 0 || (Wb % 2 == 0 && kw == Wb / 2)) ? 1.0 : 2.0;
    tw[t] = twiddle(t / mw, pix / Wb, Hb, kw, pix % Wb, Wb, amp * ck);
  }
  __syncthreads();
  for (int o = tid; o < Cout; o += 256) {
    const float2* op = O + b * nmodes * Cout + o;
    float a = 0.f;
    for (int t = 0; t < nmodes; ++t) {
      const float2 v = op[(int64_t)t * Cout];
      a = __builtin_fmaf(v.x, tw[t].x, a);
      a = __builtin_fmaf(-v.y, tw[t].y, a);
    }
    out[(b * HW + pix) * ldo + o] = a;
  }
}

}  // namespace

extern "C" {

int64_t gcl_unet_v2_launches(void) { return g_launches.load(); }

int gcl_unet_v2_gn_stats(const float* z, int32_t B, int32_t HW, int32_t C, int32_t G, float eps, float* mean, float* invstd,
                         gcl_stream_t stream) {
  GCL_CHECK_ARG(z && mean && invstd, "gcl_unet_v2_gn_stats: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && HW >= 1 && C >= 1 && G >= 1 && C % G == 0 && (int64_t)HW * C <= 0x7fffffff,
                "gcl_unet_v2_gn_stats: B %d, HW %d, C %d, G %d (G divides C, HW * C < 2^31, B <= 65535)", B, HW, C, G);
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)G, (unsigned)B), dim3(1024), 0, (hipStream_t)stream, z, mean, invstd,
                     HW, C, G, eps);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_gn_gelu(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                        float* out, int32_t B, int32_t HW, int32_t C, int32_t G, gcl_stream_t stream) {
  GCL_CHECK_ARG(z && gamma && beta && mean && invstd && out, "gcl_unet_v2_gn_gelu: null pointer");
  GCL_CHECK_ARG(B >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && G >= 1 && C % G == 0,
                "gcl_unet_v2_gn_gelu: B %d, HW %d, C %d (a multiple of 4), G %d (divides C)", B, HW, C, G);
  GCL_CHECK_ARG(gcl::aligned16(z) && gcl::aligned16(out), "gcl_unet_v2_gn_gelu: z and out must be 16-byte aligned");
  const int64_t total = (int64_t)B * HW * (C / 4);
  hipLaunchKernelGGL(gn_gelu_kernel, dim3(gcl::grid_for(total)), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, mean,
                     invstd, out, HW, C, G, total);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_conv1x1(const gcl_unet_src_t* src, const float* w, const float* bias, const float* res, float* out,
                        int64_t ldo, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, gcl_stream_t stream) {
  GCL_CHECK_ARG(out, "gcl_unet_v2_conv1x1: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 4 && Cout % 4 == 0 && ldo >= Cout &&
                    ldo % 4 == 0 && (int64_t)H * W <= 0x7fffffff / kPP,
                "gcl_unet_v2_conv1x1: B %d, H %d, W %d, Cin %d, Cout %d, ldo %lld (Cout and ldo multiples of 4, ldo >= Cout)",
                B, H, W, Cin, Cout, (long long)ldo);
  GCL_CHECK_ARG(gcl::aligned16(out), "gcl_unet_v2_conv1x1: out must be 16-byte aligned");
  GCL_CHECK_ARG(w || (Cin == Cout && !bias && !res), "gcl_unet_v2_conv1x1: w == NULL is the identity (Cin == Cout, no bias, no res)");
  PwArgs a{};
  bool vec;  // the pointwise kernels read scalars only
  if (const int rc = gcl::unet_src::bind(src, H, W, Cin, "gcl_unet_v2_conv1x1", a.src, vec)) return rc;
  a.w = w, a.bias = bias, a.res = res, a.out = out, a.ldo = ldo, a.Cout = Cout, a.NT = (int)gcl::cdiv(Cout, kPC);
  const int rc = gcl::unet_src::with_kind(src->kind, [&](auto K) {
    launch_pw<decltype(K)::value>(a, B, (hipStream_t)stream);
    return GCL_OK;
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int32_t gcl_unet_v2_tail_chunks(int32_t HW) { return HW < 1 ? 0 : (int32_t)gcl::cdiv(HW, tail_chunk_px(HW)); }

size_t gcl_unet_v2_tail_ws_bytes(int32_t B, int32_t HW, int32_t C) {
  if (B < 1 || HW < 1 || C < 1) return 0;
  return (size_t)B * gcl_unet_v2_tail_chunks(HW) * C * sizeof(double);
}

int gcl_unet_v2_block_tail(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                           const float* skip, const float* w1, const float* b1, const float* w2, const float* b2,
                           float* out, int32_t B, int32_t HW, int32_t C, int32_t G, int32_t hidden, void* ws,
                           size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(z && gamma && beta && mean && invstd && skip && w1 && b1 && w2 && b2 && out && ws,
                "gcl_unet_v2_block_tail: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && HW >= 1 && C >= 4 && C % 4 == 0 && C <= kMaxC && G >= 1 && C % G == 0 &&
                    hidden >= 1 && hidden <= kMaxHid && (int64_t)HW * C <= 0x7fffffff,
                "gcl_unet_v2_block_tail: B %d, HW %d, C %d (a multiple of 4, <= %d), G %d (divides C), hidden %d (<= %d)", B,
                HW, C, kMaxC, G, hidden, kMaxHid);
  GCL_CHECK_ARG(gcl::aligned16(z) && gcl::aligned16(skip) && gcl::aligned16(out) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "gcl_unet_v2_block_tail: z, skip and out must be 16-byte aligned, ws 8-byte aligned");
  GCL_CHECK_ARG(ws_bytes >= gcl_unet_v2_tail_ws_bytes(B, HW, C), "gcl_unet_v2_block_tail: ws holds %zu bytes, %zu needed",
                ws_bytes, gcl_unet_v2_tail_ws_bytes(B, HW, C));
  TailArgs a{};
  a.z = z, a.gamma = gamma, a.beta = beta, a.mean = mean, a.invstd = invstd, a.skip = skip;
  a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.out = out, a.part = (double*)ws;
  a.HW = HW, a.C = C, a.G = G, a.hid = hidden, a.chunk_px = tail_chunk_px(HW), a.nchunk = gcl_unet_v2_tail_chunks(HW);
  const dim3 grid((unsigned)a.nchunk, (unsigned)B);
  hipLaunchKernelGGL(tail_a_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  hipLaunchKernelGGL(tail_b_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out, int64_t rows,
                          int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(x && gamma && beta && out, "gcl_unet_v2_layernorm: null pointer");
  GCL_CHECK_ARG(rows >= 1 && C >= 1 && gcl::cdiv(rows, 4) <= 0x7fffffff, "gcl_unet_v2_layernorm: rows %lld, C %d",
                (long long)rows, C);
  hipLaunchKernelGGL(ln_kernel, dim3((unsigned)gcl::cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out,
                     rows, C, eps);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_attention(const float* qkv, float* out, int32_t B, int32_t N, int32_t heads, int32_t head_dim,
                          gcl_stream_t stream) {
  GCL_CHECK_ARG(qkv && out, "gcl_unet_v2_attention: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && N <= 4096 && heads >= 1 && heads <= 65535 && head_dim >= 1,
                "gcl_unet_v2_attention: B %d, N %d (at most 4096), heads %d, head_dim %d", B, N, heads, head_dim);
  GCL_CHECK_ARG(gcl::aligned16(qkv), "gcl_unet_v2_attention: qkv must be 16-byte aligned");
  const float scale = 1.f / sqrtf((float)head_dim);
  hipLaunchKernelGGL(attn_kernel, dim3((unsigned)gcl::cdiv(N, 4), (unsigned)heads, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, qkv, out, N, heads, head_dim, scale);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_spectral_pack(const float* w_re, const float* w_im, int32_t Cin, int32_t Cout, int32_t modes_h,
                              int32_t modes_w, int32_t mh, int32_t mw, float* packed, gcl_stream_t stream) {
  GCL_CHECK_ARG(w_re && w_im && packed, "gcl_unet_v2_spectral_pack: null pointer");
  GCL_CHECK_ARG(Cin >= 1 && Cout >= 1 && mh >= 1 && mw >= 1 && mh <= modes_h && mw <= modes_w,
                "gcl_unet_v2_spectral_pack: Cin %d, Cout %d, modes %d x %d of %d x %d", Cin, Cout, mh, mw, modes_h, modes_w);
  GCL_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 7) == 0, "gcl_unet_v2_spectral_pack: packed must be 8-byte aligned");
  const int64_t total = (int64_t)mh * mw * Cin * Cout;
  hipLaunchKernelGGL(spec_pack_kernel, dim3(gcl::grid_for(total)), dim3(256), 0, (hipStream_t)stream, w_re, w_im,
                     (float2*)packed, Cin, Cout, modes_h, modes_w, mw, total);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

#define GCL_SPEC_CHECK(name)                                                                                          \
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && Hb >= 1 && Wb >= 1 && Hb <= 32768 && Wb <= 32768 && (int64_t)Hb * Wb <= (1 << 24) && \
                    C >= 1 && mh >= 1 && mh <= Hb && mw >= 1 && mw <= Wb / 2 + 1 && mh * mw <= kMaxModes,               \
                name ": B %d, grid %d x %d, C %d, modes %d x %d (mh <= Hb, mw <= Wb / 2 + 1, at most %d modes)", B, Hb, Wb, \
                C, mh, mw, kMaxModes)

int gcl_unet_v2_spectral_fwd(const float* x, float* X, int32_t B, int32_t Hb, int32_t Wb, int32_t C, int32_t mh, int32_t mw,
                             gcl_stream_t stream) {
  GCL_CHECK_ARG(x && X, "gcl_unet_v2_spectral_fwd: null pointer");
  GCL_SPEC_CHECK("gcl_unet_v2_spectral_fwd");
  GCL_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 7) == 0, "gcl_unet_v2_spectral_fwd: X must be 8-byte aligned");
  hipLaunchKernelGGL(spec_fwd_kernel, dim3((unsigned)(mh * mw), (unsigned)gcl::cdiv(C, 256), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, x, (float2*)X, Hb, Wb, C, mw, mh * mw);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_spectral_mix(const float* X, const float* packed, float* O, int32_t B, int32_t nmodes, int32_t Cin,
                             int32_t Cout, gcl_stream_t stream) {
  GCL_CHECK_ARG(X && packed && O, "gcl_unet_v2_spectral_mix: null pointer");
  GCL_CHECK_ARG(B >= 1 && nmodes >= 1 && Cin >= 1 && Cout >= 1 && gcl::cdiv(Cout, 64) <= 65535,
                "gcl_unet_v2_spectral_mix: B %d, modes %d, Cin %d, Cout %d", B, nmodes, Cin, Cout);
  GCL_CHECK_ARG(((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(O)) & 7) == 0,
                "gcl_unet_v2_spectral_mix: X, packed and O must be 8-byte aligned");
  hipLaunchKernelGGL(spec_mix_kernel, dim3((unsigned)nmodes, (unsigned)gcl::cdiv(Cout, 64)), dim3(64 * kMixW), 0,
                     (hipStream_t)stream, (const float2*)X, (const float2*)packed, (float2*)O, B, nmodes, Cin, Cout);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_v2_spectral_inv(const float* O, float* out, int64_t ldo, int32_t B, int32_t Hb, int32_t Wb, int32_t C,
                             int32_t mh, int32_t mw, gcl_stream_t stream) {
  GCL_CHECK_ARG(O && out, "gcl_unet_v2_spectral_inv: null pointer");
  GCL_SPEC_CHECK("gcl_unet_v2_spectral_inv");
  GCL_CHECK_ARG(ldo >= C && (reinterpret_cast<uintptr_t>(O) & 7) == 0, "gcl_unet_v2_spectral_inv: ldo %lld < C %d, or O not 8-byte aligned",
                (long long)ldo, C);
  hipLaunchKernelGGL(spec_inv_kernel, dim3((unsigned)(Hb * Wb), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)O, out, ldo, Hb, Wb, C, mw, mh * mw);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

}  // extern "C"
