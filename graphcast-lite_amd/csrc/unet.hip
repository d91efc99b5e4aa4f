// WeatherUNet inference (src/unet/model.py:11-98, eval mode) and the cascade's per-step glue and scores
// (scripts/predict_cascade.py:338-372).
//
// unet_conv3x3_kernel: one 3x3 convolution + BatchNorm (running statistics) + erf GELU per launch, an implicit GEMM on
// v_mfma_f32_32x32x2_f32.  Activations are channels-last, so a pixel is a row of features and a tap is a shifted row.
//   block = 4 waves; it owns 4 x 8 output pixels of one sample (the 32 rows of one MFMA tile) and 32 output channels;
//   Cin is walked in chunks of 32 channels: the 6 x 10 input pixels (tile + one-pixel halo) of the chunk are staged in
//   LDS ONCE, through the source kind (planar / rows / pooled / upsampled + concatenated), zero outside the image and
//   past Cin (unet_src.h: stage_halo); the nine taps are nine shifted 16-byte LDS reads of that image;
//   wave w takes channels 8w .. 8w+7 of every chunk - four MFMAs per tap - so the four waves split K between them and
//   nothing but the staged image is shared; a wave's B operands come straight from the packed weights, one 16-byte
//   load per lane and (tap, 8 channels): a weight is used by one wave of the block, LDS would add a trip;
//   the four partial tiles are added in LDS as (w0 + w1) + (w2 + w3) and 256 threads run the epilogue, 4 channels each;
//   from Cin = 256 on (the deep and the concatenated layers: few pixels, long K) a block has EIGHT waves and chunks of
//   64 channels - half the K steps per wave, which is what those layers lack at B = 1 - and the tree gains
//   + ((w4 + w5) + (w6 + w7)).  The choice is a function of Cin alone.
// k order of an MFMA step q (0 .. 3): lane half h = lane >> 5 supplies channel 8g + 4h + q, so a lane's four A operands
// are one float4 of the LDS image and its four B operands one float4 of the packed record.
// The order of every sum depends on Cin alone.  A block reads one sample only.
#include <atomic>

#include <hip/hip_fp16.h>

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
using gcl::unet_src::Src;
using gcl::unet_src::stage_halo;

std::atomic<int64_t> g_launches{0};

// a block owns one tile of unet_src.h (kTH x kTW output pixels, kHP staged ones)
// channels per chunk: 8 per wave; floats between staged pixels (144 / 272 B: 16-byte aligned, 4 banks apart)
constexpr int chunk_of(int NW) { return 8 * NW; }
constexpr int pitch_of(int NW) { return 8 * NW + 4; }
constexpr int kLongCin = 256;                // from here on a block has 8 waves: half the K steps per wave
constexpr int kTN = 32;                      // output channels of a block
constexpr int kRP = kTN + 1;                 // row pitch of the partial tiles

struct ConvArgs {
  Src src;
  const float* packed;
  const float *gamma, *beta, *mean, *var;
  float eps;
  float* y;
  int32_t Cout, G, NT, TX;
};

template <int KIND, int V, int NW>
__global__ __launch_bounds__(64 * NW) void unet_conv3x3_kernel(const ConvArgs s) {
  constexpr int kKC = chunk_of(NW), kXP = pitch_of(NW);
  __shared__ __align__(16) float Xs[kHP * kXP];
  __shared__ float red[NW * 32 * kRP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = blockIdx.x % s.NT;
  const int tile = blockIdx.x / s.NT;
  const int y0 = (tile / s.TX) * kTH, x0 = (tile % s.TX) * kTW;
  const int64_t b = blockIdx.y;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  const int p = lane & 31, h = lane >> 5;
  const float* ap = Xs + ((p >> 3) * kHW + (p & 7)) * kXP + 8 * wave + 4 * h;
  const float4* wp = reinterpret_cast<const float4*>(s.packed) + ((int64_t)nt * 9 * s.G) * 64 + lane;

  const int nchunks = (s.src.Cin + kKC - 1) / kKC;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int g = ch * NW + wave;
    const bool live = g < s.G;  // wave-uniform
    float4 bw[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) bw[t] = live ? wp[((int64_t)t * s.G + g) * 64] : make_float4(0.f, 0.f, 0.f, 0.f);

    stage_halo<KIND, V, 64 * NW>(Xs, kXP, s.src, b, y0, x0, ch * kKC, kKC, tid);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float4 a = *reinterpret_cast<const float4*>(ap + ((t / 3) * kHW + (t % 3)) * kXP);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bw[t].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bw[t].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bw[t].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bw[t].w, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // the waves' partial tiles, then (w0 + w1) + (w2 + w3) (+ the same of w4 .. w7)
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 32 + d_row(r, lane)) * kRP + (lane & 31)] = acc[r];
  __syncthreads();
  const int op = tid >> 3, j0 = (tid & 7) * 4;
  const int oy = y0 + (op >> 3), ox = x0 + (op & 7);
  const int co = nt * kTN + j0;
  if (tid < 256 && oy < s.src.H && ox < s.src.W && co < s.Cout) {  // Cout % 4 == 0: four channels are inside or outside together
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* q = red + op * kRP + j0 + k;
      float v = (q[0] + q[32 * kRP]) + (q[2 * 32 * kRP] + q[3 * 32 * kRP]);
      if constexpr (NW == 8) v += (q[4 * 32 * kRP] + q[5 * 32 * kRP]) + (q[6 * 32 * kRP] + q[7 * 32 * kRP]);
      if (s.gamma) {
        const float sc = s.gamma[co + k] / sqrtf(s.var[co + k] + s.eps);
        v = gelu_erf((v - s.mean[co + k]) * sc + s.beta[co + k]);
      }
      o[k] = v;
    }
    *reinterpret_cast<float4*>(s.y + ((b * s.src.H + oy) * s.src.W + ox) * s.Cout + co) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// packed[(((nt * 9 + t) * G + g) * 64 + lane) * 4 + q] = w[co = 32 nt + (lane & 31)][ci = 8 g + 4 (lane >> 5) + q][t]
__global__ __launch_bounds__(256) void unet_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int Cin,
                                                        int Cout, int G, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i & 3), lane = (int)((i >> 2) & 63);
    int64_t r = i >> 8;
    const int g = (int)(r % G);
    r /= G;
    const int t = (int)(r % 9), nt = (int)(r / 9);
    const int co = 32 * nt + (lane & 31), ci = 8 * g + 4 * (lane >> 5) + q;
    packed[i] = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * 9 + t] : 0.f;
  }
}

__global__ __launch_bounds__(256) void unet_conv1x1_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* residual,
                                                               int64_t res_bs, float* __restrict__ y, int64_t HW, int F,
                                                               int Cout, int ngroups, int64_t total) {
  // an item is a pixel and four output channels (pixels fastest: a wave shares its weights and stores contiguously);
  // the pixel's row is read once per item, every channel's products are added in ascending f
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t pix = i % HW, bg = i / HW;
    const int co = (int)(bg % ngroups) * 4;
    const int64_t b = bg / ngroups;
    const float* xr = x + (b * HW + pix) * F;
    const float* wr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wr[k] = w + (int64_t)(co + k < Cout ? co + k : Cout - 1) * F;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < F; f += 4) {
      const float4 xv = gcl::ld4(xr + f);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4 wv = gcl::ld4(wr[k] + f);
        acc[k] = __builtin_fmaf(xv.x, wv.x, acc[k]);
        acc[k] = __builtin_fmaf(xv.y, wv.y, acc[k]);
        acc[k] = __builtin_fmaf(xv.z, wv.z, acc[k]);
        acc[k] = __builtin_fmaf(xv.w, wv.w, acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (co + k < Cout) {
        float v = gcl::rounded(acc[k] + bias[co + k]);
        if (residual) v = v + residual[b * res_bs + (int64_t)(co + k) * HW + pix];
        y[(b * Cout + co + k) * HW + pix] = v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void cascade_pack_kernel(const float* __restrict__ coarse, const float* __restrict__ gm,
                                                           const float* __restrict__ gs, const float* __restrict__ dm,
                                                           const float* __restrict__ ds, const float* __restrict__ stat,
                                                           float* __restrict__ phys, float* __restrict__ X, int B, int H,
                                                           int W, int C, int obs, int Ns) {
  const int64_t HW = (int64_t)H * W, n_dyn = (int64_t)B * HW * C, total = n_dyn + (int64_t)B * HW * Ns;
  const int64_t CX = (int64_t)obs * C + Ns;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (i < n_dyn) {
      const int c = (int)(i % C);
      const int64_t pix = (i / C) % HW, b = i / (C * HW);
      const float ph = gcl::rounded(coarse[i] * gs[c]) + gm[c];
      phys[i] = ph;
      const float nv = gcl::rounded(ph - dm[c]) / ds[c];
      for (int o = 0; o < obs; ++o) X[(b * CX + (int64_t)o * C + c) * HW + pix] = nv;
    } else {
      const int64_t j = i - n_dyn;  // (b, s, y, x), x fastest: the stores are contiguous
      const int x = (int)(j % W), y = (int)((j / W) % H);
      const int sidx = (int)((j / HW) % Ns);
      const int64_t b = j / (HW * Ns);
      X[(b * CX + (int64_t)obs * C + sidx) * HW + (int64_t)y * W + x] = stat[((int64_t)x * H + y) * Ns + sidx];
    }
  }
}

// Stage 1 of the scores: block (chunk, column tile, sample) adds the rows (pixels, y-major) of its chunk for 32 channels.
// part [B][C][3][nchunk]
__global__ __launch_bounds__(256) void cascade_scores_part_kernel(const float* __restrict__ out, const float* __restrict__ phys,
                                                                  const __half* __restrict__ fine, int T, int n_feat,
                                                                  const int64_t* __restrict__ t_fine,
                                                                  const int64_t* __restrict__ t_persist,
                                                                  const float* __restrict__ dm, const float* __restrict__ ds,
                                                                  double* __restrict__ part, int H, int W, int C, int rows_per,
                                                                  int nchunk) {
  __shared__ double red[3][256];
  const int tid = threadIdx.x, col = tid & (gcl::kColTile - 1), rl = tid / gcl::kColTile;
  const int c = blockIdx.y * gcl::kColTile + col;
  const int64_t b = blockIdx.z;
  const int64_t tf = t_fine[b], tp = t_persist[b];
  const bool ok = tf >= 0 && tf < T && tp >= 0 && tp < T;  // block-uniform
  const int n = H * W;
  const int r0 = blockIdx.x * rows_per, r1 = (r0 + rows_per) < n ? (r0 + rows_per) : n;
  double acc[3] = {0.0, 0.0, 0.0};
  if (ok && c < C) {
    const float m = dm[c], sd = ds[c];
    for (int r = r0 + rl; r < r1; r += gcl::kRowLanes) {
      const int y = r / W, x = r % W;
      const int64_t fo = ((int64_t)x * H + y) * n_feat + c;
      const float f = __half2float(fine[tf * W * H * n_feat + fo]);
      const float pe = __half2float(fine[tp * W * H * n_feat + fo]);
      const float casc = gcl::rounded(out[(b * C + c) * n + r] * sd) + m;
      const float dg = phys[(b * n + r) * C + c] - f, dc = casc - f, dp = pe - f;
      acc[0] += (double)gcl::rounded(dg * dg);
      acc[1] += (double)gcl::rounded(dc * dc);
      acc[2] += (double)gcl::rounded(dp * dp);
    }
  }
  const bool writer = rl == 0 && c < C;
  double* dst = part + ((b * C + (c < C ? c : 0)) * 3) * nchunk + blockIdx.x;
  gcl::lanes_to_part<3, 256>(red, acc, tid, gcl::kRowLanes, gcl::kColTile, writer, dst, nchunk);
}

// Stage 2: one wave per channel; the samples one after the other in batch order
__global__ __launch_bounds__(64) void cascade_scores_final_kernel(const double* __restrict__ part, int T,
                                                                  const int64_t* __restrict__ t_fine,
                                                                  const int64_t* __restrict__ t_persist,
                                                                  double* __restrict__ state, int64_t* __restrict__ count,
                                                                  int step, int B, int C, int n, int nchunk) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double* st = state + ((int64_t)step * C + c) * 3;
  double v[3] = {st[0], st[1], st[2]};
  int64_t scored = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t tf = t_fine[b], tp = t_persist[b];
    if (!(tf >= 0 && tf < T && tp >= 0 && tp < T)) continue;
    double S[3];
    gcl::wave_strided_sum<3>(part + ((b * C + c) * 3) * nchunk, nchunk, lane, S);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += S[k] / (double)n;
    ++scored;
  }
  if (lane == 0) {
    st[0] = v[0], st[1] = v[1], st[2] = v[2];
    if (c == 0) count[step] += scored;
  }
}

template <int KIND, int NW>
void launch_conv_nw(const ConvArgs& a, bool vec, dim3 grid, hipStream_t st) {
  if constexpr (KIND != GCL_UNET_SRC_PLANAR) {
    if (vec) {
      hipLaunchKernelGGL((unet_conv3x3_kernel<KIND, 4, NW>), grid, dim3(64 * NW), 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((unet_conv3x3_kernel<KIND, 1, NW>), grid, dim3(64 * NW), 0, st, a);
}
// the block shape is a function of Cin alone: the order of every sum stays a function of the layer's shape
template <int KIND>
void launch_conv(const ConvArgs& a, bool vec, dim3 grid, hipStream_t st) {
  if (a.src.Cin >= kLongCin) launch_conv_nw<KIND, 8>(a, vec, grid, st);
  else launch_conv_nw<KIND, 4>(a, vec, grid, st);
}

}  // namespace

extern "C" {

int64_t gcl_unet_launches(void) { return g_launches.load(); }

int64_t gcl_unet_packed_floats(int32_t Cin, int32_t Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  return gcl::cdiv(Cout, kTN) * 9 * gcl::cdiv(Cin, 8) * 256;
}

int gcl_unet_pack_weights(const float* w, int32_t Cin, int32_t Cout, float* packed, gcl_stream_t stream) {
  GCL_CHECK_ARG(w && packed, "gcl_unet_pack_weights: null pointer");
  GCL_CHECK_ARG(Cin >= 1 && Cout >= 1, "gcl_unet_pack_weights: Cin %d, Cout %d", Cin, Cout);
  const int64_t total = gcl_unet_packed_floats(Cin, Cout);
  hipLaunchKernelGGL(unet_pack_kernel, dim3(gcl::grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, packed, Cin, Cout,
                     (int)gcl::cdiv(Cin, 8), total);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_conv3x3(const gcl_unet_src_t* src, const float* packed, const float* gamma, const float* beta,
                     const float* mean, const float* var, float eps, float* y, int32_t B, int32_t H, int32_t W,
                     int32_t Cin, int32_t Cout, gcl_stream_t stream) {
  GCL_CHECK_ARG(packed && y, "gcl_unet_conv3x3: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 4 && Cout % 4 == 0,
                "gcl_unet_conv3x3: B %d, H %d, W %d, Cin %d, Cout %d (Cout must be a multiple of 4, B <= 65535)", B, H, W,
                Cin, Cout);
  GCL_CHECK_ARG(gcl::aligned16(y) && gcl::aligned16(packed), "gcl_unet_conv3x3: y and packed must be 16-byte aligned");
  GCL_CHECK_ARG(!gamma || (beta && mean && var), "gcl_unet_conv3x3: gamma without beta / mean / var");
  ConvArgs a{};
  bool vec;
  if (const int rc = gcl::unet_src::bind(src, H, W, Cin, "gcl_unet_conv3x3", a.src, vec)) return rc;
  a.packed = packed, a.gamma = gamma, a.beta = beta, a.mean = mean, a.var = var, a.eps = eps, a.y = y, a.Cout = Cout;
  a.G = (int)gcl::cdiv(Cin, 8), a.NT = (int)gcl::cdiv(Cout, kTN), a.TX = (int)gcl::cdiv(W, kTW);
  const int64_t blocks = gcl::cdiv(H, kTH) * a.TX * a.NT;
  GCL_CHECK_ARG(blocks <= 0x7fffffff, "gcl_unet_conv3x3: %lld blocks per sample", (long long)blocks);
  const dim3 grid((unsigned)blocks, (unsigned)B);
  const int rc = gcl::unet_src::with_kind(src->kind, [&](auto K) {
    launch_conv<decltype(K)::value>(a, vec, grid, (hipStream_t)stream);
    return GCL_OK;
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_unet_conv1x1_out(const float* x, const float* w, const float* bias, const float* residual, int64_t res_bs,
                         float* y, int32_t B, int32_t H, int32_t W, int32_t F, int32_t Cout, gcl_stream_t stream) {
  GCL_CHECK_ARG(x && w && bias && y, "gcl_unet_conv1x1_out: null pointer");
  GCL_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && F >= 4 && F % 4 == 0 && Cout >= 1,
                "gcl_unet_conv1x1_out: B %d, H %d, W %d, F %d (a multiple of 4), Cout %d", B, H, W, F, Cout);
  GCL_CHECK_ARG(gcl::aligned16(x) && gcl::aligned16(w), "gcl_unet_conv1x1_out: x and w must be 16-byte aligned");
  const int ngroups = (Cout + 3) / 4;
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * ngroups * HW;
  hipLaunchKernelGGL(unet_conv1x1_out_kernel, dim3(gcl::grid_for(total, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, w,
                     bias, residual, res_bs, y, HW, F, Cout, ngroups, total);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

int gcl_cascade_pack(const float* coarse, const float* gnn_mean, const float* gnn_std, const float* ds_mean,
                     const float* ds_std, const float* static_fine, float* coarse_phys, float* X, int32_t B, int32_t H,
                     int32_t W, int32_t C, int32_t obs, int32_t Ns, gcl_stream_t stream) {
  GCL_CHECK_ARG(coarse && gnn_mean && gnn_std && ds_mean && ds_std && coarse_phys && X, "gcl_cascade_pack: null pointer");
  GCL_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && obs >= 1 && Ns >= 0 && (Ns == 0 || static_fine),
                "gcl_cascade_pack: B %d, H %d, W %d, C %d, obs %d, Ns %d", B, H, W, C, obs, Ns);
  const int64_t total = (int64_t)B * H * W * (C + Ns);
  hipLaunchKernelGGL(cascade_pack_kernel, dim3(gcl::grid_for(total)), dim3(256), 0, (hipStream_t)stream, coarse, gnn_mean,
                     gnn_std, ds_mean, ds_std, static_fine, coarse_phys, X, B, H, W, C, obs, Ns);
  GCL_CHECK_LAUNCH();
  ++g_launches;
  return GCL_OK;
}

size_t gcl_cascade_scores_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || (int64_t)H * W > 0x7fffffff) return 0;
  return (size_t)B * C * 3 * gcl::num_chunks(H * W) * sizeof(double);
}

int gcl_cascade_scores(const float* out, const float* coarse_phys, const void* fine, int32_t T, int32_t n_feat,
                       const int64_t* t_fine, const int64_t* t_persist, const float* ds_mean, const float* ds_std,
                       double* state, int64_t* count, int32_t step, int32_t AR, int32_t B, int32_t H, int32_t W,
                       int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(out && coarse_phys && fine && t_fine && t_persist && ds_mean && ds_std && state && count && ws,
                "gcl_cascade_scores: null pointer");
  GCL_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff && C >= 1 && n_feat >= C && T >= 1,
                "gcl_cascade_scores: B %d, H %d, W %d, C %d, n_feat %d, T %d", B, H, W, C, n_feat, T);
  GCL_CHECK_ARG(step >= 0 && step < AR, "gcl_cascade_scores: step %d of %d", step, AR);
  GCL_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gcl_cascade_scores: ws must be 8-byte aligned");
  if (ws_bytes < gcl_cascade_scores_ws_bytes(B, H, W, C)) {
    gcl::set_error("gcl_cascade_scores: workspace of %zu bytes, %zu needed", ws_bytes, gcl_cascade_scores_ws_bytes(B, H, W, C));
    return GCL_ENOMEM;
  }
  const int n = H * W, rows_per = gcl::chunk_rows(n), nchunk = gcl::num_chunks(n);
  const hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(cascade_scores_part_kernel, dim3(nchunk, (unsigned)gcl::cdiv(C, gcl::kColTile), B), dim3(256), 0, st, out,
                     coarse_phys, (const __half*)fine, T, n_feat, t_fine, t_persist, ds_mean, ds_std, part, H, W, C, rows_per,
                     nchunk);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(cascade_scores_final_kernel, dim3(C), dim3(64), 0, st, part, T, t_fine, t_persist, state, count, step, B,
                     C, n, nchunk);
  GCL_CHECK_LAUNCH();
  g_launches += 2;
  return GCL_OK;
}

}  // extern "C"
