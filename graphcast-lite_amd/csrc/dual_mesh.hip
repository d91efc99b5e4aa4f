// Dual-mesh regional model glue (src/dual_mesh.py): the two edge-wise operations of the regional module that no other
// kernel does.  Both are HBM/L2-bound row traffic on 16-byte rows with int32 CSR indices; every output row has exactly
// one writer and a fixed summation order (no atomics).
//
//   gcl_segment_wsum     : out[b,i,:] (+)= addend[b,i,:] + sum_k w[k] * act(src[b, idx[k], :]),  k in [rowptr[i], rowptr[i+1])
//        forward : RegionalEncoder's scatter(mean) over the encoding edges (w = 1/deg, src/dual_mesh.py:421-425, applied
//                  to the SiLU output before the second Linear) and RegionalDecoder's IDW sum (w = dec_idw_weights,
//                  src/dual_mesh.py:464-468, on the mesh rows already projected by the decoder's mesh weight block)
//        backward: the same two sums through the transposed CSR (same per-edge weights)
//   gcl_cross_update_fwd : pre = h + (1/deg) sum_k msg[k];  y = LayerNorm_node(pre)   (src/dual_mesh.py:356-357)
//        one wave per regional row; the LayerNorm statistics are saved for gcl_layernorm_bwd, which takes this form
//        unchanged (x = pre)
#include "common.h"

namespace {

using gcl::add4;  // float4 helpers (common.h)
using gcl::ld4;
using gcl::st4;
__device__ __forceinline__ float4 silu4(float4 v) {
  return make_float4(gcl::silu_f(v.x), gcl::silu_f(v.y), gcl::silu_f(v.z), gcl::silu_f(v.w));
}

// LPR lanes per row (power of two <= 64); a row of D floats is ceil(D/4/LPR) float4 per lane.
template <int LPR>
__global__ __launch_bounds__(256) void segment_wsum_kernel(const float* __restrict__ src, int64_t lds_, int64_t bss,
                                                           int32_t n_src, int32_t silu, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ w, const int32_t* __restrict__ rowptr,
                                                           const float* __restrict__ addend, int64_t lda, int64_t bsa,
                                                           float* __restrict__ out, int64_t ldo, int64_t bso,
                                                           int32_t accumulate, int32_t B, int32_t n, int32_t D4) {
  constexpr int GPB = 256 / LPR;  // row groups per block
  const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const int64_t total = (int64_t)B * n;
  for (int64_t row = (int64_t)blockIdx.x * GPB + grp; row < total; row += (int64_t)gridDim.x * GPB) {
    const int b = (int)(row / n), i = (int)(row - (int64_t)b * n);
    const int k0 = rowptr[i], k1 = rowptr[i + 1];
    const float* sb = src + (int64_t)b * bss;
    float* o = out + (int64_t)b * bso + (int64_t)i * ldo;
    for (int c = sub; c < D4; c += LPR) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = k0; k < k1; ++k) {  // edge order
        const int j = idx ? idx[k] : k;
        if (j < 0 || j >= n_src) continue;  // a bad index contributes nothing (never read out of bounds)
        const float s = w ? w[k] : 1.f;
        float4 v = ld4(sb + (int64_t)j * lds_ + 4 * c);
        if (silu) v = silu4(v);
        acc.x = fmaf(s, v.x, acc.x), acc.y = fmaf(s, v.y, acc.y), acc.z = fmaf(s, v.z, acc.z), acc.w = fmaf(s, v.w, acc.w);
      }
      if (addend) acc = add4(acc, ld4(addend + (int64_t)b * bsa + (int64_t)i * lda + 4 * c));
      if (accumulate) acc = add4(ld4(o + 4 * c), acc);
      st4(o + 4 * c, acc);
    }
  }
}

// One wave per row (D <= 256: 4 columns per lane).  The statistics follow ln_fwd_kernel (norm.hip): mean, then the
// biased variance of the deviations, rstd = 1 / sqrt(var + eps).
__global__ __launch_bounds__(256) void cross_update_fwd_kernel(const float* __restrict__ h, int64_t ldh, int64_t bsh,
                                                               const float* __restrict__ msg, int64_t ldm, int64_t bsm,
                                                               const int32_t* __restrict__ rowptr,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps,
                                                               float* __restrict__ pre, float* __restrict__ y,
                                                               float* __restrict__ stats, int32_t B, int32_t n,
                                                               int32_t D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = 4 * lane;
  const bool on = c0 < D;
  const float invD = 1.f / (float)D;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f), bt = g;
  if (on) g = ld4(gamma + c0), bt = ld4(beta + c0);
  const int64_t total = (int64_t)B * n;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < total; row += (int64_t)gridDim.x * 4) {
    const int b = (int)(row / n), i = (int)(row - (int64_t)b * n);
    const int k0 = rowptr[i], k1 = rowptr[i + 1];
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
      float4 acc = x;
      const float* mb = msg + (int64_t)b * bsm + c0;
      for (int k = k0; k < k1; ++k) acc = add4(acc, ld4(mb + (int64_t)k * ldm));
      const float inv = k1 > k0 ? 1.f / (float)(k1 - k0) : 0.f;  // scatter(mean) of no edges is 0
      const float4 hv = ld4(h + (int64_t)b * bsh + (int64_t)i * ldh + c0);
      x = make_float4(hv.x + acc.x * inv, hv.y + acc.y * inv, hv.z + acc.z * inv, hv.w + acc.w * inv);
      st4(pre + row * D + c0, x);
    }
    const float mean = gcl::wave_sum(x.x + x.y + x.z + x.w) * invD;
    const float d0 = on ? x.x - mean : 0.f, d1 = on ? x.y - mean : 0.f, d2 = on ? x.z - mean : 0.f,
                d3 = on ? x.w - mean : 0.f;
    float sq;
    {
#pragma clang fp contract(off)
      const float q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
      sq = (q0 + q1) + (q2 + q3);
    }
    const float var = gcl::wave_sum(sq) * invD;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (on)
      st4(y + row * D + c0, make_float4(d0 * rstd * g.x + bt.x, d1 * rstd * g.y + bt.y, d2 * rstd * g.z + bt.z,
                                        d3 * rstd * g.w + bt.w));
    if (lane == 0) {
      stats[2 * row] = mean;
      stats[2 * row + 1] = rstd;
    }
  }
}

int lanes_per_row(int D4) { return D4 >= 64 ? 64 : D4 > 16 ? 32 : D4 > 8 ? 16 : 8; }
unsigned rows_grid(int64_t rows, int gpb) {
  const int64_t want = gcl::cdiv(rows, gpb);
  const int64_t cap = (int64_t)gcl::kNumCU * 32;
  return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

}  // namespace

extern "C" int gcl_segment_wsum(const float* src, int64_t ld_src, int64_t bs_src, int32_t n_src, int32_t act,
                                const int32_t* idx, const float* w, const int32_t* rowptr, const float* addend,
                                int64_t ld_add, int64_t bs_add, float* out, int64_t ld_out, int64_t bs_out,
                                int32_t accumulate, int32_t B, int32_t n, int32_t D, gcl_stream_t stream) {
  GCL_CHECK_ARG(src && rowptr && out, "segment_wsum: null argument");
  GCL_CHECK_ARG(B > 0 && n >= 0 && n_src >= 0 && D > 0 && D % 4 == 0, "segment_wsum: D=%d must be a positive multiple of 4",
                D);
  GCL_CHECK_ARG(act == GCL_ACT_NONE || act == GCL_ACT_SILU, "segment_wsum: unsupported activation %d", act);
  GCL_CHECK_ARG(ld_src % 4 == 0 && bs_src % 4 == 0 && ld_src >= D && gcl::aligned16(src),
                "segment_wsum: source rows must be 16-B aligned and at least D wide");
  GCL_CHECK_ARG(ld_out % 4 == 0 && bs_out % 4 == 0 && ld_out >= D && gcl::aligned16(out),
                "segment_wsum: destination rows must be 16-B aligned and at least D wide");
  GCL_CHECK_ARG(!addend || (ld_add % 4 == 0 && bs_add % 4 == 0 && ld_add >= D && gcl::aligned16(addend)),
                "segment_wsum: addend rows must be 16-B aligned and at least D wide");
  GCL_CHECK_ARG(B == 1 || bs_out >= (int64_t)n * ld_out, "segment_wsum: destination samples overlap");
  if (n == 0) return GCL_OK;
  const int D4 = D / 4, lpr = lanes_per_row(D4);
  const unsigned grid = rows_grid((int64_t)B * n, 256 / lpr);
  const int32_t silu = act == GCL_ACT_SILU ? 1 : 0;
#define GCL_SW(L_)                                                                                                  \
  hipLaunchKernelGGL(segment_wsum_kernel<L_>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, ld_src, bs_src, \
                     n_src, silu, idx, w, rowptr, addend, ld_add, bs_add, out, ld_out, bs_out, accumulate, B, n, D4)
  switch (lpr) {
    case 64: GCL_SW(64); break;
    case 32: GCL_SW(32); break;
    case 16: GCL_SW(16); break;
    default: GCL_SW(8); break;
  }
#undef GCL_SW
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_cross_update_fwd(const float* h, int64_t ld_h, int64_t bs_h, const float* msg, int64_t ld_msg,
                                    int64_t bs_msg, const int32_t* rowptr, const float* gamma, const float* beta,
                                    float eps, float* pre, float* y, float* stats, int32_t B, int32_t n, int32_t D,
                                    gcl_stream_t stream) {
  GCL_CHECK_ARG(h && msg && rowptr && gamma && beta && pre && y && stats, "cross_update_fwd: null argument");
  GCL_CHECK_ARG(B > 0 && n >= 0 && D > 0 && D <= 256 && D % 4 == 0,
                "cross_update_fwd: D=%d must be a multiple of 4 in [4, 256]", D);
  GCL_CHECK_ARG(ld_h % 4 == 0 && bs_h % 4 == 0 && ld_h >= D && gcl::aligned16(h) && ld_msg % 4 == 0 &&
                    bs_msg % 4 == 0 && ld_msg >= D && gcl::aligned16(msg),
                "cross_update_fwd: h / msg rows must be 16-B aligned and at least D wide");
  GCL_CHECK_ARG(gcl::aligned16(gamma) && gcl::aligned16(beta) && gcl::aligned16(pre) && gcl::aligned16(y),
                "cross_update_fwd: gamma / beta / outputs must be 16-B aligned");
  if (n == 0) return GCL_OK;
  const int64_t rows = (int64_t)B * n;
  const int64_t want = gcl::cdiv(rows, 4);
  const int64_t cap = (int64_t)gcl::kNumCU * 16;
  hipLaunchKernelGGL(cross_update_fwd_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0,
                     (hipStream_t)stream, h, ld_h, bs_h, msg, ld_msg, bs_msg, rowptr, gamma, beta, eps, pre, y, stats, B,
                     n, D);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
