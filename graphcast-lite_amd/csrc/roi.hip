// ROI residual head glue (src/roi_residual.py:165-169,183-185): the row gather that builds the head's skip input and
// the composition of the global prediction with the ROI correction.  Both are memory-bound row copies.
#include "common.h"

namespace {

constexpr int kRoiBlocks = 2048;  // grid cap of the streaming kernels (8 blocks of 256 per CU), grid-stride beyond

inline unsigned roi_grid(int64_t total) {
  int64_t nb = gcl::cdiv(total > 0 ? total : 1, 256);
  return (unsigned)(nb > kRoiBlocks ? kRoiBlocks : nb);
}

// dst[b, i, 4q .. 4q+3] for one 16-byte quad: the columns come from [s0 | s1 | s2 | 0] at source row g.  The sources
// start at arbitrary column offsets of the destination row (38 + 256 + 19 at the roi_residual_krsk shape), so their
// loads are per column - adjacent lanes still read adjacent addresses of one source row - and the store is one
// 16-byte vector.
struct Src3 {
  const float* p[3];
  int64_t ld[3], bs[3];
  int32_t w[3];
};

__global__ __launch_bounds__(256) void roi_gather_kernel(const int32_t* __restrict__ rows, int32_t n, int32_t rows_src,
                                                         Src3 s, float* __restrict__ dst, int64_t ldd, int64_t bsd,
                                                         int32_t Q, int32_t B) {
  const int64_t total = (int64_t)B * n * Q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int e1 = s.w[0], e2 = s.w[0] + s.w[1], e3 = s.w[0] + s.w[1] + s.w[2];
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int q = (int)(t % Q);
    const int64_t r = t / Q;
    const int i = (int)(r % n);
    const int64_t b = r / n;
    const int g = rows ? rows[i] : i;
    const bool ok = g >= 0 && g < rows_src;  // a bad index reads nothing (the row is written as zeros)
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      float x = 0.f;
      if (ok) {
        if (c < e1)
          x = s.p[0][b * s.bs[0] + (int64_t)g * s.ld[0] + c];
        else if (c < e2)
          x = s.p[1][b * s.bs[1] + (int64_t)g * s.ld[1] + (c - e1)];
        else if (c < e3)
          x = s.p[2][b * s.bs[2] + (int64_t)g * s.ld[2] + (c - e2)];
      }
      v[j] = x;
    }
    *reinterpret_cast<float4*>(dst + b * bsd + (int64_t)i * ldd + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// out[b, g, c] = pred[b, g, c] + (0 + corr[b, pos[g], c]) for ROI rows (pos[g] >= 0), pred[b, g, c] elsewhere: the
// reference's `pred + zeros.index_add(0, roi, corr)` without the [G, C] zero tensor.  Rows outside the ROI are copied,
// never added to, so they stay bit-equal to pred (a +0 would turn -0 into +0).
// VEC: pred and out are dense [B, G, C] and 16-B aligned, so the B*G*C elements are walked as 16-byte quads of one
// flat array (the last quad may be partial); otherwise one element per step with the given strides.
template <bool VEC>
__global__ __launch_bounds__(256) void roi_compose_kernel(const float* __restrict__ pred, int64_t ldp, int64_t bsp,
                                                          const float* __restrict__ corr, int64_t ldc, int64_t bsc,
                                                          const int32_t* __restrict__ pos, float* __restrict__ out,
                                                          int64_t ldo, int64_t bso, int32_t B, int32_t G, int32_t C) {
  const int64_t total = (int64_t)B * G * C;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t start = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const int64_t nq = (total + 3) / 4;
    for (int64_t t = start; t < nq; t += stride) {
      const int64_t k0 = 4 * t;
      int c = (int)(k0 % C);
      int64_t r = k0 / C;  // flat row b * G + g
      const bool full = k0 + 4 <= total;
      float v[4];
      if (full) {
        const float4 p4 = *reinterpret_cast<const float4*>(pred + k0);
        v[0] = p4.x, v[1] = p4.y, v[2] = p4.z, v[3] = p4.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < total ? pred[k0 + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int g = (int)(r % G);
        const int p = pos[g];
        if (p >= 0 && k0 + j < total) v[j] = v[j] + (0.f + corr[(r / G) * bsc + (int64_t)p * ldc + c]);
        if (++c == C) c = 0, ++r;
      }
      if (full) {
        *reinterpret_cast<float4*>(out + k0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k0 + j < total) out[k0 + j] = v[j];
      }
    }
  } else {
    for (int64_t k = start; k < total; k += stride) {
      const int c = (int)(k % C);
      const int64_t r = k / C;
      const int g = (int)(r % G);
      const int64_t b = r / G;
      float v = pred[b * bsp + (int64_t)g * ldp + c];
      const int p = pos[g];
      if (p >= 0) v = v + (0.f + corr[b * bsc + (int64_t)p * ldc + c]);
      out[b * bso + (int64_t)g * ldo + c] = v;
    }
  }
}

}  // namespace

extern "C" int gcl_roi_gather_rows(const int32_t* rows, int32_t n, int32_t rows_src, const float* s0, int64_t ld0,
                                   int64_t bs0, int32_t w0, const float* s1, int64_t ld1, int64_t bs1, int32_t w1,
                                   const float* s2, int64_t ld2, int64_t bs2, int32_t w2, float* dst, int64_t ldd,
                                   int64_t bsd, int32_t Fp, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(dst && B > 0 && n >= 0 && rows_src >= 0, "roi_gather_rows: bad argument");
  GCL_CHECK_ARG(w0 >= 0 && w1 >= 0 && w2 >= 0 && (!w0 || (s0 && ld0 >= w0)) && (!w1 || (s1 && ld1 >= w1)) &&
                    (!w2 || (s2 && ld2 >= w2)),
                "roi_gather_rows: a source is missing or narrower than its width");
  GCL_CHECK_ARG(rows || n <= rows_src, "roi_gather_rows: identity map with more rows (%d) than the source has (%d)", n,
                rows_src);
  GCL_CHECK_ARG(Fp % 4 == 0 && Fp >= w0 + w1 + w2 && ldd >= Fp,
                "roi_gather_rows: Fp=%d must be a multiple of 4 covering %d columns, ldd=%lld", Fp, w0 + w1 + w2,
                (long long)ldd);
  GCL_CHECK_ARG(ldd % 4 == 0 && bsd % 4 == 0 && gcl::aligned16(dst), "roi_gather_rows: destination rows must be 16-B aligned");
  GCL_CHECK_ARG(B == 1 || bsd >= (int64_t)n * ldd, "roi_gather_rows: destination samples overlap");
  if (n == 0 || Fp == 0) return GCL_OK;
  Src3 s{{s0, s1, s2}, {ld0, ld1, ld2}, {bs0, bs1, bs2}, {w0, w1, w2}};
  const int64_t total = (int64_t)B * n * (Fp / 4);
  hipLaunchKernelGGL(roi_gather_kernel, dim3(roi_grid(total)), dim3(256), 0, (hipStream_t)stream, rows, n, rows_src, s,
                     dst, ldd, bsd, Fp / 4, B);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_roi_compose(const float* pred, int64_t ldp, int64_t bsp, const float* corr, int64_t ldc, int64_t bsc,
                               const int32_t* pos, float* out, int64_t ldo, int64_t bso, int32_t B, int32_t G, int32_t C,
                               gcl_stream_t stream) {
  GCL_CHECK_ARG(pred && corr && pos && out, "roi_compose: null argument");
  GCL_CHECK_ARG(B > 0 && G >= 0 && C > 0 && ldp >= C && ldc >= C && ldo >= C, "roi_compose: bad shape");
  GCL_CHECK_ARG(B == 1 || (bsp >= (int64_t)G * ldp && bso >= (int64_t)G * ldo), "roi_compose: samples overlap");
  const int64_t total = (int64_t)B * G * C;
  if (total == 0) return GCL_OK;
  const bool vec = ldp == C && ldo == C && (B == 1 || (bsp == (int64_t)G * C && bso == (int64_t)G * C)) &&
                   gcl::aligned16(pred) && gcl::aligned16(out);
  if (vec)
    hipLaunchKernelGGL(roi_compose_kernel<true>, dim3(roi_grid(gcl::cdiv(total, 4))), dim3(256), 0, (hipStream_t)stream,
                       pred, ldp, bsp, corr, ldc, bsc, pos, out, ldo, bso, B, G, C);
  else
    hipLaunchKernelGGL(roi_compose_kernel<false>, dim3(roi_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, ldp,
                       bsp, corr, ldc, bsc, pos, out, ldo, bso, B, G, C);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
