// The row arithmetic of the node LayerNorm forward, shared by the plain 16-byte-row instantiations of ln_fwd_kernel
// (norm.hip) and the LayerNorm epilogue of the chained MLP forward (linear_x3.hip), so a row gets the same bits from
// either.  Every rounding is written out (fmaf where one is meant, contraction off for the rest): left to the compiler,
// two kernels fuse these expressions differently and their results differ in the last bit.  The fused operations are
// the ones ln_fwd_kernel<LPR, true> has always been compiled to.
#pragma once
#include "common.h"

#ifdef __HIPCC__
namespace gcl {
namespace ln {

// sum over the LPR lanes that hold one row (LPR consecutive lanes, a power of two)
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One row held by LPR lanes, four columns c0 .. c0 + 3 a lane (x = 0 in the columns past F):
// y = (x - mean) * rstd * gamma + beta, and the row's (mean, rstd).
template <int LPR>
__device__ __forceinline__ void fwd_row(float x0, float x1, float x2, float x3, int c0, int F, float invF, float eps,
                                        float g0, float g1, float g2, float g3, float b0, float b1, float b2, float b3,
                                        float& mean, float& rstd, float& y0, float& y1, float& y2, float& y3) {
#pragma clang fp contract(off)
  const float s = group_sum<LPR>(x0 + x1 + x2 + x3);
  mean = s * invF;
  // the first two columns subtract the unrounded mean (one fused operation), the other two the rounded one
  const float d0 = (c0 < F) ? fmaf(-invF, s, x0) : 0.f, d1 = (c0 + 1 < F) ? fmaf(-invF, s, x1) : 0.f;
  const float d2 = (c0 + 2 < F) ? x2 - mean : 0.f, d3 = (c0 + 3 < F) ? x3 - mean : 0.f;
  const float q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
  const float sq = (q0 + q1) + (q2 + q3);
  rstd = 1.0f / sqrtf(fmaf(group_sum<LPR>(sq), invF, eps));
  y0 = fmaf(d0 * rstd, g0, b0);
  y1 = fmaf(d1 * rstd, g1, b1);
  y2 = fmaf(d2 * rstd, g2, b2);
  y3 = fmaf(d3 * rstd, g3, b3);
}

}  // namespace ln
}  // namespace gcl
#endif
