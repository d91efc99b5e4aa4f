// How a WeatherUNet 3x3 convolution reads its input (gcl_unet_src_t of gcl.h): the one copy of the source read, shared by
// the forward convolution (unet.hip) and the weight gradient (unet_train.hip).  MaxPool2d(2), the bilinear Upsample, the
// pad to the skip's size and the concatenation are never tensors: they are `src_read`.
#pragma once
#include "common.h"

namespace gcl {
namespace unet_src {

template <int V>
struct Vec {
  float v[V];
};
template <int V>
__device__ __forceinline__ Vec<V> ldv(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

// torch's max_pool2d update: a NaN replaces the running maximum and then stays
__device__ __forceinline__ bool pool_takes(float m, float v) { return v > m || v != v; }
__device__ __forceinline__ float pool_take(float m, float v) { return pool_takes(m, v) ? v : m; }

// The bilinear weights of destination index d (align_corners=True, scale s = (in - 1) / (out - 1) in float32, as torch
// forms it): i0 = floor(s d), i1 = min(i0 + 1, n - 1), l = s d - i0, h = 1 - l.  One rule for the read and its adjoint.
struct Lerp {
  int i0, i1;
  float l, h;
};
__device__ __forceinline__ Lerp lerp_of(float s, int d, int n) {
  const float f = s * (float)d;
  Lerp r;
  r.i0 = (int)f;
  r.i1 = r.i0 + (r.i0 < n - 1 ? 1 : 0);
  r.l = f - (float)r.i0;
  r.h = 1.f - r.l;
  return r;
}

// V channels c .. c+V-1 (all < Cin, and on one side of C1) of input pixel (y, x) of sample b; 0 <= y < H, 0 <= x < W.
// S: a struct with the fields a, b, C1, C2, Hs, Ws, sy, sx, H, W, Cin.
template <int KIND, int V, class S>
__device__ __forceinline__ Vec<V> src_read(const S& s, int64_t b, int y, int x, int c) {
  if constexpr (KIND == GCL_UNET_SRC_PLANAR) {
    static_assert(V == 1, "planar sources are read channel by channel");
    return ldv<1>(s.a + ((b * s.Cin + c) * s.H + y) * s.W + x);
  } else if constexpr (KIND == GCL_UNET_SRC_ROWS) {
    return ldv<V>(s.a + ((b * s.H + y) * s.W + x) * s.Cin + c);
  } else if constexpr (KIND == GCL_UNET_SRC_POOL) {
    const float* p = s.a + ((b * s.Hs + 2 * y) * s.Ws + 2 * x) * s.Cin + c;
    const int64_t row = (int64_t)s.Ws * s.Cin;
    const Vec<V> v00 = ldv<V>(p), v01 = ldv<V>(p + s.Cin), v10 = ldv<V>(p + row), v11 = ldv<V>(p + row + s.Cin);
    Vec<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float m = -INFINITY;
      m = pool_take(m, v00.v[i]);
      m = pool_take(m, v01.v[i]);
      m = pool_take(m, v10.v[i]);
      m = pool_take(m, v11.v[i]);
      r.v[i] = m;
    }
    return r;
  } else {
    if (c < s.C1) return ldv<V>(s.a + ((b * s.H + y) * s.W + x) * s.C1 + c);
    Vec<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = 0.f;
    if (y >= 2 * s.Hs || x >= 2 * s.Ws) return r;  // the pad to the skip's size
    const float fy = s.sy * (float)y, fx = s.sx * (float)x;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < s.Hs - 1 ? 1 : 0), x1 = x0 + (x0 < s.Ws - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float* base = s.b + b * s.Hs * s.Ws * s.C2 + (c - s.C1);
    const Vec<V> v00 = ldv<V>(base + ((int64_t)y0 * s.Ws + x0) * s.C2), v01 = ldv<V>(base + ((int64_t)y0 * s.Ws + x1) * s.C2),
                 v10 = ldv<V>(base + ((int64_t)y1 * s.Ws + x0) * s.C2), v11 = ldv<V>(base + ((int64_t)y1 * s.Ws + x1) * s.C2);
#pragma unroll
    for (int i = 0; i < V; ++i)
      r.v[i] = hy * (hx * v00.v[i] + lx * v01.v[i]) + ly * (hx * v10.v[i] + lx * v11.v[i]);
    return r;
  }
}

// The scales of an UPCAT source, (in - 1) / (out - 1) per axis in float32
inline float upcat_scale(int n) { return (float)(n - 1) / (float)(2 * n - 1); }

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

}  // namespace unet_src
}  // namespace gcl
