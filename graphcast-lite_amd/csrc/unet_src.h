// How a U-Net convolution reads its input (gcl_unet_src_t of gcl.h), in one copy for the forward convolution
// (unet.hip), the weight gradient (unet_train.hip) and the pointwise convolution (unet_v2.hip): the device view `Src`,
// the host `bind` that checks a descriptor and fills the view, `with_kind` that turns the kind into a template constant,
// `src_read`, and the 6 x 10 halo image `stage_halo` puts in LDS.  MaxPool2d(2), the bilinear Upsample, the pad to the
// skip's size and the concatenation are never tensors: they are `src_read`.
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

// The device view of a source: the descriptor's fields, the UPCAT scales and the shape of the virtual input
struct Src {
  const float* a;
  const float* b;
  int32_t C1, C2, Hs, Ws;
  float sy, sx;  // UPCAT: (in - 1) / (out - 1) per axis, in float32 as torch forms it
  int32_t H, W, Cin;
};

// V channels c .. c+V-1 (all < Cin, and on one side of C1) of input pixel (y, x) of sample b; 0 <= y < H, 0 <= x < W.
template <int KIND, int V>
__device__ __forceinline__ Vec<V> src_read(const Src& s, int64_t b, int y, int x, int c) {
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
    const Lerp ly = lerp_of(s.sy, y, s.Hs), lx = lerp_of(s.sx, x, s.Ws);
    const float* base = s.b + b * s.Hs * s.Ws * s.C2 + (c - s.C1);
    const Vec<V> v00 = ldv<V>(base + ((int64_t)ly.i0 * s.Ws + lx.i0) * s.C2),
                 v01 = ldv<V>(base + ((int64_t)ly.i0 * s.Ws + lx.i1) * s.C2),
                 v10 = ldv<V>(base + ((int64_t)ly.i1 * s.Ws + lx.i0) * s.C2),
                 v11 = ldv<V>(base + ((int64_t)ly.i1 * s.Ws + lx.i1) * s.C2);
#pragma unroll
    for (int i = 0; i < V; ++i)
      r.v[i] = ly.h * (lx.h * v00.v[i] + lx.l * v01.v[i]) + ly.l * (lx.h * v10.v[i] + lx.l * v11.v[i]);
    return r;
  }
}

// The tile of the 3x3 kernels: 4 x 8 output pixels (the 32 rows of one MFMA tile), 6 x 10 staged with the halo
constexpr int kTH = 4, kTW = 8;
constexpr int kHH = kTH + 2, kHW = kTW + 2;
constexpr int kHP = kHH * kHW;

// Channels c0 .. c0+nchan-1 of the kHP pixels around the tile at (y0, x0) of sample b into lds[pixel * pitch + channel],
// through the source kind: zero outside the image and past Cin, V channels per item.  Every thread of the block calls it
// with constant pitch and nchan (nchan % V == 0; V == 4: pitch % 4 == 0 and lds 16-byte aligned).
template <int KIND, int V, int NTHREADS>
__device__ __forceinline__ void stage_halo(float* lds, int pitch, const Src& s, int64_t b, int y0, int x0, int c0, int nchan,
                                           int tid) {
  const int per = nchan / V;
  for (int idx = tid; idx < kHP * per; idx += NTHREADS) {
    const int px = idx / per, cc = (idx % per) * V;
    const int y = y0 - 1 + px / kHW, x = x0 - 1 + px % kHW;
    const int c = c0 + cc;
    Vec<V> v;
#pragma unroll
    for (int i = 0; i < V; ++i) v.v[i] = 0.f;
    if (y >= 0 && y < s.H && x >= 0 && x < s.W && c < s.Cin) v = src_read<KIND, V>(s, b, y, x, c);
    float* d = lds + px * pitch + cc;
    if constexpr (V == 4) {
      st4(d, make_float4(v.v[0], v.v[1], v.v[2], v.v[3]));
    } else {
      *d = v.v[0];
    }
  }
}

// The scales of an UPCAT source, (in - 1) / (out - 1) per axis in float32
inline float upcat_scale(int n) { return (float)(n - 1) / (float)(2 * n - 1); }

// The view of `src` as the H x W x Cin input of entry point `who`, or the refusal.  vec: the 16-byte read (V = 4) is
// legal - whole groups of four channels on one side of C1, at aligned addresses; never for a planar source.
inline int bind(const gcl_unet_src_t* src, int H, int W, int Cin, const char* who, Src& out, bool& vec) {
  GCL_CHECK_ARG(src && src->a, "%s: null pointer", who);
  out = Src{src->a, src->b, src->C1, src->C2, src->Hs, src->Ws, 0.f, 0.f, H, W, Cin};
  vec = Cin % 4 == 0 && aligned16(src->a);
  switch (src->kind) {
    case GCL_UNET_SRC_PLANAR:
      vec = false;
      break;
    case GCL_UNET_SRC_ROWS:
      break;
    case GCL_UNET_SRC_POOL:
      GCL_CHECK_ARG(src->Hs / 2 == H && src->Ws / 2 == W, "%s: POOL source %d x %d does not halve to %d x %d", who, src->Hs,
                    src->Ws, H, W);
      break;
    case GCL_UNET_SRC_UPCAT:
      GCL_CHECK_ARG(src->b && src->C1 >= 1 && src->C2 >= 1 && src->C1 + src->C2 == Cin,
                    "%s: UPCAT needs b and C1 + C2 == Cin (C1 %d, C2 %d, Cin %d)", who, src->C1, src->C2, Cin);
      GCL_CHECK_ARG(src->Hs >= 1 && src->Ws >= 1 && 2 * src->Hs <= H && 2 * src->Ws <= W,
                    "%s: UPCAT low tensor %d x %d does not fit %d x %d", who, src->Hs, src->Ws, H, W);
      out.sy = upcat_scale(src->Hs), out.sx = upcat_scale(src->Ws);
      vec = src->C1 % 4 == 0 && src->C2 % 4 == 0 && aligned16(src->a) && aligned16(src->b);
      break;
    default:
      GCL_CHECK_ARG(false, "%s: source kind %d", who, src->kind);
  }
  return GCL_OK;
}

// f(std::integral_constant<int, KIND>) for the kind of a bound source
template <class F>
int with_kind(int kind, F&& f) {
  return plan::pick<GCL_UNET_SRC_PLANAR, GCL_UNET_SRC_ROWS, GCL_UNET_SRC_POOL, GCL_UNET_SRC_UPCAT>(kind, f);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

}  // namespace unet_src
}  // namespace gcl
