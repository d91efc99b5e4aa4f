// Per-grid-point error maps (scripts/metrics_maps.py:40-90): RMSE / MAE / bias / ACC at every scored (lead, row,
// channel), accumulated sample by sample in a float64 device state instead of stacking the test set on the host.
//
// Units.  Every value is converted on its own in float32, in the reference's order (inverse_standardize :40-44, then
// apply_units :65-73), each operation rounded alone (gcl::rounded keeps a product out of the add that follows):
//   v = x scale[k];  v = v + mean[k]          (flag kDenorm)
//   v = v / 9.80665f                           (flag kZDiv, a true division: the reciprocal is not bit-equal)
//   v = v factor[k]; v = v + offset[k]
// conv is float [K][4] = {scale, mean, factor, offset}, flags int32 [K], k = lead * C + c; conv NULL: identity.
//
// Column statistics (for ACC, compute_stat :84-89): per sample b and column k the mean and the unbiased standard
// deviation over the scored rows of the converted prediction and truth, in float64.  Sums are shifted by the column's
// first scored row, so a column 1e4 sigma from zero keeps its precision and a constant column has exactly zero
// variance.  Two launches with a fixed order: chunks of rows summed by 8 row lanes, then a column's chunks summed
// by one wave (csrc/colsum.h, which also says why a column's result depends on its own data and n only).
//
// Accumulate.  One thread owns its state elements and adds the B samples of the batch in sample order, so the state
// is read and written once per update and there are no atomics.  State: float64 [lead][sum][row * C + c], sums in the
// order of their bits (kSumE, kSumSq, kSumAbs, kSumPT), only the requested ones present.  The flat kernel reads four
// consecutive values per 16-byte load; the generic one (row list, column map, padded rows) reads one element per
// thread.  Both call add_sample, so they produce the same bits.
#include "colsum.h"
#include "common.h"

namespace {

using gcl::chunk_rows;
using gcl::kColTile;  // at most this many columns per block
using gcl::kRowLanes;
using gcl::num_chunks;
using gcl::rounded;

constexpr int kSumE = 1, kSumSq = 2, kSumAbs = 4, kSumPT = 8;  // sum e, sum e^2, sum |e|, sum p^ t^
constexpr int kDenorm = 1, kZDiv = 2;
constexpr float kG0 = 9.80665f;
constexpr int kKindRmse = 0, kKindSkill = 4;  // 1 mae, 2 bias, 3 acc: the sum over n

constexpr int kColBlock = 512;   // threads of a partial block: as many whole chunks as fit (3 x 152 lanes at K = 19)
constexpr int kPartSums = 4;     // Sp, Spp, St, Stt

struct Conv {
  float scale, mean, factor, offset;
  int flags;  // < 0: identity
};

__device__ __forceinline__ Conv load_conv(const float* __restrict__ conv, const int32_t* __restrict__ flags, int k) {
  Conv cv{1.f, 0.f, 1.f, 0.f, -1};
  if (conv) {
    const float4 v = gcl::ld4(conv + 4 * (int64_t)k);
    cv.scale = v.x, cv.mean = v.y, cv.factor = v.z, cv.offset = v.w;
    cv.flags = flags[k];
  }
  return cv;
}

__device__ __forceinline__ float to_units(float x, const Conv& cv) {
  if (cv.flags < 0) return x;
  float v = x;
  if (cv.flags & kDenorm) v = rounded(rounded(v * cv.scale) + cv.mean);
  if (cv.flags & kZDiv) v = rounded(v / kG0);
  return rounded(v * cv.factor) + cv.offset;
}

// One sample of one element: s = {sum e, sum e^2, sum |e|, sum p^ t^}; cs4 = {mean_p, std_p, mean_t, std_t}.
__device__ __forceinline__ void add_sample(double* s, float vp, float vt, int mask, const double* __restrict__ cs4) {
  const double dp = (double)vp, dt = (double)vt;
  const double e = dp - dt;
  if (mask & kSumE) s[0] += e;
  if (mask & kSumSq) s[1] = fma(e, e, s[1]);
  if (mask & kSumAbs) s[2] += fabs(e);
  if (mask & kSumPT) {
    const double ph = (dp - cs4[0]) / (cs4[1] + 1e-8);
    const double th = (dt - cs4[2]) / (cs4[3] + 1e-8);
    s[3] = fma(ph, th, s[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Column statistics
// ---------------------------------------------------------------------------------------------------------------------
// Block: GP chunks x kRowLanes row lanes x CT columns.  part layout [B][K][kPartSums][nchunk].
__global__ __launch_bounds__(kColBlock) void maps_colstats_partial_kernel(
    const float* __restrict__ T, int64_t ldt, int64_t bst, const float* __restrict__ P, int64_t ldp, int64_t bsp,
    const int32_t* __restrict__ pmap, const float* __restrict__ conv, const int32_t* __restrict__ flags,
    const int32_t* __restrict__ rows, int32_t n, int32_t K, int32_t CT, int32_t GP, double* __restrict__ part) {
  __shared__ double red[kPartSums][kColBlock];
  const int tid = threadIdx.x;
  const int per = kRowLanes * CT;
  const int g = tid / per, lt = tid - g * per;
  const int rl = lt / CT, cl = lt - rl * CT;
  const int k = blockIdx.y * CT + cl;
  const int crow = chunk_rows(n), nchunk = num_chunks(n);
  const int ch = blockIdx.x * GP + g, b = blockIdx.z;
  const bool live = g < GP && k < K && ch < nchunk;
  double acc[kPartSums] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
    const Conv cv = load_conv(conv, flags, k);
    const float* Tb = T + (int64_t)b * bst + k;
    const float* Pb = P + (int64_t)b * bsp + (pmap ? pmap[k] : k);
    const int64_t r0 = rows ? rows[0] : 0;
    const double t0 = (double)to_units(Tb[r0 * ldt], cv);
    const double p0 = (double)to_units(Pb[r0 * ldp], cv);
    const int i0 = ch * crow, i1 = min(n, i0 + crow);
    constexpr int U = 4;
    for (int i = i0 + rl; i < i1; i += U * kRowLanes) {
      float tv[U], pv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ii = i + u * kRowLanes;
        if (ii < i1) {
          const int64_t r = rows ? rows[ii] : ii;
          tv[u] = Tb[r * ldt];
          pv[u] = Pb[r * ldp];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i + u * kRowLanes < i1) {
          const double p = (double)to_units(pv[u], cv) - p0;
          const double t = (double)to_units(tv[u], cv) - t0;
          acc[0] += p;
          acc[1] = fma(p, p, acc[1]);
          acc[2] += t;
          acc[3] = fma(t, t, acc[3]);
        }
      }
    }
  }
  gcl::lanes_to_part(red, acc, tid, kRowLanes, CT, live && rl == 0,
                     part + ((int64_t)b * K + k) * kPartSums * nchunk + ch, nchunk);
}

// One wave per (column blockIdx.x, sample blockIdx.y): cs[(b * K + k) * 4 + {mean_p, std_p, mean_t, std_t}].
__global__ __launch_bounds__(64) void maps_colstats_combine_kernel(
    const double* __restrict__ part, const float* __restrict__ T, int64_t ldt, int64_t bst, const float* __restrict__ P,
    int64_t ldp, int64_t bsp, const int32_t* __restrict__ pmap, const float* __restrict__ conv,
    const int32_t* __restrict__ flags, const int32_t* __restrict__ rows, int32_t n, int32_t K, double* __restrict__ cs) {
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nchunk = num_chunks(n);
  const double* src = part + ((int64_t)b * K + k) * kPartSums * nchunk;
  // the shift, loaded ahead of the sums so that its latency is not added to theirs
  const Conv cv = load_conv(conv, flags, k);
  const int64_t r0 = rows ? rows[0] : 0;
  const float tf = T[(int64_t)b * bst + r0 * ldt + k];
  const float pf = P[(int64_t)b * bsp + r0 * ldp + (pmap ? pmap[k] : k)];
  double S[kPartSums];
  gcl::wave_strided_sum(src, nchunk, tid, S);
  if (tid == 0) {
    const double t0 = (double)to_units(tf, cv);
    const double p0 = (double)to_units(pf, cv);
    const double N = (double)n;
    // unbiased, as torch.std: a single row gives 0 / 0 = NaN there and here
    const double vp = fmax(S[1] - S[0] * (S[0] / N), 0.0) / (N - 1.0);
    const double vt = fmax(S[3] - S[2] * (S[2] / N), 0.0) / (N - 1.0);
    double* o = cs + ((int64_t)b * K + k) * 4;
    o[0] = p0 + S[0] / N;
    o[1] = sqrt(vp);
    o[2] = t0 + S[2] / N;
    o[3] = sqrt(vt);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Accumulate
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kBU = 4;  // samples whose loads are issued together
// Largest statistics table a block of the flat kernel copies into LDS.  Measured at 512 x 256 x 19, B = 8: a 4.9 KB
// table (one lead) takes the kernel from 109 to 83 us, a 19 KB one (four leads) from 467 to 568 us - a block of 1024
// elements then copies a fifth of what it streams, behind a barrier - so larger tables stay in global memory.
constexpr int64_t kCsLdsBytes = 8192;

// Rows of exactly K floats, no row list, no column map: thread t owns the flat values q0 = 4 t .. q0 + 3 of every
// sample (one 16-byte load per tensor and sample).  VSTATE (leads == 1): its four state elements of a sum are
// consecutive too and move as two 16-byte accesses.  CSLDS: the block first copies the B x K x 4 column statistics
// into LDS - every thread reads 4 B entries of that table, and read from global memory they are two thirds of the
// kernel's vector loads, on the path that the streamed samples need.
template <bool VSTATE, bool CSLDS>
__global__ __launch_bounds__(256) void maps_accumulate_flat_kernel(
    const float* __restrict__ T, int64_t bst, const float* __restrict__ P, int64_t bsp, int32_t K, int32_t C,
    const float* __restrict__ conv, const int32_t* __restrict__ flags, int64_t nflat, int32_t B,
    const double* __restrict__ cs, int32_t mask, double* __restrict__ state, int64_t nE, int64_t* __restrict__ count) {
  extern __shared__ double cs_lds[];
  const int64_t q0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (q0 == 0) *count += B;
  if (CSLDS) {
    const int ncs = B * K * 4;  // a multiple of 4, and cs is 16-byte aligned
    for (int i = 2 * threadIdx.x; i < ncs; i += 2 * 256)
      *reinterpret_cast<double2*>(cs_lds + i) = *reinterpret_cast<const double2*>(cs + i);
    __syncthreads();
  }
  if (q0 >= nflat) return;
  const int nsums = __popc(mask);
  int kk[4];
  int64_t so[4];
  Conv cv[4];
  {
    // (row, lead, channel) of q0 by division, of the next three by stepping (nflat < 2^31 on this path)
    int i = (int)((uint32_t)q0 / (uint32_t)K);
    int k = (int)q0 - i * K;
    int l = k / C, c = k - l * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kk[j] = k;
      so[j] = (int64_t)l * nsums * nE + (int64_t)i * C + c;
      cv[j] = load_conv(conv, flags, k);
      ++k, ++c;
      if (c == C) c = 0, ++l;
      if (k == K) k = 0, l = 0, ++i;
    }
  }
  double s[4][4];
  {
    int p = 0;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      if (mask & (1 << slot)) {
        if (VSTATE) {
          const double2* src = reinterpret_cast<const double2*>(state + (int64_t)p * nE + q0);
          const double2 a = src[0], b2 = src[1];
          s[0][slot] = a.x, s[1][slot] = a.y, s[2][slot] = b2.x, s[3][slot] = b2.y;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j][slot] = state[so[j] + (int64_t)p * nE];
        }
        ++p;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j][slot] = 0.0;
      }
    }
  }
  for (int b0 = 0; b0 < B; b0 += kBU) {
    float4 tv[kBU], pv[kBU];
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      if (b0 + u < B) {
        tv[u] = gcl::ld4(T + (int64_t)(b0 + u) * bst + q0);
        pv[u] = gcl::ld4(P + (int64_t)(b0 + u) * bsp + q0);
      }
    }
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      if (b0 + u < B) {
        const float t4[4] = {tv[u].x, tv[u].y, tv[u].z, tv[u].w};
        const float p4[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
        const int64_t csb = (int64_t)(b0 + u) * K * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          add_sample(s[j], to_units(p4[j], cv[j]), to_units(t4[j], cv[j]), mask,
                     (CSLDS ? cs_lds : cs) + (csb + 4 * kk[j]));
      }
    }
  }
  {
    int p = 0;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      if (mask & (1 << slot)) {
        if (VSTATE) {
          double2* dst = reinterpret_cast<double2*>(state + (int64_t)p * nE + q0);
          dst[0] = make_double2(s[0][slot], s[1][slot]);
          dst[1] = make_double2(s[2][slot], s[3][slot]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) state[so[j] + (int64_t)p * nE] = s[j][slot];
        }
        ++p;
      }
    }
  }
}

// Any layout: one thread per element (lead, scored row i, channel c).
__global__ __launch_bounds__(256) void maps_accumulate_kernel(
    const float* __restrict__ T, int64_t ldt, int64_t bst, const float* __restrict__ P, int64_t ldp, int64_t bsp,
    const int32_t* __restrict__ pmap, int32_t leads, int32_t C, const float* __restrict__ conv,
    const int32_t* __restrict__ flags, const int32_t* __restrict__ rows, int32_t B, const double* __restrict__ cs,
    int32_t mask, double* __restrict__ state, int64_t nE, int64_t* __restrict__ count) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx == 0) *count += B;
  if (idx >= nE * leads) return;
  const int nsums = __popc(mask);
  const int K = leads * C;
  const int l = (int)(idx / nE);
  const int64_t sidx = idx - (int64_t)l * nE;
  const int64_t i = sidx / C;
  const int c = (int)(sidx - i * C);
  const int k = l * C + c;
  const int64_t r = rows ? rows[i] : i;
  const Conv cv = load_conv(conv, flags, k);
  const float* Tp = T + r * ldt + k;
  const float* Pp = P + r * ldp + (pmap ? pmap[k] : k);
  double* sp = state + (int64_t)l * nsums * nE + sidx;
  double s[4];
  {
    int p = 0;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) s[slot] = (mask & (1 << slot)) ? sp[(int64_t)(p++) * nE] : 0.0;
  }
  for (int b0 = 0; b0 < B; b0 += kBU) {
    float tv[kBU], pv[kBU];
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      if (b0 + u < B) {
        tv[u] = Tp[(int64_t)(b0 + u) * bst];
        pv[u] = Pp[(int64_t)(b0 + u) * bsp];
      }
    }
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      if (b0 + u < B)
        add_sample(s, to_units(pv[u], cv), to_units(tv[u], cv), mask, cs + ((int64_t)(b0 + u) * K + k) * 4);
    }
  }
  {
    int p = 0;
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      if (mask & (1 << slot)) sp[(int64_t)(p++) * nE] = s[slot];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Finalize, convert
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maps_finalize_kernel(const double* __restrict__ state,
                                                            const int64_t* __restrict__ count, int32_t plane,
                                                            int32_t nsums, int32_t leads, int64_t nE, int32_t kind,
                                                            const double* __restrict__ rstate,
                                                            const int64_t* __restrict__ rcount, int32_t rplane,
                                                            int32_t rnsums, float* __restrict__ out) {
  const int64_t total = nE * leads;
  const double n = (double)*count;
  const double rn = rstate ? (double)*rcount : 0.0;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t l = t / nE, e = t - l * nE;
    const double v = state[(l * nsums + plane) * nE + e];
    float o = 0.f;
    if (kind == kKindSkill) {
      const float r = n > 0.0 ? (float)sqrt(v / n) : 0.f;
      const float rr = rn > 0.0 ? (float)sqrt(rstate[(l * rnsums + rplane) * nE + e] / rn) : 0.f;
      o = (float)(1.0 - (double)r / fmax((double)rr, 1e-9));
    } else if (n > 0.0) {
      o = kind == kKindRmse ? (float)sqrt(v / n) : (float)(v / n);
    }
    out[t] = o;
  }
}

__global__ __launch_bounds__(256) void maps_convert_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           int64_t total, int32_t K, const float* __restrict__ conv,
                                                           const int32_t* __restrict__ flags) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256)
    out[t] = to_units(x[t], load_conv(conv, flags, (int)(t % K)));
}

}  // namespace

extern "C" size_t gcl_maps_colstats_ws_bytes(int32_t n, int32_t K, int32_t B) {
  if (n <= 0 || K <= 0 || B <= 0) return 0;
  return (size_t)B * K * kPartSums * num_chunks(n) * sizeof(double);
}

extern "C" int gcl_maps_colstats(const float* truth, int64_t ldt, int64_t bst, const float* pred, int64_t ldp,
                                 int64_t bsp, const int32_t* pmap, int32_t K, const float* conv, const int32_t* flags,
                                 const int32_t* rows, int32_t n, int32_t B, double* cs, void* ws, size_t ws_bytes,
                                 gcl_stream_t stream) {
  GCL_CHECK_ARG(truth && pred && cs, "maps_colstats: null argument");
  GCL_CHECK_ARG(K > 0 && n > 0 && B > 0, "maps_colstats: bad shape (K=%d, n=%d, B=%d)", K, n, B);
  GCL_CHECK_ARG(K <= 65535 * kColTile && B <= 65535, "maps_colstats: K=%d or B=%d too large", K, B);
  GCL_CHECK_ARG(!conv == !flags, "maps_colstats: conv and flags go together");
  const size_t need = gcl_maps_colstats_ws_bytes(n, K, B);
  GCL_CHECK_ARG(ws && ws_bytes >= need, "maps_colstats: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const int CT = K < kColTile ? K : kColTile;
  const int GP = kColBlock / (kRowLanes * CT);
  const int nchunk = num_chunks(n);
  double* part = (double*)ws;
  hipLaunchKernelGGL(maps_colstats_partial_kernel, dim3((unsigned)gcl::cdiv(nchunk, GP), (unsigned)gcl::cdiv(K, CT), B),
                     dim3(kColBlock), 0, st, truth, ldt, bst, pred, ldp, bsp, pmap, conv, flags, rows, n, K, CT, GP,
                     part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(maps_colstats_combine_kernel, dim3(K, B), dim3(64), 0, st, (const double*)part, truth, ldt, bst,
                     pred, ldp, bsp, pmap, conv, flags, rows, n, K, cs);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_maps_accumulate(const float* truth, int64_t ldt, int64_t bst, const float* pred, int64_t ldp,
                                   int64_t bsp, const int32_t* pmap, int32_t leads, int32_t C, const float* conv,
                                   const int32_t* flags, const int32_t* rows, int32_t n, int32_t B, const double* cs,
                                   int32_t sums, double* state, int64_t* count, gcl_stream_t stream) {
  GCL_CHECK_ARG(truth && pred && state && count, "maps_accumulate: null argument");
  GCL_CHECK_ARG(leads > 0 && C > 0 && n > 0 && B > 0, "maps_accumulate: bad shape (leads=%d, C=%d, n=%d, B=%d)", leads,
                C, n, B);
  GCL_CHECK_ARG(sums > 0 && sums < 16, "maps_accumulate: sums=%d is not a set of the four sums", sums);
  GCL_CHECK_ARG(!(sums & kSumPT) || cs, "maps_accumulate: the ACC sum needs the column statistics");
  GCL_CHECK_ARG(!conv == !flags, "maps_accumulate: conv and flags go together");
  const int64_t K = (int64_t)leads * C, nE = (int64_t)n * C;
  // one launch covers every element: 256-thread blocks, the grid well inside what HIP accepts
  GCL_CHECK_ARG(nE * leads < ((int64_t)1 << 31), "maps_accumulate: %lld elements, at most 2^31 - 1 per call",
                (long long)(nE * leads));
  const hipStream_t st = (hipStream_t)stream;
  const int64_t nflat = (int64_t)n * K;
  const bool flat = !rows && !pmap && ldt == K && ldp == K && nflat % 4 == 0 && nflat < ((int64_t)1 << 31) &&
                    gcl::aligned16(truth) &&
                    gcl::aligned16(pred) && gcl::aligned16(state) && (B == 1 || (bst % 4 == 0 && bsp % 4 == 0));
  if (flat) {
    const unsigned grid = (unsigned)gcl::cdiv(nflat / 4, 256);
    // the statistics table goes to LDS when it is used, fits kCsLdsBytes and can move as 16-byte pairs
    const int64_t cs_bytes = (int64_t)B * K * 4 * sizeof(double);
    const bool cs_lds = (sums & kSumPT) && cs_bytes <= kCsLdsBytes && gcl::aligned16(cs);
    const unsigned lds = cs_lds ? (unsigned)cs_bytes : 0u;
    const auto kernel =
        leads == 1 ? (cs_lds ? maps_accumulate_flat_kernel<true, true> : maps_accumulate_flat_kernel<true, false>)
                   : (cs_lds ? maps_accumulate_flat_kernel<false, true> : maps_accumulate_flat_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, truth, bst, pred, bsp, (int32_t)K, C, conv, flags, nflat,
                       B, cs, sums, state, nE, count);
  } else {
    hipLaunchKernelGGL(maps_accumulate_kernel, dim3((unsigned)gcl::cdiv(nE * leads, 256)), dim3(256), 0, st, truth,
                       ldt, bst, pred, ldp, bsp, pmap, leads, C, conv, flags, rows, B, cs, sums, state, nE, count);
  }
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_maps_finalize(const double* state, const int64_t* count, int32_t plane, int32_t nsums,
                                 int32_t leads, int64_t nelem, int32_t kind, const double* ref_state,
                                 const int64_t* ref_count, int32_t ref_plane, int32_t ref_nsums, float* out,
                                 gcl_stream_t stream) {
  GCL_CHECK_ARG(state && count && out, "maps_finalize: null argument");
  GCL_CHECK_ARG(kind >= kKindRmse && kind <= kKindSkill, "maps_finalize: kind=%d", kind);
  GCL_CHECK_ARG(nsums >= 1 && nsums <= 4 && plane >= 0 && plane < nsums, "maps_finalize: plane %d of %d", plane, nsums);
  GCL_CHECK_ARG(leads > 0 && nelem >= 0, "maps_finalize: bad shape (leads=%d)", leads);
  if (kind == kKindSkill) {
    GCL_CHECK_ARG(ref_state && ref_count, "maps_finalize: skill needs the reference state");
    GCL_CHECK_ARG(ref_nsums >= 1 && ref_nsums <= 4 && ref_plane >= 0 && ref_plane < ref_nsums,
                  "maps_finalize: reference plane %d of %d", ref_plane, ref_nsums);
  }
  if (nelem == 0) return GCL_OK;
  hipLaunchKernelGGL(maps_finalize_kernel, dim3(gcl::grid_for(nelem * leads, 8192)), dim3(256), 0, (hipStream_t)stream,
                     state, count, plane, nsums, leads, nelem, kind, kind == kKindSkill ? ref_state : nullptr, ref_count,
                     ref_plane, ref_nsums, out);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_maps_convert(const float* x, float* out, int64_t total, int32_t K, const float* conv,
                                const int32_t* flags, gcl_stream_t stream) {
  GCL_CHECK_ARG(x && out && conv && flags, "maps_convert: null argument");
  GCL_CHECK_ARG(total >= 0 && K > 0, "maps_convert: bad shape (total=%lld, K=%d)", (long long)total, K);
  if (total == 0) return GCL_OK;
  hipLaunchKernelGGL(maps_convert_kernel, dim3(gcl::grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, x, out,
                     total, K, conv, flags);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
