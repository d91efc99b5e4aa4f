// Building, repairing and extending the fp16 dataset on the device (gfx950): the arithmetic core the reference's
// scripts/build_dataset_512x256.py, recompute_wb2_scalers.py, repair_dataset.py, add_time_features.py and
// check_23f_data.py share - one strided 2-byte pass per channel over a memmap plus two passes for the sums - done as
// one pass over the (T, lon, lat, Ct) series in HBM.  Reductions are two-stage and fixed-order (no atomics): a result
// depends only on the data and the shapes.
#include "common.h"

using gcl::load_span;
using gcl::rounded;
using gcl::store_span;
using gcl::wave_sum;

namespace {

constexpr int kMaxSrc = 32;    // sources of one pack call (they travel in the kernel arguments)
constexpr int kTile = 512;     // points of one pack tile: 512 * Ct halves are staged in LDS
constexpr int kBlocks = 2048;  // most blocks of a reducing kernel = partial records of its second stage
constexpr int kStatQ = 6;      // sum, sumsq, min, max, #NaN, #inf

// ---- pack ------------------------------------------------------------------------------------------------------------
struct PackArgs {
  const float* src[kMaxSrc];  // [nt, P] float32 planes, time stride tstride (0: time-invariant)
  int64_t tstride[kMaxSrc];
  int32_t chan[kMaxSrc];
  float scale[kMaxSrc];
  int32_t nsrc, Ct, full;
  int64_t P, t0, tiles_per_t, ntiles;
  uint16_t* series;  // NULL: sums only
  double* part;      // [gridDim.x][nsrc][2]
};

// A block walks tiles of kTile points of one time step, tile = blockIdx.x, + gridDim.x, ..: a fixed assignment, so the
// partial sums of a (shape, data) pair are always formed in the same order.  Per source: 2 KiB of consecutive floats
// in, scaled (the product rounded to float32 on its own), squared (rounded again), both widened to float64 and summed
// over the wave; lane 0 of a wave adds them onto the wave's accumulators in LDS.  (Keeping the sums in registers until
// the end - the source loop unrolled, one pair per source and thread - costs 168 VGPRs at 19 channels and measured
// slower with 4-byte loads, 5.05 ms against 4.42 ms for the 500-step block; what helped was wider loads, 2.56 ms.)
// With every channel listed the fp16 values of the tile are one contiguous span of the series: staged as
// [point][channel] in LDS and written by store_span.  With a partial list every value is one 2-byte store and the
// other channels are never touched.
//
// VEC (every plane 16-byte aligned, P and the time strides multiples of 4, and no scattered stores: all channels or
// sums only): a thread takes four consecutive points of a source with one 16-byte load; threads 0-127 serve the even
// sources of a group of eight, threads 128-255 the odd ones.  Otherwise a thread takes points tid and tid + 256 of
// each source of a group of four.
template <bool VEC>
__global__ __launch_bounds__(256) void dataset_pack_kernel(PackArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* wacc = reinterpret_cast<double*>(smem);  // [4 waves][kMaxSrc][2]
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem + 4 * kMaxSrc * 2 * sizeof(double));
  constexpr int K = VEC ? 4 : 2;                   // values of one source a thread takes from a tile
  constexpr int G = VEC ? 8 : 4;                   // sources of a group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = VEC ? __builtin_amdgcn_readfirstlane(tid >> 7) : 0;  // wave-uniform
  const int first = VEC ? 4 * (tid & 127) : tid;   // the thread's first point of a tile
  for (int i = tid; i < 4 * kMaxSrc * 2; i += 256) wacc[i] = 0.0;
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t t = tile / a.tiles_per_t;
    const int64_t p0 = (tile - t * a.tiles_per_t) * kTile;
    const int np = (int)((a.P - p0) < kTile ? (a.P - p0) : kTile);
    const int64_t row0 = ((a.t0 + t) * a.P + p0) * a.Ct;  // first half of the tile in the series
    for (int j0 = 0; j0 < a.nsrc; j0 += G) {
      float v[4][K];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = VEC ? j0 + 2 * u + half : j0 + u;
#pragma unroll
        for (int k = 0; k < K; ++k) v[u][k] = 0.f;
        if (j < a.nsrc) {
          const float* __restrict__ x = a.src[j] + t * a.tstride[j] + p0;
          const float sc = a.scale[j];
          if constexpr (VEC) {
            if (first < np) {  // np is a multiple of 4 here
              const float4 w = gcl::ld4(x + first);
              v[u][0] = rounded(w.x * sc); v[u][1] = rounded(w.y * sc);
              v[u][2] = rounded(w.z * sc); v[u][3] = rounded(w.w * sc);
            }
          } else {
#pragma unroll
            for (int k = 0; k < K; ++k)
              if (first + 256 * k < np) v[u][k] = rounded(x[first + 256 * k] * sc);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = VEC ? j0 + 2 * u + half : j0 + u;
        if (j >= a.nsrc) break;  // wave-uniform
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int p = VEC ? first + k : first + 256 * k;
          if (p < np) {
            const float x = v[u][k];
            s += (double)x;
            q += (double)rounded(x * x);
            if (a.series) {
              const uint16_t h = __builtin_bit_cast(uint16_t, (_Float16)x);
              if (a.full) stage[p * a.Ct + a.chan[j]] = h;
              else a.series[row0 + (int64_t)p * a.Ct + a.chan[j]] = h;
            }
          }
        }
        s = wave_sum(s);
        q = wave_sum(q);
        if (lane == 0) {
          wacc[(wave * kMaxSrc + j) * 2] += s;
          wacc[(wave * kMaxSrc + j) * 2 + 1] += q;
        }
      }
    }
    if (a.series && a.full) {
      __syncthreads();
      store_span<256>(a.series + row0, np * a.Ct, [&](int k) { return stage[k]; });
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < a.nsrc * 2) {
    const int j = tid >> 1, k = tid & 1;
    double s = wacc[j * 2 + k];
    for (int w = 1; w < 4; ++w) s += wacc[(w * kMaxSrc + j) * 2 + k];
    a.part[((int64_t)blockIdx.x * a.nsrc + j) * 2 + k] = s;
  }
}

struct PackChan {
  int32_t chan[kMaxSrc];
};

// second stage: one wave per source adds the nparts records in a fixed order (lane l takes l, l + 64, ..)
__global__ __launch_bounds__(64) void dataset_pack_reduce_kernel(const double* __restrict__ part, int nparts, int nsrc,
                                                                 PackChan c, double* sum, double* sumsq) {
  const int j = blockIdx.x, lane = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int b = lane; b < nparts; b += 64) {
    s += part[((int64_t)b * nsrc + j) * 2];
    q += part[((int64_t)b * nsrc + j) * 2 + 1];
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if (lane == 0) {
    sum[c.chan[j]] = s;
    sumsq[c.chan[j]] = q;
  }
}

// ---- stats -----------------------------------------------------------------------------------------------------------
// `x` is the first half of row t_s, n the halves of rows [t_s, t_e).  A thread takes 8 consecutive halves (one 16-byte
// load when the span is aligned) of a chunk of A * 8 halves, A the largest thread count <= 256 for which the chunk is
// a whole number of rows: the channel of a thread's m-th half is then (tid * 8 + m) % Ct in every chunk, so a thread
// keeps 8 records in registers.  Chunks are dealt blockIdx.x, + gridDim.x, ...  At the end the records go through LDS,
// one quantity at a time, and thread c < Ct folds those of channel c in index order.
__global__ __launch_bounds__(256) void dataset_stats_kernel(const uint16_t* __restrict__ x, int64_t n, int32_t Ct,
                                                            int32_t A, int32_t flags, int32_t vec, double* part) {
  __shared__ double red[256 * 8];
  const int tid = threadIdx.x;
  double s[8], q[8];
  float mn[8], mx[8];
  int32_t nn[8], ni[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    s[m] = q[m] = 0.0;
    mn[m] = __builtin_inff();
    mx[m] = -__builtin_inff();
    nn[m] = ni[m] = 0;
  }
  const int64_t chunk = (int64_t)A * 8;
  if (tid < A) {
    for (int64_t e0 = (int64_t)blockIdx.x * chunk + tid * 8; e0 < n; e0 += (int64_t)gridDim.x * chunk) {
      union { uint4 qv; uint16_t h[8]; } u;
      const bool whole = e0 + 8 <= n;
      if (vec && whole) {
        u.qv = *reinterpret_cast<const uint4*>(x + e0);
      } else {
#pragma unroll
        for (int m = 0; m < 8; ++m) u.h[m] = e0 + m < n ? x[e0 + m] : (uint16_t)0;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        if (!whole && e0 + m >= n) continue;
        float v = (float)__builtin_bit_cast(_Float16, u.h[m]);
        const bool isn = v != v, isi = __builtin_fabsf(v) == __builtin_inff();
        nn[m] += isn;
        ni[m] += isi;
        if (!isn && !isi) {
          mn[m] = v < mn[m] ? v : mn[m];
          mx[m] = v > mx[m] ? v : mx[m];
        }
        if ((isn && (flags & 1)) || (isi && (flags & 2))) v = 0.f;
        s[m] += (double)v;
        q[m] += (double)rounded(v * v);
      }
    }
  }
  for (int qty = 0; qty < kStatQ; ++qty) {
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m)
      red[tid * 8 + m] = qty == 0 ? s[m] : qty == 1 ? q[m] : qty == 2 ? (double)mn[m] : qty == 3 ? (double)mx[m]
                         : qty == 4 ? (double)nn[m] : (double)ni[m];
    __syncthreads();
    if (tid < Ct) {
      double r = red[tid];
      for (int i = tid + Ct; i < A * 8; i += Ct) {
        const double y = red[i];
        r = qty == 2 ? (y < r ? y : r) : qty == 3 ? (y > r ? y : r) : r + y;
      }
      part[((int64_t)blockIdx.x * Ct + tid) * kStatQ + qty] = r;
    }
  }
}

__global__ __launch_bounds__(64) void dataset_stats_reduce_kernel(const double* __restrict__ part, int nparts, int Ct,
                                                                  double* sum, double* sumsq, float* vmin, float* vmax,
                                                                  int64_t* n_nan, int64_t* n_inf) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double r[kStatQ] = {0.0, 0.0, (double)__builtin_inff(), -(double)__builtin_inff(), 0.0, 0.0};
  for (int b = lane; b < nparts; b += 64) {
    const double* p = part + ((int64_t)b * Ct + c) * kStatQ;
    r[0] += p[0];
    r[1] += p[1];
    r[2] = p[2] < r[2] ? p[2] : r[2];
    r[3] = p[3] > r[3] ? p[3] : r[3];
    r[4] += p[4];
    r[5] += p[5];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kStatQ; ++k) {
      const double y = __shfl_xor(r[k], off, 64);
      r[k] = k == 2 ? (y < r[k] ? y : r[k]) : k == 3 ? (y > r[k] ? y : r[k]) : r[k] + y;
    }
  }
  if (lane == 0) {
    sum[c] = r[0];
    sumsq[c] = r[1];
    vmin[c] = (float)r[2];
    vmax[c] = (float)r[3];
    n_nan[c] = (int64_t)r[4];  // counts are whole numbers below 2^53: exact in float64
    n_inf[c] = (int64_t)r[5];
  }
}

// ---- welford ---------------------------------------------------------------------------------------------------------
// welford_update of the reference on the device, every operation of the numpy expression rounded alone in its order.
__global__ __launch_bounds__(256) void dataset_welford_kernel(double* mean, double* m2, int64_t* n,
                                                              const double* __restrict__ bsum,
                                                              const double* __restrict__ bsumsq, int64_t block_n, int C) {
  const int64_t total_n = *n, new_n = total_n + block_n;
  const double bn = (double)block_n, tn = (double)total_n, nn = (double)new_n;
  const double frac = rounded(bn / nn);
  for (int c = threadIdx.x; c < C; c += 256) {
    const double bm = rounded(bsum[c] / bn);
    double bv = rounded(bsumsq[c] / bn) - rounded(bm * bm);
    bv = bv != bv ? bv : (bv > 0.0 ? bv : 0.0);  // np.maximum(block_var, 0.0): NaN stays
    const double delta = bm - mean[c];
    mean[c] = mean[c] + rounded(delta * frac);
    const double between = rounded(rounded(rounded(rounded(delta * delta) * tn) * bn) / nn);
    m2[c] = m2[c] + rounded(rounded(bv * bn) + between);
  }
  __syncthreads();  // every thread has read *n
  if (threadIdx.x == 0) *n = new_n;
}

// ---- widen -----------------------------------------------------------------------------------------------------------
// One tile of `tile` points of one time step: Co * tile halves in (one span of src), Cn * tile halves out (one span of
// dst), the new channels from extra[t, :].  Bits are moved, never converted.
__global__ __launch_bounds__(256) void dataset_widen_kernel(const uint16_t* __restrict__ src, uint16_t* dst,
                                                            const uint16_t* __restrict__ extra, int64_t P, int32_t Co,
                                                            int32_t Cn, int32_t tile, int64_t tiles_per_t, int64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t t = tl / tiles_per_t;
    const int64_t p0 = (tl - t * tiles_per_t) * tile;
    const int np = (int)((P - p0) < tile ? (P - p0) : tile);
    load_span<256>(src + (t * P + p0) * Co, np * Co, stage);
    __syncthreads();
    const uint16_t* ex = extra + t * (Cn - Co);
    store_span<256>(dst + (t * P + p0) * Cn, np * Cn, [&](int k) {
      const int p = k / Cn, c = k - p * Cn;
      return c < Co ? stage[p * Co + c] : ex[c - Co];
    });
    __syncthreads();
  }
}

unsigned blocks_for(int64_t items) { return (unsigned)(items < kBlocks ? (items > 0 ? items : 1) : kBlocks); }

}  // namespace

extern "C" size_t gcl_dataset_ws_bytes(int32_t C) {
  const size_t pack = (size_t)kBlocks * kMaxSrc * 2 * sizeof(double);
  const size_t stats = (size_t)kBlocks * (size_t)(C > 0 ? C : 1) * kStatQ * sizeof(double);
  return pack > stats ? pack : stats;
}

extern "C" int gcl_dataset_max_sources(void) { return kMaxSrc; }

extern "C" int gcl_dataset_pack(const float* const* src, const int64_t* tstride, const int32_t* chan, const float* scale,
                                int32_t nsrc, int32_t nt, int32_t n_lon, int32_t n_lat, uint16_t* series, int64_t T,
                                int32_t Ct, int64_t t0, double* sum, double* sumsq, void* ws, size_t ws_bytes,
                                gcl_stream_t stream) {
  GCL_CHECK_ARG(src && tstride && chan && scale && sum && sumsq && ws, "dataset_pack: null argument");
  GCL_CHECK_ARG(nsrc > 0 && nsrc <= kMaxSrc, "dataset_pack: %d sources (1 .. %d per call)", nsrc, kMaxSrc);
  GCL_CHECK_ARG(nt > 0 && n_lon > 0 && n_lat > 0 && Ct > 0 && Ct <= 256 && T > 0 && t0 >= 0 && t0 + nt <= T,
                "dataset_pack: bad shape (nt=%d grid %dx%d Ct=%d rows [%lld, %lld) of %lld)", nt, n_lon, n_lat, Ct,
                (long long)t0, (long long)t0 + nt, (long long)T);
  const int64_t P = (int64_t)n_lon * n_lat;
  uint64_t seen[4] = {0, 0, 0, 0};
  for (int j = 0; j < nsrc; ++j) {
    GCL_CHECK_ARG(src[j], "dataset_pack: source %d is null", j);
    GCL_CHECK_ARG(tstride[j] == 0 || tstride[j] >= P, "dataset_pack: source %d has time stride %lld (0 or >= %lld)", j,
                  (long long)tstride[j], (long long)P);
    GCL_CHECK_ARG(chan[j] >= 0 && chan[j] < Ct, "dataset_pack: source %d goes to channel %d of %d", j, chan[j], Ct);
    GCL_CHECK_ARG(!(seen[chan[j] >> 6] >> (chan[j] & 63) & 1), "dataset_pack: channel %d is listed twice", chan[j]);
    seen[chan[j] >> 6] |= 1ull << (chan[j] & 63);
  }
  GCL_CHECK_ARG(!series || (reinterpret_cast<uintptr_t>(series) & 1) == 0, "dataset_pack: series is not 2-byte aligned");
  PackArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < nsrc; ++j) {
    a.src[j] = src[j];
    a.tstride[j] = tstride[j];
    a.chan[j] = chan[j];
    a.scale[j] = scale[j];
  }
  a.nsrc = nsrc; a.Ct = Ct; a.full = nsrc == Ct; a.P = P; a.t0 = t0;
  a.tiles_per_t = gcl::cdiv(P, kTile);
  a.ntiles = a.tiles_per_t * nt;
  a.series = series;
  a.part = reinterpret_cast<double*>(ws);
  const unsigned nb = blocks_for(a.ntiles);
  GCL_CHECK_ARG(ws_bytes >= (size_t)nb * nsrc * 2 * sizeof(double), "dataset_pack: workspace of %zu bytes is too small",
                ws_bytes);
  const size_t lds = 4 * kMaxSrc * 2 * sizeof(double) + (series && a.full ? (size_t)kTile * Ct * sizeof(uint16_t) : 0);
  bool vec = P % 4 == 0 && (a.full || !series);  // scattered 2-byte stores of four points per lane measured slower
  for (int j = 0; j < nsrc; ++j) vec = vec && gcl::aligned16(src[j]) && tstride[j] % 4 == 0;
  if (vec) hipLaunchKernelGGL(dataset_pack_kernel<true>, dim3(nb), dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(dataset_pack_kernel<false>, dim3(nb), dim3(256), lds, (hipStream_t)stream, a);
  GCL_CHECK_LAUNCH();
  PackChan pc;
  memcpy(pc.chan, a.chan, sizeof(pc.chan));
  hipLaunchKernelGGL(dataset_pack_reduce_kernel, dim3(nsrc), dim3(64), 0, (hipStream_t)stream, a.part, (int)nb, nsrc, pc,
                     sum, sumsq);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_dataset_stats(const uint16_t* series, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct, int64_t t_s,
                                 int64_t t_e, int32_t flags, double* sum, double* sumsq, float* vmin, float* vmax,
                                 int64_t* n_nan, int64_t* n_inf, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(series && sum && sumsq && vmin && vmax && n_nan && n_inf && ws, "dataset_stats: null argument");
  GCL_CHECK_ARG(T > 0 && n_lon > 0 && n_lat > 0 && Ct > 0 && Ct <= 256 && t_s >= 0 && t_s < t_e && t_e <= T,
                "dataset_stats: bad shape (grid %dx%d Ct=%d rows [%lld, %lld) of %lld)", n_lon, n_lat, Ct, (long long)t_s,
                (long long)t_e, (long long)T);
  GCL_CHECK_ARG((flags & ~3) == 0, "dataset_stats: unknown flag bits in %d", flags);
  GCL_CHECK_ARG((reinterpret_cast<uintptr_t>(series) & 1) == 0, "dataset_stats: series is not 2-byte aligned");
  const int64_t P = (int64_t)n_lon * n_lat;
  const uint16_t* x = series + t_s * P * Ct;
  const int64_t n = (t_e - t_s) * P * Ct;
  int g = Ct, e = 8;  // g = Ct / gcd(Ct, 8)
  while (e > 1 && g % 2 == 0) { g /= 2; e /= 2; }
  const int A = 256 / g * g;
  const unsigned nb = blocks_for(gcl::cdiv(n, (int64_t)A * 8));
  GCL_CHECK_ARG(ws_bytes >= (size_t)nb * Ct * kStatQ * sizeof(double), "dataset_stats: workspace of %zu bytes is too small",
                ws_bytes);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(dataset_stats_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, n, Ct, A, flags,
                     (int32_t)gcl::aligned16(x), part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(dataset_stats_reduce_kernel, dim3(Ct), dim3(64), 0, (hipStream_t)stream, part, (int)nb, Ct, sum, sumsq,
                     vmin, vmax, n_nan, n_inf);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_dataset_welford(double* mean, double* m2, int64_t* n, const double* block_sum,
                                   const double* block_sumsq, int64_t block_n, int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(mean && m2 && n && block_sum && block_sumsq, "dataset_welford: null argument");
  GCL_CHECK_ARG(C > 0 && block_n > 0, "dataset_welford: bad shape (C=%d block_n=%lld)", C, (long long)block_n);
  hipLaunchKernelGGL(dataset_welford_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mean, m2, n, block_sum,
                     block_sumsq, block_n, C);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_dataset_widen(const uint16_t* src, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct_old,
                                 const uint16_t* extra, int32_t Ct_new, uint16_t* dst, gcl_stream_t stream) {
  GCL_CHECK_ARG(src && extra && dst, "dataset_widen: null argument");
  GCL_CHECK_ARG(T > 0 && n_lon > 0 && n_lat > 0 && Ct_old > 0 && Ct_new > Ct_old && Ct_new <= 256,
                "dataset_widen: bad shape (T=%lld grid %dx%d channels %d -> %d)", (long long)T, n_lon, n_lat, Ct_old,
                Ct_new);
  GCL_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(extra)) & 1) == 0,
                "dataset_widen: a buffer is not 2-byte aligned");
  GCL_CHECK_ARG(src != dst, "dataset_widen: in place is not possible");
  const int64_t P = (int64_t)n_lon * n_lat;
  int tile = kTile;  // LDS: tile * Ct_old halves, within 32 KiB
  while (tile > 32 && (int64_t)tile * Ct_old * 2 > 32768) tile >>= 1;
  const int64_t tiles_per_t = gcl::cdiv(P, tile), ntiles = tiles_per_t * T;
  const unsigned nb = (unsigned)(ntiles < (1 << 20) ? ntiles : (1 << 20));
  hipLaunchKernelGGL(dataset_widen_kernel, dim3(nb), dim3(256), (size_t)tile * Ct_old * sizeof(uint16_t),
                     (hipStream_t)stream, src, dst, extra, P, Ct_old, Ct_new, tile, tiles_per_t, ntiles);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

// ---- legacy tensor datasets --------------------------------------------------------------------------------------------
// Batches from the stored tensors of src/data/dataloader.py:25-153 ([N, G, W, F] float32: X_train.pt etc. as saved, the
// grid flattened): the last Wu of the W stored steps, the first Fu of the F stored features (:129-132), sample idx[b]:
//   outX[b, g, w * Fu + f] = X[idx[b], g, Wx - Wxu + w, f],   outY[b, g, w * Fu + f] = Y[idx[b], g, Wy - Wyu + w, f]
// One thread per output element, X and Y rows in one launch; plain copies, so bit-exact.  A sample outside [0, N)
// comes back as NaN, as a window that leaves the series does in gcl_window_pack.
namespace {

__global__ __launch_bounds__(256) void tensor_batch_pack_kernel(const float* __restrict__ X, int32_t Wx, int32_t Wxu,
                                                                const float* __restrict__ Y, int32_t Wy, int32_t Wyu,
                                                                int64_t N, int32_t G, int32_t F, int32_t Fu,
                                                                const int64_t* __restrict__ idx, int32_t B,
                                                                float* __restrict__ outX, int64_t ldx, int64_t bsx,
                                                                float* __restrict__ outY, int64_t ldy, int64_t bsy) {
  const int rowx = Wxu * Fu, row = rowx + (Y ? Wyu * Fu : 0);
  const int64_t total = (int64_t)B * G * row;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int k = (int)(t % row);
    const int64_t bg = t / row;
    const int64_t g = bg % G;
    const int64_t b = bg / G;
    const bool is_y = k >= rowx;
    if (is_y) k -= rowx;
    const int w = k / Fu, f = k - w * Fu;
    const int64_t n = idx[b];
    float v = __builtin_nanf("");
    if (n >= 0 && n < N) {
      const int W = is_y ? Wy : Wx, w0 = is_y ? Wy - Wyu : Wx - Wxu;
      v = (is_y ? Y : X)[((n * G + g) * W + w0 + w) * F + f];
    }
    if (is_y) outY[b * bsy + g * ldy + k] = v;
    else outX[b * bsx + g * ldx + k] = v;
  }
}

}  // namespace

extern "C" int gcl_tensor_batch_pack(const float* X, int32_t Wx, int32_t Wxu, const float* Y, int32_t Wy, int32_t Wyu,
                                     int64_t N, int32_t G, int32_t F, int32_t Fu, const int64_t* idx, int32_t B,
                                     float* outX, int64_t ldx, int64_t bsx, float* outY, int64_t ldy, int64_t bsy,
                                     gcl_stream_t stream) {
  GCL_CHECK_ARG(X && idx && outX, "tensor_batch_pack: null argument");
  GCL_CHECK_ARG(!Y == !outY, "tensor_batch_pack: Y and outY go together");
  GCL_CHECK_ARG(N > 0 && G > 0 && F > 0 && B > 0, "tensor_batch_pack: bad shape (N=%lld, G=%d, F=%d, B=%d)", (long long)N,
                G, F, B);
  GCL_CHECK_ARG(Fu >= 1 && Fu <= F, "tensor_batch_pack: %d of %d features", Fu, F);
  GCL_CHECK_ARG(Wxu >= 1 && Wxu <= Wx, "tensor_batch_pack: %d of %d stored steps (X)", Wxu, Wx);
  GCL_CHECK_ARG(!Y || (Wyu >= 1 && Wyu <= Wy), "tensor_batch_pack: %d of %d stored steps (Y)", Wyu, Wy);
  GCL_CHECK_ARG(ldx >= (int64_t)Wxu * Fu && (!Y || ldy >= (int64_t)Wyu * Fu), "tensor_batch_pack: output row too short");
  const int64_t total = (int64_t)B * G * ((int64_t)Wxu * Fu + (Y ? (int64_t)Wyu * Fu : 0));
  hipLaunchKernelGGL(tensor_batch_pack_kernel, dim3(gcl::grid_for(total, 16384)), dim3(256), 0, (hipStream_t)stream, X, Wx,
                     Wxu, Y, Wy, Wyu, N, G, F, Fu, idx, B, outX, ldx, bsx, outY, ldy, bsy);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
