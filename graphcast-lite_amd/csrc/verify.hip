// Forecast scoring (scripts/predict.py:53-122 StreamingMetrics) and global -> regional blending
// (scripts/predict_pipeline.py:95-149).
//
// Column statistics.  For every column k of a truth T [n rows, K] and up to four predictions P_q (column k of P_q is
// column map_q[k] of its base), the sums behind the reference's per-column numbers, in float64:
//   se = sum (p - t)^2,  ae = sum |p - t|,  corr = sum (t - tm)(p - pm) / (||t - tm|| ||p - pm|| + 1e-8).
// The centred sums come from one pass over values shifted by the column's first row (t' = t - t[row 0],
// p' = p - p[row 0]), so a column whose mean is 1e4 standard deviations from 0 loses nothing to cancellation and a
// constant column has exactly zero centred sums (corr = 0 / 1e-8 = 0).  Two launches with a fixed order: the
// partial kernel sums fixed chunks of rows, the combine kernel sums the chunks of a column in a fixed tree
// (csrc/colsum.h, which also says why a column's result depends on its own data and n only).
//
// Accumulate.  Adds the column results of one or more samples into the float64 state of StreamingMetrics objects
// (one job per object), in the reference's order.
//
// Regrid + blend.  Bilinear interpolation with host-built tables (cell, four float64 weights), summed in float64 in
// scipy's order and rounded once to float32; optionally the taper blend m r + (1 - m) g in float32.
#include "colsum.h"
#include "common.h"

namespace {

using gcl::chunk_rows;
using gcl::kColTile;
using gcl::kRowLanes;
using gcl::num_chunks;
using gcl::rounded;  // products rounded on their own, never contracted (common.h)

constexpr int kMaxPred = 4;

struct Preds {
  const float* p[kMaxPred];
  int64_t ld[kMaxPred];
  int64_t bs[kMaxPred];
  const int32_t* map[kMaxPred];
};

// Sums per column, in this order: St, Stt, then per prediction Sp, Spp, Stp, Sse, Sae.
template <int NP>
struct Acc {
  static constexpr int NS = 2 + 5 * NP;
  double v[NS];
};

// Partial sums of chunk blockIdx.x, columns [kColTile * blockIdx.y, ...), sample blockIdx.z.
// part layout: [B][K][NS][nchunk] (a column's chunks contiguous for the combine kernel).
template <int NP>
__global__ __launch_bounds__(256) void colstats_partial_kernel(const float* __restrict__ T, int64_t ldt, int64_t bst,
                                                               Preds P, const int32_t* __restrict__ rows, int32_t n,
                                                               int32_t K, double* __restrict__ part) {
  constexpr int NS = Acc<NP>::NS;
  __shared__ double red[NS][256];
  const int tid = threadIdx.x;
  const int cl = tid % kColTile, lane_r = tid / kColTile;
  const int c = blockIdx.y * kColTile + cl;
  const int ch = blockIdx.x, b = blockIdx.z;
  const int crow = chunk_rows(n), nchunk = num_chunks(n);
  const int i0 = ch * crow, i1 = min(n, i0 + crow);
  const bool live = c < K;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  if (live) {
    const float* Tb = T + (int64_t)b * bst + c;
    const float* pb[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) pb[q] = P.p[q] + (int64_t)b * P.bs[q] + (P.map[q] ? P.map[q][c] : c);
    const int64_t r0 = rows ? rows[0] : 0;
    const double t0 = (double)Tb[r0 * ldt];
    double p0[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) p0[q] = (double)pb[q][r0 * P.ld[q]];
    // Positions i0 + lane_r + kRowLanes * j, j ascending: fixed per (n, position) whatever K is.
    constexpr int U = 4;
    for (int i = i0 + lane_r; i < i1; i += U * kRowLanes) {
      float tv[U], pv[U][NP];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int ii = i + u * kRowLanes;
        if (ii < i1) {
          const int64_t r = rows ? rows[ii] : ii;
          tv[u] = Tb[r * ldt];
#pragma unroll
          for (int q = 0; q < NP; ++q) pv[u][q] = pb[q][r * P.ld[q]];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i + u * kRowLanes < i1) {
          const double t = (double)tv[u] - t0;
          acc[0] += t;
          acc[1] = fma(t, t, acc[1]);
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            const double pd = (double)pv[u][q];
            const double p = pd - p0[q];
            const double d = pd - (double)tv[u];
            acc[2 + 5 * q] += p;
            acc[3 + 5 * q] = fma(p, p, acc[3 + 5 * q]);
            acc[4 + 5 * q] = fma(t, p, acc[4 + 5 * q]);
            acc[5 + 5 * q] = fma(d, d, acc[5 + 5 * q]);
            acc[6 + 5 * q] += fabs(d);
          }
        }
      }
    }
  }
  gcl::lanes_to_part(red, acc, tid, kRowLanes, kColTile, lane_r == 0 && live,
                     part + ((int64_t)b * K + c) * NS * nchunk + ch, nchunk);
}

// One block per (column blockIdx.x, sample blockIdx.y): the column's chunks in a fixed tree, then the three results
// per prediction, stats[((b * NP + q) * K + k) * 3 + {0: se, 1: ae, 2: corr}].
template <int NP>
__global__ __launch_bounds__(256) void colstats_combine_kernel(const double* __restrict__ part, int32_t n, int32_t K,
                                                               double* __restrict__ stats) {
  constexpr int NS = Acc<NP>::NS;
  __shared__ double red[NS][256];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int nchunk = num_chunks(n);
  const double* src = part + ((int64_t)b * K + k) * NS * nchunk;
  for (int s = 0; s < NS; ++s) red[s][tid] = gcl::strided_sum(src + (int64_t)s * nchunk, nchunk, tid);
  gcl::block_tree_sum(red, tid);
  if (tid < NP) {
    const int q = tid;
    const double N = (double)n;
    const double St = red[0][0], Stt = red[1][0];
    const double Sp = red[2 + 5 * q][0], Spp = red[3 + 5 * q][0], Stp = red[4 + 5 * q][0];
    const double vt = fmax(Stt - St * (St / N), 0.0);
    const double vp = fmax(Spp - Sp * (Sp / N), 0.0);
    const double cov = Stp - St * (Sp / N);
    double* o = stats + (((int64_t)b * NP + q) * K + k) * 3;
    o[0] = red[5 + 5 * q][0];
    o[1] = red[6 + 5 * q][0];
    o[2] = n > 0 ? cov / (sqrt(vt) * sqrt(vp) + 1e-8) : 0.0;
  }
}

// One wave per job.  A job (int64 x 8): {stats offset of its first column of sample 0 (doubles), doubles between
// samples, columns, channels C, state offset (doubles), mask offset (bytes, -1: none), rows per column, samples}.
// State of an object (C channels, float64): [sum_se, sum_ae, n, total_elem, sum_se_per_ch[C], sum_acc[C],
// elem_per_ch[C], acc_count[C]].  Per sample, in the reference's order: lane ch adds column ch, ch + C, ... of its
// channel (ascending); lane 0 forms the sample's sums over the columns of non-excluded channels (ascending, from 0)
// and adds them to sum_se / sum_ae.
constexpr int kJobFields = 8;

__global__ __launch_bounds__(64) void accumulate_kernel(const double* __restrict__ stats, const int64_t* __restrict__ jobs,
                                                        int32_t njobs, double* __restrict__ state,
                                                        const uint8_t* __restrict__ masks) {
  const int j = blockIdx.x;
  if (j >= njobs) return;
  const int64_t* jb = jobs + (int64_t)j * kJobFields;
  const int64_t off = jb[0], bstride = jb[1];
  const int ncols = (int)jb[2], C = (int)jb[3];
  double* st = state + jb[4];
  const uint8_t* mask = jb[5] >= 0 ? masks + jb[5] : nullptr;
  const double nrows = (double)jb[6];
  const int B = (int)jb[7];
  double* se_ch = st + 4;
  double* acc_ch = se_ch + C;
  double* elem_ch = acc_ch + C;
  double* cnt_ch = elem_ch + C;
  for (int b = 0; b < B; ++b) {
    const double* sb = stats + off + (int64_t)b * bstride;
    for (int ch = threadIdx.x; ch < C; ch += 64) {
      for (int c = ch; c < ncols; c += C) {
        se_ch[ch] += sb[(int64_t)c * 3 + 0];
        acc_ch[ch] += sb[(int64_t)c * 3 + 2];
        elem_ch[ch] += nrows;
        cnt_ch[ch] += 1.0;
      }
    }
    if (threadIdx.x == 0) {
      double se = 0.0, ae = 0.0, cols = 0.0;
      for (int c = 0; c < ncols; ++c) {
        if (mask && mask[c % C]) continue;
        se += sb[(int64_t)c * 3 + 0];
        ae += sb[(int64_t)c * 3 + 1];
        cols += 1.0;
      }
      if (cols > 0.0) {
        st[0] += se;
        st[1] += ae;
        st[3] += cols * nrows;
      }
      st[2] += 1.0;
    }
  }
}

// g[b, i, k] = fp32( v00 w0 + v01 w1 + v10 w2 + v11 w3 ) in float64, left to right, each product rounded on its own:
// v00 = src[b, ilon * nlat + ilat, k], v01 = (ilon, ilat + 1), v10 = (ilon + 1, ilat), v11 = (ilon + 1, ilat + 1).
// With a mask: out[b, i, k] = m[i] r[b, i, k] + (1 - m[i]) g  in float32 (src/predict_pipeline.py:326 order).
template <typename TS>
__global__ __launch_bounds__(256) void regrid_kernel(const TS* __restrict__ src, int64_t lds, int64_t bss, int32_t nlat,
                                                     const int32_t* __restrict__ cell, const double* __restrict__ w,
                                                     int32_t nt, int32_t K, float* g, int64_t ldg, int64_t bsg,
                                                     const float* __restrict__ mask, const float* __restrict__ r,
                                                     int64_t ldr, int64_t bsr, float* out, int64_t ldo, int64_t bso,
                                                     int32_t B) {
  const int64_t total = (int64_t)B * nt * K;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % K);
    const int64_t rem = t / K;
    const int i = (int)(rem % nt);
    const int64_t b = rem / nt;
    const int64_t n00 = (int64_t)cell[2 * i] * nlat + cell[2 * i + 1];
    const TS* s = src + b * bss + k;
    const float gv = (float)gcl::cell_corner_sum(s, lds, n00, nlat, w + 4 * (int64_t)i);
    if (g) g[b * bsg + (int64_t)i * ldg + k] = gv;
    if (out) {
      const float m = mask[i];
      out[b * bso + (int64_t)i * ldo + k] = rounded(m * r[b * bsr + (int64_t)i * ldr + k]) + rounded((1.0f - m) * gv);
    }
  }
}

// out[b, i, k] = m[i] r[b, i, k] + (1 - m[i]) g[b, i, k]  (float32, one rounding per operation)
__global__ __launch_bounds__(256) void blend_kernel(const float* __restrict__ mask, const float* __restrict__ r,
                                                    int64_t ldr, int64_t bsr, const float* __restrict__ g, int64_t ldg,
                                                    int64_t bsg, float* out, int64_t ldo, int64_t bso, int32_t nt,
                                                    int32_t K, int32_t B) {
  const int64_t total = (int64_t)B * nt * K;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % K);
    const int64_t rem = t / K;
    const int i = (int)(rem % nt);
    const int64_t b = rem / nt;
    const float m = mask[i];
    out[b * bso + (int64_t)i * ldo + k] =
        rounded(m * r[b * bsr + (int64_t)i * ldr + k]) + rounded((1.0f - m) * g[b * bsg + (int64_t)i * ldg + k]);
  }
}

template <int NP>
int launch_colstats(hipStream_t st, const float* T, int64_t ldt, int64_t bst, const Preds& P, const int32_t* rows,
                    int32_t n, int32_t K, int32_t B, double* stats, double* part) {
  const int nchunk = num_chunks(n);
  hipLaunchKernelGGL(colstats_partial_kernel<NP>, dim3(nchunk, (unsigned)gcl::cdiv(K, kColTile), B), dim3(256), 0, st,
                     T, ldt, bst, P, rows, n, K, part);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(colstats_combine_kernel<NP>, dim3(K, B), dim3(256), 0, st, (const double*)part, n, K, stats);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // namespace

extern "C" size_t gcl_verify_colstats_ws_bytes(int32_t n, int32_t K, int32_t npred, int32_t B) {
  if (n <= 0 || K <= 0 || npred <= 0 || B <= 0) return 0;
  return (size_t)B * K * (2 + 5 * npred) * num_chunks(n) * sizeof(double);
}

extern "C" int gcl_verify_colstats(const float* truth, int64_t ldt, int64_t bst, int32_t K, int32_t npred,
                                   const float* p0, int64_t ld0, int64_t bs0, const int32_t* map0, const float* p1,
                                   int64_t ld1, int64_t bs1, const int32_t* map1, const float* p2, int64_t ld2,
                                   int64_t bs2, const int32_t* map2, const float* p3, int64_t ld3, int64_t bs3,
                                   const int32_t* map3, const int32_t* rows, int32_t n, int32_t B, double* stats,
                                   void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(truth && stats, "verify_colstats: null argument");
  GCL_CHECK_ARG(npred >= 1 && npred <= kMaxPred, "verify_colstats: npred=%d outside [1, %d]", npred, kMaxPred);
  GCL_CHECK_ARG(K > 0 && n > 0 && B > 0, "verify_colstats: bad shape (K=%d, n=%d, B=%d)", K, n, B);
  GCL_CHECK_ARG(K <= 65535 && B <= 65535, "verify_colstats: K=%d or B=%d above 65535", K, B);
  Preds P{};
  const float* ps[kMaxPred] = {p0, p1, p2, p3};
  const int64_t lds[kMaxPred] = {ld0, ld1, ld2, ld3}, bss[kMaxPred] = {bs0, bs1, bs2, bs3};
  const int32_t* maps[kMaxPred] = {map0, map1, map2, map3};
  for (int q = 0; q < npred; ++q) {
    GCL_CHECK_ARG(ps[q], "verify_colstats: prediction %d is null", q);
    P.p[q] = ps[q], P.ld[q] = lds[q], P.bs[q] = bss[q], P.map[q] = maps[q];
  }
  const size_t need = gcl_verify_colstats_ws_bytes(n, K, npred, B);
  GCL_CHECK_ARG(ws && ws_bytes >= need, "verify_colstats: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  switch (npred) {
    case 1: return launch_colstats<1>(st, truth, ldt, bst, P, rows, n, K, B, stats, part);
    case 2: return launch_colstats<2>(st, truth, ldt, bst, P, rows, n, K, B, stats, part);
    case 3: return launch_colstats<3>(st, truth, ldt, bst, P, rows, n, K, B, stats, part);
    default: return launch_colstats<4>(st, truth, ldt, bst, P, rows, n, K, B, stats, part);
  }
}

extern "C" int gcl_verify_accumulate(const double* stats, const int64_t* jobs, int32_t njobs, double* state,
                                     const uint8_t* masks, gcl_stream_t stream) {
  GCL_CHECK_ARG(stats && jobs && state, "verify_accumulate: null argument");
  GCL_CHECK_ARG(njobs >= 0, "verify_accumulate: njobs=%d", njobs);
  if (njobs == 0) return GCL_OK;
  hipLaunchKernelGGL(accumulate_kernel, dim3(njobs), dim3(64), 0, (hipStream_t)stream, stats, jobs, njobs, state, masks);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_regrid_blend(const void* src, int32_t src_f64, int64_t lds, int64_t bss, int32_t nlat,
                                const int32_t* cell, const double* w, int32_t nt, int32_t K, float* g, int64_t ldg,
                                int64_t bsg, const float* mask, const float* r, int64_t ldr, int64_t bsr, float* out,
                                int64_t ldo, int64_t bso, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(src && cell && w, "regrid_blend: null argument");
  GCL_CHECK_ARG(g || out, "regrid_blend: neither g nor out given");
  GCL_CHECK_ARG(!out || (mask && r), "regrid_blend: the blend needs mask and r");
  GCL_CHECK_ARG(nt >= 0 && K > 0 && B > 0 && nlat >= 2, "regrid_blend: bad shape");
  const int64_t total = (int64_t)B * nt * K;
  if (total == 0) return GCL_OK;
  const hipStream_t st = (hipStream_t)stream;
  if (src_f64)
    hipLaunchKernelGGL(regrid_kernel<double>, dim3(gcl::grid_for(total, 8192)), dim3(256), 0, st, (const double*)src, lds, bss,
                       nlat, cell, w, nt, K, g, ldg, bsg, mask, r, ldr, bsr, out, ldo, bso, B);
  else
    hipLaunchKernelGGL(regrid_kernel<float>, dim3(gcl::grid_for(total, 8192)), dim3(256), 0, st, (const float*)src, lds, bss,
                       nlat, cell, w, nt, K, g, ldg, bsg, mask, r, ldr, bsr, out, ldo, bso, B);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_taper_blend(const float* mask, const float* r, int64_t ldr, int64_t bsr, const float* g,
                               int64_t ldg, int64_t bsg, float* out, int64_t ldo, int64_t bso, int32_t nt, int32_t K,
                               int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(mask && r && g && out, "taper_blend: null argument");
  GCL_CHECK_ARG(nt >= 0 && K > 0 && B > 0, "taper_blend: bad shape");
  const int64_t total = (int64_t)B * nt * K;
  if (total == 0) return GCL_OK;
  hipLaunchKernelGGL(blend_kernel, dim3(gcl::grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream, mask, r, ldr, bsr, g, ldg,
                     bsg, out, ldo, bso, nt, K, B);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
