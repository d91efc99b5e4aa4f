// Training and scoring the regional heads without leaving the device (scripts/train_dual_mesh.py):
//   * the cache of the frozen global model's outputs (`--precompute`, :548-580) kept in HBM, one float32 record per
//     sample in the layout the regional kernels read, written by one launch per precomputed batch and read back by one
//     launch per step through a DEVICE slot array - a captured step replays with another sample by changing 8 bytes;
//   * the per-step body of eval_dual (:318-356, cached :289-308): the corrected and the global-only prediction advance
//     in lock-step and their ROI losses are added into a float64 state on the device.
//
// Record (all float32; every row is padded with zeros to a multiple of 4 floats, so every part starts on a 16-byte
// boundary of a 16-byte aligned cache):
//   roi3 [n_roi, Sp]   = [X[rows[i]] | latent[rows[i]] | 0],  Sp  = roundup(XF + D, 4)     (XF = obs * C)
//   send [half_E, Dgp] = [mesh[snd[k]] | 0],                  Dgp = roundup(Dm, 4)
//   pred [n_roi, Cp]   = [pred[rows[i]] | 0],                 Cp  = roundup(C, 4)
//   y    [n_roi, Yp]   = [y[rows[i]] | 0],                    Yp  = roundup(P * C, 4)
// No kernel here allocates, synchronises or uses atomics; the reductions have a fixed order.
#include "colsum.h"
#include "common.h"

namespace {

inline int32_t up4(int64_t v) { return (int32_t)((v + 3) / 4 * 4); }

// Sizes of one record in 16-byte quads.
struct RecLayout {
  int32_t XF, D, Dm, C, YF;         // used columns
  int32_t Sp, Dgp, Cp, Yp;          // padded row widths (floats)
  int64_t q_roi, q_send, q_pred, q_y, q_rec;
};

inline RecLayout make_layout(int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C, int32_t P) {
  RecLayout L;
  L.XF = XF, L.D = D, L.Dm = Dm, L.C = C, L.YF = P * C;
  L.Sp = up4((int64_t)XF + D), L.Dgp = up4(Dm), L.Cp = up4(C), L.Yp = up4((int64_t)P * C);
  L.q_roi = (int64_t)n_roi * (L.Sp / 4);
  L.q_send = (int64_t)half_E * (L.Dgp / 4);
  L.q_pred = (int64_t)n_roi * (L.Cp / 4);
  L.q_y = (int64_t)n_roi * (L.Yp / 4);
  L.q_rec = L.q_roi + L.q_send + L.q_pred + L.q_y;
  return L;
}

inline bool shape_ok(int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C, int32_t P) {
  const int64_t lim = 1 << 24;  // keeps every width sum and P * C inside int32
  return n_roi > 0 && half_E >= 0 && XF > 0 && D >= 0 && Dm >= 0 && C > 0 && P > 0 && XF < lim && D < lim && Dm < lim &&
         C < lim && (int64_t)P * C < lim && (half_E == 0 || Dm > 0);
}

__device__ __forceinline__ bool dev_aligned16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Columns c .. c+3 of the row [r0[0 .. w0) | r1[0 .. w1) | 0]: one 16-byte load when the quad lies inside one source on
// a 16-byte boundary, else per column (adjacent lanes still read adjacent addresses).  r1 may be NULL when w1 == 0.
__device__ __forceinline__ float4 row_quad(const float* r0, int w0, const float* r1, int w1, int c) {
  if (c + 4 <= w0 && dev_aligned16(r0 + c)) return gcl::ld4(r0 + c);
  if (c >= w0 && c - w0 + 4 <= w1 && dev_aligned16(r1 + (c - w0))) return gcl::ld4(r1 + (c - w0));
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int cc = c + j;
    float x = 0.f;
    if (cc < w0)
      x = r0[cc];
    else if (cc - w0 < w1)
      x = r1[cc - w0];
    v[j] = x;
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

struct StoreSrc {
  const float *pred, *lat, *mesh, *X, *y;
  int64_t ldp, bsp, ldl, bsl, ldm, bsm, ldx, bsx, ldy, bsy;
};

// One thread per 16-byte quad of the B records.  A row index outside its source gives a zero row (as
// gcl_roi_gather_rows); a slot outside [0, n_slots) writes nothing.
__global__ __launch_bounds__(256) void region_store_kernel(StoreSrc s, RecLayout L, const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ snd,
                                                           const int64_t* __restrict__ slots, float* __restrict__ cache,
                                                           int64_t n_slots, int32_t B, int32_t G, int32_t M) {
  const int64_t total = (int64_t)B * L.q_rec;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int64_t b = t / L.q_rec;
    const int64_t qq = t - b * L.q_rec;
    const int64_t slot = slots[b];
    if (slot < 0 || slot >= n_slots) continue;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t q = qq;
    if (q < L.q_roi) {
      const int Q = L.Sp / 4;
      const int i = (int)(q / Q), c = 4 * (int)(q % Q);
      const int g = rows[i];
      if (g >= 0 && g < G)
        v = row_quad(s.X + b * s.bsx + (int64_t)g * s.ldx, L.XF, L.D ? s.lat + b * s.bsl + (int64_t)g * s.ldl : nullptr,
                     L.D, c);
    } else if ((q -= L.q_roi) < L.q_send) {
      const int Q = L.Dgp / 4;
      const int k = (int)(q / Q), c = 4 * (int)(q % Q);
      const int g = snd[k];
      if (g >= 0 && g < M) v = row_quad(s.mesh + b * s.bsm + (int64_t)g * s.ldm, L.Dm, nullptr, 0, c);
    } else if ((q -= L.q_send) < L.q_pred) {
      const int Q = L.Cp / 4;
      const int i = (int)(q / Q), c = 4 * (int)(q % Q);
      const int g = rows[i];
      if (g >= 0 && g < G) v = row_quad(s.pred + b * s.bsp + (int64_t)g * s.ldp, L.C, nullptr, 0, c);
    } else {
      q -= L.q_pred;
      const int Q = L.Yp / 4;
      const int i = (int)(q / Q), c = 4 * (int)(q % Q);
      const int g = rows[i];
      if (g >= 0 && g < G) v = row_quad(s.y + b * s.bsy + (int64_t)g * s.ldy, L.YF, nullptr, 0, c);
    }
    gcl::st4(cache + (slot * L.q_rec + qq) * 4, v);
  }
}

struct FetchDst {
  float* p[4];     // roi3, send, pred, y (NULL: that part is not wanted)
  int64_t bs[4];   // sample stride of each, in floats
};

// One thread per quad of the B fetched records: a 16-byte load from the record, a 16-byte store to the part's buffer.
// A slot outside [0, n_slots) reads nothing and stores zeros.
__global__ __launch_bounds__(256) void region_fetch_kernel(const float* __restrict__ cache, int64_t n_slots,
                                                           const int64_t* __restrict__ slots, int32_t B, RecLayout L,
                                                           FetchDst d) {
  const int64_t total = (int64_t)B * L.q_rec;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int64_t b = t / L.q_rec;
    const int64_t qq = t - b * L.q_rec;
    const int64_t slot = slots[b];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (slot >= 0 && slot < n_slots) v = gcl::ld4(cache + (slot * L.q_rec + qq) * 4);
    int part = 0;
    int64_t q = qq;
    if (q >= L.q_roi) {
      q -= L.q_roi, part = 1;
      if (q >= L.q_send) {
        q -= L.q_send, part = 2;
        if (q >= L.q_pred) q -= L.q_pred, part = 3;
      }
    }
    float* dst = part == 0 ? d.p[0] : part == 1 ? d.p[1] : part == 2 ? d.p[2] : d.p[3];
    const int64_t bs = part == 0 ? d.bs[0] : part == 1 ? d.bs[1] : part == 2 ? d.bs[2] : d.bs[3];
    if (dst) gcl::st4(dst + b * bs + q * 4, v);
  }
}

// ---- eval pair ----------------------------------------------------------------------------------------------------
constexpr int kPairChunk = 2048;  // elements of one partial sum: 256 threads x 8, a function of nothing else

struct PairIn {
  const float* delta[2];
  int64_t ldd[2], bsd[2];
  const float* win[2];  // the input window [B, G, obs * C] with (ld, bs); x_last is its last slot
  int64_t ldw[2], bsw[2];
  float* new_win[2];    // contiguous [B, G, obs, C] or NULL
  float* out[2];        // step_out [B, G, C] with (ld, bs) or NULL
  int64_t ldo[2], bso[2];
  const float* y;
  int64_t ldy, bsy;
  const int32_t* chan_kind;
  int32_t residual, obs, nq;
};

// step_out of prediction q at (b, g, c): the arithmetic of ar_advance_kernel (csrc/misc.hip).
__device__ __forceinline__ float pair_predict(const PairIn& a, int q, int64_t b, int64_t g, int c, int C) {
  const float xl = a.win[q][b * a.bsw[q] + g * a.ldw[q] + (int64_t)(a.obs - 1) * C + c];
  float v = a.delta[q][b * a.bsd[q] + g * a.ldd[q] + c];
  if (a.residual) v += xl;
  const int kind = a.chan_kind ? a.chan_kind[c] : 0;
  if (kind == 1) v = xl;
  else if (kind == 2) v = a.y[b * a.bsy + g * a.ldy + c];
  return v;
}

// step_out and the shifted window of every prediction over the whole grid.  K = obs when a window is written, else 1
// (only the new slot is visited).
template <int NQ>
__global__ __launch_bounds__(256) void pair_advance_kernel(PairIn a, int32_t B, int32_t G, int32_t C, int32_t K) {
  const int obs = a.obs;
  const int64_t total = (int64_t)B * G * K * C;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    const int c = (int)(idx % C);
    const int k = K == 1 ? obs - 1 : (int)((idx / C) % K);
    const int64_t bg = idx / ((int64_t)C * K);
    const int64_t g = bg % G, b = bg / G;
    const int64_t widx = (bg * obs + k) * C + c;  // position in a contiguous [B, G, obs, C] window
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (k < obs - 1) {
        if (a.new_win[q]) a.new_win[q][widx] = a.win[q][b * a.bsw[q] + g * a.ldw[q] + (int64_t)(k + 1) * C + c];
      } else {
        const float v = pair_predict(a, q, b, g, c, C);
        if (a.new_win[q]) a.new_win[q][widx] = v;
        if (a.out[q]) a.out[q][b * a.bso[q] + g * a.ldo[q] + c] = v;
      }
    }
  }
}

// Stage 1: block j sums the squared errors of elements [j * 2048, (j + 1) * 2048) of the [B, n, C] loss rows: thread t
// takes t, t + 256, .. in ascending order, the block adds its threads in a fixed tree.  part[q * nchunk + j].
template <int NQ>
__global__ __launch_bounds__(256) void pair_partial_kernel(PairIn a, const int32_t* __restrict__ rows, int32_t n,
                                                           int32_t B, int32_t G, int32_t C, int64_t nchunk,
                                                           double* __restrict__ part) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)B * n * C;
  const int64_t e0 = (int64_t)blockIdx.x * kPairChunk;
  double acc[2] = {0.0, 0.0};
  for (int k = 0; k < kPairChunk / 256; ++k) {
    const int64_t e = e0 + tid + 256 * k;
    if (e >= total) break;
    const int c = (int)(e % C);
    const int64_t r = e / C;
    const int i = (int)(r % n);
    const int64_t b = r / n;
    const int g = rows ? rows[i] : i;
    if (g < 0 || g >= G) continue;  // a bad row index reads nothing
    const double yv = (double)a.y[b * a.bsy + (int64_t)g * a.ldy + c];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double dq = (double)pair_predict(a, q, b, g, c, C) - yv;
      acc[q] = fma(dq, dq, acc[q]);
    }
  }
  red[0][tid] = acc[0], red[1][tid] = acc[1];
  gcl::block_tree_sum(red, tid);
  if (tid < NQ) part[(int64_t)tid * nchunk + blockIdx.x] = red[tid][0];
}

// Stage 2, one block: thread t sums partials t, t + 256, .. ascending, a fixed tree over the threads, and thread q adds
// weight * sum / (B n C) into acc[q].
__global__ __launch_bounds__(256) void pair_combine_kernel(const double* __restrict__ part, int64_t nchunk, int32_t nq,
                                                           double scale, double* __restrict__ acc) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  for (int q = 0; q < 2; ++q) red[q][tid] = q < nq ? gcl::strided_sum(part + (int64_t)q * nchunk, nchunk, tid) : 0.0;
  gcl::block_tree_sum(red, tid);
  if (tid < nq) acc[tid] += scale * red[tid][0];
}

inline int64_t pair_chunks(int32_t B, int32_t n, int32_t C) { return gcl::cdiv((int64_t)B * n * C, kPairChunk); }

}  // namespace

extern "C" size_t gcl_region_cache_record_bytes(int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm,
                                                int32_t C, int32_t P) {
  if (!shape_ok(n_roi, half_E, XF, D, Dm, C, P)) return 0;
  return (size_t)make_layout(n_roi, half_E, XF, D, Dm, C, P).q_rec * 16;
}

extern "C" int gcl_region_cache_store(const float* pred, int64_t ldp, int64_t bsp, const float* lat, int64_t ldl,
                                      int64_t bsl, const float* mesh, int64_t ldm, int64_t bsm, const float* X,
                                      int64_t ldx, int64_t bsx, const float* y, int64_t ldy, int64_t bsy,
                                      const int32_t* rows, const int32_t* snd, const int64_t* slots, float* cache,
                                      int64_t n_slots, int32_t B, int32_t G, int32_t M, int32_t n_roi, int32_t half_E,
                                      int32_t XF, int32_t D, int32_t Dm, int32_t C, int32_t P, gcl_stream_t stream) {
  GCL_CHECK_ARG(shape_ok(n_roi, half_E, XF, D, Dm, C, P),
                "region_cache_store: bad record shape (n_roi=%d, half_E=%d, XF=%d, D=%d, Dm=%d, C=%d, P=%d)", n_roi,
                half_E, XF, D, Dm, C, P);
  GCL_CHECK_ARG(pred && X && y && rows && slots && cache && (!D || lat) && (!half_E || (mesh && snd)),
                "region_cache_store: null argument");
  GCL_CHECK_ARG(B > 0 && G > 0 && M >= 0 && n_slots > 0, "region_cache_store: bad shape (B=%d, G=%d, M=%d, n_slots=%lld)",
                B, G, M, (long long)n_slots);
  GCL_CHECK_ARG(ldp >= C && ldx >= XF && ldy >= (int64_t)P * C && (!D || ldl >= D) && (!half_E || ldm >= Dm),
                "region_cache_store: a source row stride is smaller than its width");
  GCL_CHECK_ARG(gcl::aligned16(cache), "region_cache_store: the cache must be 16-byte aligned");
  const RecLayout L = make_layout(n_roi, half_E, XF, D, Dm, C, P);
  StoreSrc s{pred, lat, mesh, X, y, ldp, bsp, ldl, bsl, ldm, bsm, ldx, bsx, ldy, bsy};
  hipLaunchKernelGGL(region_store_kernel, dim3(gcl::grid_for((int64_t)B * L.q_rec)), dim3(256), 0, (hipStream_t)stream,
                     s, L, rows, snd, slots, cache, n_slots, B, G, M);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_region_cache_fetch(const float* cache, int64_t n_slots, const int64_t* slots, int32_t B,
                                      int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C,
                                      int32_t P, float* roi3, int64_t bs_roi, float* send, int64_t bs_send, float* pred,
                                      int64_t bs_pred, float* y, int64_t bs_y, gcl_stream_t stream) {
  GCL_CHECK_ARG(shape_ok(n_roi, half_E, XF, D, Dm, C, P),
                "region_cache_fetch: bad record shape (n_roi=%d, half_E=%d, XF=%d, D=%d, Dm=%d, C=%d, P=%d)", n_roi,
                half_E, XF, D, Dm, C, P);
  GCL_CHECK_ARG(cache && slots && B > 0 && n_slots > 0, "region_cache_fetch: bad argument (B=%d, n_slots=%lld)", B,
                (long long)n_slots);
  GCL_CHECK_ARG(roi3 || send || pred || y, "region_cache_fetch: no destination");
  const RecLayout L = make_layout(n_roi, half_E, XF, D, Dm, C, P);
  FetchDst d{{roi3, send, pred, y}, {bs_roi, bs_send, bs_pred, bs_y}};
  const int64_t need[4] = {L.q_roi * 4, L.q_send * 4, L.q_pred * 4, L.q_y * 4};
  for (int k = 0; k < 4; ++k) {
    GCL_CHECK_ARG(!d.p[k] || (gcl::aligned16(d.p[k]) && d.bs[k] % 4 == 0 && (B == 1 || d.bs[k] >= need[k])),
                  "region_cache_fetch: destination %d must be 16-byte aligned with a sample stride of at least %lld floats "
                  "(a multiple of 4), got %lld",
                  k, (long long)need[k], (long long)d.bs[k]);
  }
  GCL_CHECK_ARG(gcl::aligned16(cache), "region_cache_fetch: the cache must be 16-byte aligned");
  hipLaunchKernelGGL(region_fetch_kernel, dim3(gcl::grid_for((int64_t)B * L.q_rec)), dim3(256), 0, (hipStream_t)stream,
                     cache, n_slots, slots, B, L, d);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" size_t gcl_region_eval_pair_ws_bytes(int32_t nq, int32_t B, int32_t n, int32_t C) {
  if (nq < 1 || nq > 2 || B <= 0 || n <= 0 || C <= 0) return 0;
  return (size_t)nq * pair_chunks(B, n, C) * sizeof(double);
}

extern "C" int gcl_region_eval_pair(int32_t nq, const float* delta0, int64_t ldd0, int64_t bsd0, const float* win0,
                                    int64_t ldw0, int64_t bsw0, float* new_win0, float* out0, int64_t ldo0, int64_t bso0,
                                    const float* delta1, int64_t ldd1, int64_t bsd1, const float* win1, int64_t ldw1,
                                    int64_t bsw1, float* new_win1, float* out1, int64_t ldo1, int64_t bso1,
                                    const float* y_step, int64_t ldy, int64_t bsy, const int32_t* chan_kind,
                                    int32_t residual, const int32_t* rows, int32_t n, double weight, double* acc,
                                    int32_t B, int32_t G, int32_t obs, int32_t C, void* ws, size_t ws_bytes,
                                    gcl_stream_t stream) {
  GCL_CHECK_ARG(nq == 1 || nq == 2, "region_eval_pair: nq=%d, one or two predictions", nq);
  GCL_CHECK_ARG(delta0 && win0 && y_step && acc && (nq == 1 || (delta1 && win1)), "region_eval_pair: null argument");
  GCL_CHECK_ARG(B > 0 && G > 0 && obs >= 1 && C > 0 && n > 0, "region_eval_pair: bad shape (B=%d, G=%d, obs=%d, C=%d, n=%d)",
                B, G, obs, C, n);
  GCL_CHECK_ARG(rows || n <= G, "region_eval_pair: identity rows with n=%d above G=%d", n, G);
  const int64_t wC = (int64_t)obs * C;
  GCL_CHECK_ARG(ldd0 >= C && ldw0 >= wC && ldy >= C && (nq == 1 || (ldd1 >= C && ldw1 >= wC)),
                "region_eval_pair: a row stride is smaller than its width");
  GCL_CHECK_ARG((!out0 || ldo0 >= C) && (nq == 1 || !out1 || ldo1 >= C), "region_eval_pair: output row stride smaller than C");
  GCL_CHECK_ARG((!new_win0 || new_win0 != win0) && (nq == 1 || !new_win1 || new_win1 != win1),
                "region_eval_pair: the window shift cannot be done in place");
  GCL_CHECK_ARG((!out0 || (out0 != delta0 && out0 != win0)) && (nq == 1 || !out1 || (out1 != delta1 && out1 != win1)),
                "region_eval_pair: out may not be the delta or the window (the loss pass forms step_out from them again)");
  const size_t need = gcl_region_eval_pair_ws_bytes(nq, B, n, C);
  GCL_CHECK_ARG(ws && ws_bytes >= need, "region_eval_pair: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  PairIn a{};
  a.delta[0] = delta0, a.ldd[0] = ldd0, a.bsd[0] = bsd0, a.win[0] = win0, a.ldw[0] = ldw0, a.bsw[0] = bsw0;
  a.new_win[0] = new_win0, a.out[0] = out0, a.ldo[0] = ldo0, a.bso[0] = bso0;
  if (nq == 2) {
    a.delta[1] = delta1, a.ldd[1] = ldd1, a.bsd[1] = bsd1, a.win[1] = win1, a.ldw[1] = ldw1, a.bsw[1] = bsw1;
    a.new_win[1] = new_win1, a.out[1] = out1, a.ldo[1] = ldo1, a.bso[1] = bso1;
  }
  a.y = y_step, a.ldy = ldy, a.bsy = bsy, a.chan_kind = chan_kind, a.residual = residual, a.obs = obs, a.nq = nq;
  const bool any_win = a.new_win[0] || a.new_win[1];
  if (any_win || a.out[0] || a.out[1]) {
    const int32_t K = any_win ? obs : 1;
    const dim3 grid(gcl::grid_for((int64_t)B * G * K * C, 8192));
    if (nq == 2)
      hipLaunchKernelGGL(pair_advance_kernel<2>, grid, dim3(256), 0, st, a, B, G, C, K);
    else
      hipLaunchKernelGGL(pair_advance_kernel<1>, grid, dim3(256), 0, st, a, B, G, C, K);
    GCL_CHECK_LAUNCH();
  }
  const int64_t nchunk = pair_chunks(B, n, C);
  GCL_CHECK_ARG(nchunk <= 0x7fffffff, "region_eval_pair: B * n * C too large");
  double* part = (double*)ws;
  if (nq == 2)
    hipLaunchKernelGGL(pair_partial_kernel<2>, dim3((unsigned)nchunk), dim3(256), 0, st, a, rows, n, B, G, C, nchunk, part);
  else
    hipLaunchKernelGGL(pair_partial_kernel<1>, dim3((unsigned)nchunk), dim3(256), 0, st, a, rows, n, B, G, C, nchunk, part);
  GCL_CHECK_LAUNCH();
  const double scale = weight / ((double)B * (double)n * (double)C);
  hipLaunchKernelGGL(pair_combine_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nchunk, nq, scale, acc);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
