// Dense per-node transforms for K, N <= 64 on the bf16 matrix pipe with 3-way operand splitting (x3.h):
// fp32 in, fp32 out, fp32-GEMM accuracy, 0.375x the matrix-pipe time of the fp32-operand instruction.
// Same contracts as the fp32 kernels of linear.hip (nn.Linear + preceding PReLU of MLP.forward,
// src/models.py:106-109, and the `lin` GEMM of GCNConv / GATConv, src/models.py:419,425).
//
// Operand maps of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md §3), lane l: r = l & 31, h = l >> 5:
//   A: A[row r][k = 8h + j], j = 0..7      B: B[k = 8h + j][col r]      D: reg q -> D[(q&3) + 8(q>>2) + 4h][col r]
// so both fragments are 16 contiguous bytes of a [row | col][k] bf16 image: one ds_read_b128 each.
#include "ln_row.h"
#include "mfma_io.h"
#include "x3.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#ifndef GCL_X3_ST_AUX
#define GCL_X3_ST_AUX 2  // cache-policy bits of the streamed-out stores: 2 = non-temporal (measured +1.1 % end to end: the outputs are
                         // consumed by a LATER kernel, keeping them out of the producer XCD's L2 leaves it to the inputs); 0 = default
#endif
#ifndef GCL_X3_LN_ST_AUX
#define GCL_X3_LN_ST_AUX 0  // the LayerNorm output of the chained MLP forward keeps the plain stores ln_fwd_kernel gives it: its
                           // reader is the NEXT kernel (the gather into the encoder's input, 19.3 -> 17.6 us a launch against 2)
#endif
// rows that this kernel reads exactly once: non-temporal loads (measured +0.7 % end to end; -DGCL_X3_LD_PLAIN: plain)
__device__ __forceinline__ float4 ld_stream(const float4* p) {
#ifndef GCL_X3_LD_PLAIN
  typedef float lv4f __attribute__((ext_vector_type(4)));
  const lv4f v = __builtin_nontemporal_load(reinterpret_cast<const lv4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}
using namespace gcl::mfma_io;  // f32x16, d_row, buffer stores, zero4 (mfma_io.h)
using namespace gcl::x3;  // pk_bf16, Pk3, split2, mfma_lo / _mid / _hi, bf16x8 (x3.h)

// LDS image of a [32 rows][64 k] bf16 piece: 144-byte rows (128 + 16): the 16 lanes one ds_read_b128 cycle
// serves ({0-3,12-15,20-27} ...) then sit on 16 distinct 4-bank groups.  Three piece images back to back.
constexpr int kRowB = 144;
constexpr int kImgB = 32 * kRowB;     // one piece
constexpr int kTileB = 3 * kImgB;     // hi | mid | lo of a 32-row tile (13.5 KiB)

__device__ unsigned long long x3_stamps[8 * 4096];  // diagnostic builds only (make STAMPS=1)
#ifdef GCL_STAMPS
#define X3_STAMP(slot)                                                           \
  do {                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                           \
    unsigned long long t_;                                                       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                           \
    stamp_acc[slot] += t_ - stamp_last;                                          \
    stamp_last = t_;                                                             \
  } while (0)
#else
#define X3_STAMP(slot) do {} while (0)
#endif

// ---------------------------------------------------------------------------------------------
// The tile body of the forward as functions: ONE text for linear_x3_fwd_kernel and for the chained kernel of a whole
// MLP (mlp_x3_chain_kernel), so a layer computes the same bits in either.
// ---------------------------------------------------------------------------------------------
struct X3Stamp {  // diagnostic builds only (X3_STAMP): unused, and so removed, in the product
  unsigned long long acc[8], last;
};

// what a lane knows about its place: its wave's LDS region, its fragment offset, its place in the staging map
// (16 lanes x float4 = one 64-float row, 4 rows per wave-instruction, 8 instructions per tile)
struct X3Lane {
  int tid, lane, wave, fo, rsub, csub;
  unsigned char* Aw;
};
__device__ __forceinline__ X3Lane x3_lane(unsigned char* smem8) {
  X3Lane l;
  l.tid = threadIdx.x;
  l.lane = l.tid & 63;
  l.wave = __builtin_amdgcn_readfirstlane(l.tid >> 6);
  l.Aw = smem8 + l.wave * kTileB;
  l.fo = (l.lane & 31) * kRowB + (l.lane >> 5) * 16;  // this lane's fragment inside a row-block, k-step 0
  l.rsub = l.lane >> 4;
  l.csub = l.lane & 15;
  return l;
}

// weight fragments: the block splits W once into piece images laid over the (still unused) tile regions, every wave
// then lifts its NS * NKS * 3 fragments into registers.  Two block barriers; the regions are free again afterwards.
template <int NS, int NKS>
__device__ __forceinline__ void x3_fwd_weights(unsigned char* smem8, const X3Lane& l, const float* __restrict__ W, int K,
                                               int N, bf16x8 (&wf)[NS][NKS][3]) {
  constexpr int kWimgB = NS * 32 * kRowB;  // one piece of the whole panel
  const int tid = l.tid;
  float2 wv[NS * 4];
#pragma unroll
  for (int i = 0; i < NS * 4; ++i) {  // NS*32 rows x 32 k-pairs over 256 threads, all loads in flight at once
    const int idx = i * 256 + tid;
    const int j = idx >> 5, k = (idx & 31) * 2;
    const bool okj = j < N;
    wv[i].x = (okj && k < K) ? W[(int64_t)j * K + k] : 0.f;
    wv[i].y = (okj && k + 1 < K) ? W[(int64_t)j * K + k + 1] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < NS * 4; ++i) {
    const int idx = i * 256 + tid;
    const int j = idx >> 5, k = (idx & 31) * 2;
    const Pk3 p = split2(wv[i].x, wv[i].y);
    unsigned char* d = smem8 + j * kRowB + k * 2;
    *reinterpret_cast<unsigned*>(d) = p.h;
    *reinterpret_cast<unsigned*>(d + kWimgB) = p.m;
    *reinterpret_cast<unsigned*>(d + 2 * kWimgB) = p.l;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int s = 0; s < NKS; ++s)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        wf[t][s][p] = *reinterpret_cast<const bf16x8*>(smem8 + p * kWimgB + t * 32 * kRowB + l.fo + s * 32);
  __syncthreads();  // the last block barrier of a layer's set-up: afterwards every wave only touches its own region
}

// bias of the four columns this lane stores (added after the transpose: one rounding on the finished sum)
template <int NS>
__device__ __forceinline__ float4 x3_fwd_bias(const float* __restrict__ bias, int lane, int N) {
  float4 bq;
  const int oc = (lane % (NS * 8)) * 4;
  bq.x = (bias && oc < N) ? bias[oc] : 0.f;
  bq.y = (bias && oc + 1 < N) ? bias[oc + 1] : 0.f;
  bq.z = (bias && oc + 2 < N) ? bias[oc + 2] : 0.f;
  bq.w = (bias && oc + 3 < N) ? bias[oc + 3] : 0.f;
  return bq;
}

// the loads of this wave's 32 rows of `tile`; rows past `rows_ld` and columns past K read the zero page
__device__ __forceinline__ void x3_fwd_issue(const X3Lane& l, const float* __restrict__ X, int64_t ldx, int64_t rows_ld,
                                             int K, int64_t tile, float4 (&pre)[8]) {
  const bool cok = l.csub * 4 < K;
  const int64_t r0 = tile * 128 + l.wave * 32;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int64_t row = r0 + it * 4 + l.rsub;
    const float4* p = (cok && row < rows_ld) ? reinterpret_cast<const float4*>(X + row * ldx + l.csub * 4) : zero4;
    pre[it] = ld_stream(p);
  }
}

// activation and 3-way split of the rows in `pre` into the wave's hi / mid / lo images
template <bool SILU>
__device__ __forceinline__ void x3_fwd_commit(const X3Lane& l, const float4 (&pre)[8], int K, float pa) {
  // K % 4 != 0: the 16 bytes of the last loading lane end in the row's padding (columns K.. of a 16-byte row), which
  // is not data: it is cleared before the split, whatever it holds (a NaN there would meet the zero weight and still
  // poison the row).  Block-uniform test: nothing changes for K % 4 == 0.
  const int kleft = K - l.csub * 4;  // data columns in this lane's float4
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    float4 v = pre[it];
    if (K & 3) {
      v.y = kleft > 1 ? v.y : 0.f; v.z = kleft > 2 ? v.z : 0.f; v.w = kleft > 3 ? v.w : 0.f;
    }
    if (SILU) {
      v.x = gcl::silu_f(v.x); v.y = gcl::silu_f(v.y); v.z = gcl::silu_f(v.z); v.w = gcl::silu_f(v.w);
    } else {  // PReLU and "none" (pa = 1) share one branch-free form
      const float mx = v.x * pa, my = v.y * pa, mz = v.z * pa, mw = v.w * pa;
      v.x = v.x > 0.f ? v.x : mx; v.y = v.y > 0.f ? v.y : my;
      v.z = v.z > 0.f ? v.z : mz; v.w = v.w > 0.f ? v.w : mw;
    }
    const Pk3 p01 = split2(v.x, v.y), p23 = split2(v.z, v.w);
    unsigned char* d = l.Aw + (it * 4 + l.rsub) * kRowB + l.csub * 8;
    *reinterpret_cast<u32x2*>(d) = u32x2{p01.h, p23.h};
    *reinterpret_cast<u32x2*>(d + kImgB) = u32x2{p01.m, p23.m};
    *reinterpret_cast<u32x2*>(d + 2 * kImgB) = u32x2{p01.l, p23.l};
  }
}

// the NS * NKS * 6 MFMAs of a tile, smallest piece products first.  The row fragments are re-read from LDS in every
// pass (6 * NKS ds_read_b128 per tile) rather than held
template <int NS, int NKS>
__device__ __forceinline__ void x3_fwd_mfma(const X3Lane& l, const bf16x8 (&wf)[NS][NKS][3], f32x16 (&acc)[NS]) {
  const unsigned char* Aw = l.Aw;
  const int fo = l.fo;
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const unsigned char* ap = Aw + fo + s * 32;
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap);
    const bf16x8 am = *reinterpret_cast<const bf16x8*>(ap + kImgB);
    const bf16x8 al = *reinterpret_cast<const bf16x8*>(ap + 2 * kImgB);
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = mfma_lo(acc[c], ah, am, al, wf[c][s][0], wf[c][s][1], wf[c][s][2]);
  }
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const unsigned char* ap = Aw + fo + s * 32;
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap);
    const bf16x8 am = *reinterpret_cast<const bf16x8*>(ap + kImgB);
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = mfma_mid(acc[c], ah, am, wf[c][s][0], wf[c][s][1]);
  }
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Aw + fo + s * 32);
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = mfma_hi(acc[c], ah, wf[c][s][0]);
  }
}

// rows a lane holds after the transpose: float4 number p is row p * RPP + lane / LPO, columns (lane % LPO) * 4 ..
template <int NS>
struct X3Out {
  static constexpr int OS = NS * 32, LPO = OS / 4, RPP = 64 / LPO, NP = 32 / RPP;
};

// transpose of the accumulators through the wave's region ([32][NS*32] fp32 <= 8 KiB of its 13.5), the bias, and the
// store of whole 16-byte row segments of this wave's rows of `tile`; `out` keeps what was stored.  For NS = 2 a lane
// then holds row p * 4 + (lane >> 4), columns (lane & 15) * 4 ..: the element x3_fwd_commit expects in pre[p], and the
// 16-lanes-per-row layout of ln_fwd_kernel<16>.
template <int NS>
__device__ __forceinline__ void x3_fwd_finish(const X3Lane& l, const f32x16 (&acc)[NS], float4 bq, float* __restrict__ Y,
                                              int64_t ldy, int64_t rows, int N, int64_t tile, bool drop,
                                              float4 (&out)[X3Out<NS>::NP]) {
  const int lane = l.lane;
  const int64_t r0 = tile * 128 + l.wave * 32;
  const int64_t nr64 = rows - r0;
  const int nr = nr64 < 0 ? 0 : (nr64 < 32 ? (int)nr64 : 32);
  constexpr int OS = X3Out<NS>::OS, LPO = X3Out<NS>::LPO, RPP = X3Out<NS>::RPP;
  float* Ot = reinterpret_cast<float*>(l.Aw);
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) Ot[d_row(r, lane) * OS + s * 32 + (lane & 31)] = acc[s][r];
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(Y + r0 * ldy, (nr > 0 && !drop) ? ((int64_t)(nr - 1) * ldy + N) * 4 : 0);
  const int orow = lane / LPO, ocol = (lane % LPO) * 4;
#pragma unroll
  for (int p = 0; p < 32 / RPP; ++p) {
    const int i = p * RPP + orow;
    float4 v = *reinterpret_cast<const float4*>(Ot + i * OS + ocol);
    v.x += bq.x; v.y += bq.y; v.z += bq.z; v.w += bq.w;
    buf_st4<GCL_X3_ST_AUX>(ry, (ocol < N) ? (unsigned)((i * ldy + ocol) * 4) : kOOB, v);
    out[p] = v;
  }
}

// One layer on one tile: commit `in`, (NEXT: issue the loads of `next_tile` into `in`), MFMA passes, transpose, bias,
// store; `out` = the biased rows.  abl: see linear_x3_fwd_kernel (0 in the product).
template <int NS, bool SILU, int NKS, bool NEXT>
__device__ __forceinline__ void x3_fwd_tile_layer(const X3Lane& l, X3Stamp& stamps, float4 (&in)[8],
                                                  const float* __restrict__ X, int64_t ldx, int64_t rows_ld,
                                                  int64_t next_tile, int K, float pa, const bf16x8 (&wf)[NS][NKS][3],
                                                  float4 bq, float* __restrict__ Y, int64_t ldy, int64_t rows, int N,
                                                  int64_t tile, int abl, float4 (&out)[X3Out<NS>::NP]) {
#ifdef GCL_STAMPS
  unsigned long long(&stamp_acc)[8] = stamps.acc;
  unsigned long long& stamp_last = stamps.last;
#endif
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // LDS operations of one wave complete in order
  X3_STAMP(0);
#ifdef GCL_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // split "waiting for the prefetched rows" from the commit work
#endif
  X3_STAMP(1);
  x3_fwd_commit<SILU>(l, in, K, pa);
  X3_STAMP(2);
  if (NEXT) x3_fwd_issue(l, X, ldx, rows_ld, K, next_tile, in);  // rows past the end read the zero page
  X3_STAMP(3);

  f32x16 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
  if (!(abl & 2)) x3_fwd_mfma<NS, NKS>(l, wf, acc);  // uniform
#ifdef GCL_STAMPS
  asm volatile("" ::"v"(acc[0][0]));
#endif
  X3_STAMP(4);
  x3_fwd_finish<NS>(l, acc, bq, Y, ldy, rows, N, tile, (abl & 1) != 0, out);
  X3_STAMP(5);
}

// ---------------------------------------------------------------------------------------------
// Forward:  Y[r, j] = sum_k act(X[r, k]) W[j, k] + bias[j].   4 waves per block, each wave owns 32 rows of the
// block's 128-row tile and ITS OWN LDS region: no block barrier after the set-up.  The weight fragments of
// all six piece combinations live in registers for the whole launch (NS * 4 * 3 fragments).  Per tile a wave
// (1) splits the rows it prefetched into its hi/mid/lo images, (2) issues the loads of its next tile,
// (3) runs NS * nks * 6 MFMAs on fragments read with ds_read_b128, (4) transposes the accumulators through
// the same LDS region and stores whole 16-byte row segments.
// ---------------------------------------------------------------------------------------------
template <int NS, bool SILU, int NKS>  // NKS: k-steps of 16 (2 for K <= 32, else 4)
__global__ __launch_bounds__(256, 2) void linear_x3_fwd_kernel(const float* __restrict__ X, int64_t ldx,
                                                               const float* __restrict__ slope_p, int32_t akind,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ bias, float* __restrict__ Y,
                                                               int64_t ldy, int64_t rows, int32_t K, int32_t N,
                                                               int32_t abl) {
  // abl: timing-only ablation bits of tools/ablate.sh (0 in the product): 1 = stores dropped (empty window),
  // 2 = no MFMA passes, 4 = loads read the zero page.  Runtime values: the code is the same.
  extern __shared__ __align__(16) unsigned char smem8[];
#ifdef GCL_STAMPS
  const unsigned long long stamp_t0 = __builtin_amdgcn_s_memtime();
#endif
  const X3Lane l = x3_lane(smem8);
  const int64_t rows_ld = (abl & 4) ? 0 : rows;
  bf16x8 wf[NS][NKS][3];
  x3_fwd_weights<NS, NKS>(smem8, l, W, K, N, wf);
  const float pa = (akind == gcl::kActPrelu) ? *slope_p : 1.f;  // x > 0 ? x : x * pa ("none": pa = 1, exact)
  const float4 bq = x3_fwd_bias<NS>(bias, l.lane, N);

  const int64_t ntiles = (rows + 127) / 128;
  float4 pre[8];
  x3_fwd_issue(l, X, ldx, rows_ld, K, blockIdx.x, pre);
  X3Stamp stamps;
#ifdef GCL_STAMPS
  unsigned long long(&stamp_acc)[8] = stamps.acc;
  unsigned long long& stamp_last = stamps.last;
  for (int i = 0; i < 8; ++i) stamp_acc[i] = 0;
  stamp_last = __builtin_amdgcn_s_memtime();
  stamp_acc[6] = stamp_last - stamp_t0;  // set-up (weight fragments)
  stamp_acc[7] = stamp_t0;               // absolute start: are all blocks resident at once?
#endif
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float4 out[X3Out<NS>::NP];
    x3_fwd_tile_layer<NS, SILU, NKS, true>(l, stamps, pre, X, ldx, rows_ld, t + gridDim.x, K, pa, wf, bq, Y, ldy, rows, N,
                                           t, abl, out);
  }
#ifdef GCL_STAMPS
  if (l.lane == 0 && blockIdx.x < 1024)
    for (int i = 0; i < 8; ++i) x3_stamps[(blockIdx.x * 4 + l.wave) * 8 + i] = stamp_acc[i];
#endif
}

// ---------------------------------------------------------------------------------------------
// A run of L = 2 or 3 Linear layers of an MLP in one launch: y_k = act_k(y_{k-1}) W_k^T + b_k, every y_k stored for the
// backward, each layer the text of linear_x3_fwd_kernel<2, false, 4> (all widths 33..64).  A wave keeps the biased
// float4s of its 32 rows after a layer's store and commits them as the next layer's input: the rows never come back
// from memory, and since a wave only touches its own LDS region there is no barrier between layers either.  Only layer 0
// loads from global memory, one tile ahead.
// Every layer's 24 weight fragments stay in registers (96 VGPRs a layer): one 4-wave block per CU, one wave per SIMD
// with the whole 512-register file.  (Two waves per SIMD would have to keep the layers' piece images in LDS and re-read
// the fragments per tile: 27 KiB a layer next to 8 x 13.5 KiB of tile regions is more than the 160 KiB of a CU for two
// layers already.)
// LN: the run ends at the MLP's last Linear and a node LayerNorm follows: the 16 lanes that hold a row apply the row
// arithmetic of ln_fwd_kernel<16, true> (ln_row.h) to it and store y and (mean, rstd) besides the pre-norm row.
// ---------------------------------------------------------------------------------------------
struct X3Chain {
  const float* W[3];
  const float* bias[3];
  const float* slope[3];  // PReLU slope in front of layer k, or null: no activation
  float* Z[3];            // pre-activation output of layer k [rows, N[k]], row stride ldz[k]
  int64_t ldz[3];
  int32_t K[3], N[3];
  const float* gamma;  // LN only
  const float* beta;
  float* Y;  // [rows, N[L-1]], row stride ldy
  int64_t ldy;
  float* stats;  // [rows][2]
  float eps;
};

template <int L, bool LN>
__global__ __launch_bounds__(256, 1) void mlp_x3_chain_kernel(const float* __restrict__ X, int64_t ldx, int64_t rows,
                                                             const X3Chain a) {
  extern __shared__ __align__(16) unsigned char smem8[];
  const X3Lane l = x3_lane(smem8);
  bf16x8 wf[L][2][4][3];
  float pa[L];
  float4 bq[L];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    x3_fwd_weights<2, 4>(smem8, l, a.W[k], a.K[k], a.N[k], wf[k]);
    pa[k] = a.slope[k] ? *a.slope[k] : 1.f;
    bq[k] = x3_fwd_bias<2>(a.bias[k], l.lane, a.N[k]);
  }
  // LayerNorm: this lane's four columns of gamma and beta (F % 4 == 0)
  const int c0 = l.csub * 4, F = a.N[L - 1];
  const bool cin = c0 < F;
  float g0 = 0, g1 = 0, g2 = 0, g3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  if (LN && cin) {
    g0 = a.gamma[c0]; g1 = a.gamma[c0 + 1]; g2 = a.gamma[c0 + 2]; g3 = a.gamma[c0 + 3];
    b0 = a.beta[c0]; b1 = a.beta[c0 + 1]; b2 = a.beta[c0 + 2]; b3 = a.beta[c0 + 3];
  }
  const float invF = 1.f / (float)F;
  const int64_t ntiles = (rows + 127) / 128;
  float4 pre[8];
  x3_fwd_issue(l, X, ldx, rows, a.K[0], blockIdx.x, pre);
  X3Stamp stamps;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float4 cur[8];
    x3_fwd_tile_layer<2, false, 4, true>(l, stamps, pre, X, ldx, rows, t + gridDim.x, a.K[0], pa[0], wf[0], bq[0], a.Z[0],
                                         a.ldz[0], rows, a.N[0], t, 0, cur);
#pragma unroll
    for (int k = 1; k < L; ++k) {
      // the columns K.. of a row are zeros where the layer loads them (zero page): the same here, whatever the
      // accumulators of the unused columns hold (NaN x 0 for a row with a NaN in it)
      const bool cok = l.csub * 4 < a.K[k];
#pragma unroll
      for (int p = 0; p < 8; ++p) cur[p] = cok ? cur[p] : make_float4(0.f, 0.f, 0.f, 0.f);
      x3_fwd_tile_layer<2, false, 4, false>(l, stamps, cur, nullptr, 0, 0, 0, a.K[k], pa[k], wf[k], bq[k], a.Z[k],
                                            a.ldz[k], rows, a.N[k], t, 0, cur);
    }
    if (LN) {
      const int64_t r0 = t * 128 + l.wave * 32;
      const int64_t nr64 = rows - r0;
      const int nr = nr64 < 0 ? 0 : (nr64 < 32 ? (int)nr64 : 32);
      const __amdgpu_buffer_rsrc_t ry = make_rsrc(a.Y + r0 * a.ldy, nr > 0 ? ((int64_t)(nr - 1) * a.ldy + F) * 4 : 0);
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.stats + r0 * 2, (int64_t)nr * 8);
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int i = p * 4 + l.rsub;
        float mean, rstd;
        float4 y;  // the columns past F are zeros where ln_fwd_kernel does not load them
        gcl::ln::fwd_row<16>(cin ? cur[p].x : 0.f, cin ? cur[p].y : 0.f, cin ? cur[p].z : 0.f, cin ? cur[p].w : 0.f, c0, F,
                             invF, a.eps, g0, g1, g2, g3, b0, b1, b2, b3, mean, rstd, y.x, y.y, y.z, y.w);
        buf_st4<GCL_X3_LN_ST_AUX>(ry, cin ? (unsigned)((i * a.ldy + c0) * 4) : kOOB, y);
        buf_st2<0>(rs, l.csub == 0 ? (unsigned)(i * 8) : kOOB, make_float2(mean, rstd));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Fused backward of  y = act(P) W^T + b  for Fin in 33..64 (FiP = 64) and Fout <= 64, 64-row tiles, 4 waves:
//   dX = (dY W) * act'(P)      dW += dY^T act(P)      db += colsum(dY)      colsum_dx += colsum(dX)
//   d_slope += sum(dY W * P, P <= 0)
// Every thread splits the 4 + 4 float4 of dY and act(P) it loaded (coalesced, 16 lanes per row) into the two
// hi/mid/lo LDS images [64 rows][64 columns] of the tile.  Wave (rg, sg) then computes the dX block rows 32rg..,
// columns 32sg.. (A fragments = ds_read_b128 rows of the dY image, B = W^T fragments held in registers) and
// the dW block (so, sc) whose operands sum over the tile's ROWS: both are read from the same images with
// ds_read_b64_tr_b16 (the hardware transposing read: a 4-row x 16-column block per 16 lanes, delivered
// column-major), so no transposed copy of either tile exists.  dX goes through a fp32 staging tile and is
// finished (act', slope and column sums) by the thread that still holds the matching float4 of P, then stored
// as whole 16-byte row segments.  Two block barriers per tile.
// Partial-record layout and outputs are those of linear_bwd_fused64_kernel (linear.hip).
// ---------------------------------------------------------------------------------------------
// Backward images: [64 rows][64 bf16] with UNPADDED 128-byte rows and the eight 16-byte chunks of row r stored at
// chunk ^ swz(r), swz(r) = (bit1(r) << 2) | (bit3(r) << 1) | bit2(r).  One image serves both kinds of read without
// bank conflicts: the 16 rows one ds_read_b128 cycle serves ({0-3,12-15,20-27}, ...) differ in their low four bits, so
// (r & 1, swz(r)) - which 4-bank group of which half of the 64 banks - is distinct for all of them; and of the four
// rows x four chunks one half-wave of ds_read_b64_tr_b16 takes, rows 0/2 (same parity) land on chunk sets that differ
// in bit 2.  (With 144-byte padded rows a quarter of this kernel's LDS cycles were 2-way conflicts of the
// transposing reads: profiles/r02_pmc_linear_x3.txt.)
constexpr int kBRowB = 128;
constexpr int kImg64B = 64 * kBRowB;  // one piece of a 64-row tile
__device__ __forceinline__ int swz(int r) { return (((r >> 1) & 1) << 2) | (((r >> 3) & 1) << 1) | ((r >> 2) & 1); }
// byte offset of byte `b` (< 128) of row `r`
__device__ __forceinline__ int sw_off(int r, int b) { return r * kBRowB + ((((b >> 4) ^ swz(r)) << 4) | (b & 15)); }

typedef short s16x4 __attribute__((ext_vector_type(4)));
// rows rb..rb+3 (offset o0) and rb+4..rb+7 (offset o1: the swizzle differs) of 16 columns, delivered column-major
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* base, int o0, int o1) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o0));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + o1));
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// One body for the two kernels below (as agg_heavy_row in aggregate.hip).  A flag that is off removes the code of what the
// caller did not ask for instead of testing a pointer where the result would be stored:
//   ACT   - an input activation (in_slope may be given): act(P), act', the slope gradient and the copy of P kept for them;
//           off: a = P, dX = dY W
//   DB    - the running column sums of dY (part_db)          CS - the running column sums of dX (part_cs)
//   YMASK - the element masks of dY's last partial float4 (needed when Fout % 4 != 0)
// With all four on this is the text of linear_x3_bwd_kernel as it was, run-time tests included.
template <int NO, bool ACT, bool DB, bool CS, bool YMASK>
__device__ __forceinline__ void linear_x3_bwd_body(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ W, const float* __restrict__ P,
    int64_t ldp, const float* __restrict__ in_slope, float* __restrict__ dX, int64_t lddx, int64_t rows, int32_t Fin,
    int32_t Fout, float* __restrict__ part_dw, float* __restrict__ part_db, float* __restrict__ part_cs,
    double* __restrict__ part_slope) {
  constexpr int FoP = NO * 32, FiP = 64, NKO = NO * 2, NT = NO * 2;
  extern __shared__ __align__(16) unsigned char smem8[];
  unsigned char* Yimg = smem8;                 // [3][64][128 B]  dY pieces (swizzled chunks)
  unsigned char* Pimg = smem8 + 3 * kImg64B;   // [3][64][128 B]  act(P) pieces
  float* Stg = reinterpret_cast<float*>(smem8 + 6 * kImg64B);  // [64][64] fp32: dX before act'
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int rg = wave & 1, sg = wave >> 1;
  const int so = wave % NO, sc = wave / NO;
  const bool has_tile = wave < NT;

  // ---- W^T fragments of this wave's dX column slab: B[k = o][n = c] = W[o][c], image rows = c ----
  bf16x8 wtf[NKO][3];
  {
    float2 wv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // 64 columns x 32 o-pairs over 256 threads
      const int idx = i * 256 + tid;
      const int c = idx & 63, o = (idx >> 6) * 2;
      wv[i].x = (c < Fin && o < Fout) ? W[(int64_t)o * Fin + c] : 0.f;
      wv[i].y = (c < Fin && o + 1 < Fout) ? W[(int64_t)(o + 1) * Fin + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = i * 256 + tid;
      const int c = idx & 63, o = (idx >> 6) * 2;
      const Pk3 p = split2(wv[i].x, wv[i].y);
      unsigned char* d = Yimg + sw_off(c, o * 2);
      *reinterpret_cast<unsigned*>(d) = p.h;
      *reinterpret_cast<unsigned*>(d + kImg64B) = p.m;
      *reinterpret_cast<unsigned*>(d + 2 * kImg64B) = p.l;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NKO; ++s)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        wtf[s][p] = *reinterpret_cast<const bf16x8*>(Yimg + p * kImg64B + sw_off(32 * sg + li, (16 * s + 8 * h) * 2));
    __syncthreads();
  }

  const bool act = ACT && in_slope != nullptr;
  const float slope = act ? *in_slope : 1.f;
  const int64_t ntiles = (rows + 63) / 64;

  // staging map: 16 lanes x float4 = one 64-float row; 4 rows per wave-instruction; a wave stages 16 rows
  const int rsub = lane >> 4, csub = lane & 15;
  const bool yok = csub * 4 < Fout, pok = csub * 4 < Fin;
  // element masks of the last partial float4 (Fout % 4 != 0: the padding columns of dY hold finite junk)
  const unsigned ym0 = csub * 4 < Fout ? ~0u : 0u, ym1 = csub * 4 + 1 < Fout ? ~0u : 0u, ym2 = csub * 4 + 2 < Fout ? ~0u : 0u,
                 ym3 = csub * 4 + 3 < Fout ? ~0u : 0u;
  float4 pre_y[4], pre_p[4];
  auto issue = [&](int64_t tile) {
    const int64_t r0 = tile * 64 + wave * 16;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t row = r0 + it * 4 + rsub;
      const bool rok = row < rows;
      pre_y[it] = ld_stream((yok && rok) ? reinterpret_cast<const float4*>(dY + row * lddy + csub * 4) : zero4);
      pre_p[it] = ld_stream((pok && rok) ? reinterpret_cast<const float4*>(P + row * ldp + csub * 4) : zero4);
    }
  };

  // lane parts of the fragment addresses
  // lane parts of the fragment addresses.  Row fragment (ds_read_b128) of k-step s: row 32 rg + li, chunk 2 s + h.
  int fo[NKO];
#pragma unroll
  for (int s = 0; s < NKO; ++s) fo[s] = sw_off(rg * 32 + li, (2 * s + h) * 16);
  // Transposing read of k-step s, half j: lane 4q + pp of 16-lane group g supplies row 16 s + 8 (g >> 1) + 4 j + q,
  // bytes 64 slab + 32 (g & 1) + 8 pp .. +7; bits 4.. of the row do not enter the swizzle, so the k-step is an offset
  const int g = lane >> 4, i16 = lane & 15;
  int troY[2], troP[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 8 * (g >> 1) + 4 * j + (i16 >> 2), b = 32 * (g & 1) + 8 * (i16 & 3);
    troY[j] = sw_off(r, 64 * so + b);
    troP[j] = sw_off(r, 64 * sc + b);
  }

  f32x16 dw_hi, dw_lo;  // running dW block: the hi x hi products and the five correction products apart
#pragma unroll
  for (int r = 0; r < 16; ++r) dw_hi[r] = 0.f, dw_lo[r] = 0.f;
  float4 db4 = make_float4(0.f, 0.f, 0.f, 0.f), cs4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double slope_acc = 0.0;
  float4 cur_p[4];

  issue(blockIdx.x);
#ifdef GCL_STAMPS
  unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_last = __builtin_amdgcn_s_memtime();
#endif
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
#ifdef GCL_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    X3_STAMP(0);
    // ---- split this thread's rows into the images ----
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      float4 y = pre_y[it];
      if (YMASK) {
        y.x = __uint_as_float(__float_as_uint(y.x) & ym0); y.y = __uint_as_float(__float_as_uint(y.y) & ym1);
        y.z = __uint_as_float(__float_as_uint(y.z) & ym2); y.w = __uint_as_float(__float_as_uint(y.w) & ym3);
      }
      if (DB) { db4.x += y.x; db4.y += y.y; db4.z += y.z; db4.w += y.w; }
      const float4 z = pre_p[it];
      float4 a = z;
      if (ACT) {
        cur_p[it] = z;
        const float mx = z.x * slope, my = z.y * slope, mz = z.z * slope, mw = z.w * slope;
        a.x = z.x > 0.f ? z.x : mx; a.y = z.y > 0.f ? z.y : my; a.z = z.z > 0.f ? z.z : mz; a.w = z.w > 0.f ? z.w : mw;
      }
      const Pk3 y01 = split2(y.x, y.y), y23 = split2(y.z, y.w), a01 = split2(a.x, a.y), a23 = split2(a.z, a.w);
      const int off = sw_off(wave * 16 + it * 4 + rsub, csub * 8);
      *reinterpret_cast<u32x2*>(Yimg + off) = u32x2{y01.h, y23.h};
      *reinterpret_cast<u32x2*>(Yimg + off + kImg64B) = u32x2{y01.m, y23.m};
      *reinterpret_cast<u32x2*>(Yimg + off + 2 * kImg64B) = u32x2{y01.l, y23.l};
      *reinterpret_cast<u32x2*>(Pimg + off) = u32x2{a01.h, a23.h};
      *reinterpret_cast<u32x2*>(Pimg + off + kImg64B) = u32x2{a01.m, a23.m};
      *reinterpret_cast<u32x2*>(Pimg + off + 2 * kImg64B) = u32x2{a01.l, a23.l};
    }
    X3_STAMP(1);
    __syncthreads();
    X3_STAMP(2);
    issue(t + gridDim.x);
    X3_STAMP(3);

    // ---- dX block (rows 32rg.., columns 32sg..), smallest piece products first ----
    {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int s = 0; s < NKO; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Yimg + fo[s]);
        const bf16x8 am = *reinterpret_cast<const bf16x8*>(Yimg + fo[s] + kImg64B);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(Yimg + fo[s] + 2 * kImg64B);
        acc = mfma_lo(acc, ah, am, al, wtf[s][0], wtf[s][1], wtf[s][2]);
      }
#pragma unroll
      for (int s = 0; s < NKO; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Yimg + fo[s]);
        const bf16x8 am = *reinterpret_cast<const bf16x8*>(Yimg + fo[s] + kImg64B);
        acc = mfma_mid(acc, ah, am, wtf[s][0], wtf[s][1]);
      }
#pragma unroll
      for (int s = 0; s < NKO; ++s) acc = mfma_hi(acc, *reinterpret_cast<const bf16x8*>(Yimg + fo[s]), wtf[s][0]);
#pragma unroll
      for (int r = 0; r < 16; ++r) Stg[(rg * 32 + d_row(r, lane)) * 64 + sg * 32 + li] = acc[r];
    }

    X3_STAMP(4);
    // ---- dW block (so, sc) over the 64 rows of the tile: both operands by transposing reads ----
    if (has_tile) {  // wave-uniform
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const unsigned char* ya = Yimg + s * 16 * kBRowB;
        const unsigned char* pa = Pimg + s * 16 * kBRowB;
        const bf16x8 ah = tr_frag(ya, troY[0], troY[1]), am = tr_frag(ya + kImg64B, troY[0], troY[1]),
                     al = tr_frag(ya + 2 * kImg64B, troY[0], troY[1]);
        const bf16x8 bh = tr_frag(pa, troP[0], troP[1]), bm = tr_frag(pa + kImg64B, troP[0], troP[1]),
                     bl = tr_frag(pa + 2 * kImg64B, troP[0], troP[1]);
        dw_lo = mfma_lo(dw_lo, ah, am, al, bh, bm, bl);
        dw_lo = mfma_mid(dw_lo, ah, am, bh, bm);
        dw_hi = mfma_hi(dw_hi, ah, bh);
      }
    }
#ifdef GCL_STAMPS
    asm volatile("" ::"v"(dw_hi[0]), "v"(dw_lo[0]));
#endif
    X3_STAMP(5);
    __syncthreads();
    X3_STAMP(6);

    // ---- finish dX: the thread that loaded P[row, 4 columns] owns that float4 of the result ----
    {
      const int64_t r0 = t * 64;
      const int64_t nr = (rows - r0) < 64 ? (rows - r0) : 64;
      const __amdgpu_buffer_rsrc_t rx = make_rsrc(dX + r0 * lddx, nr > 0 ? ((nr - 1) * lddx + Fin) * 4 : 0);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = wave * 16 + it * 4 + rsub;
        float4 v = *reinterpret_cast<const float4*>(Stg + row * 64 + csub * 4);
        if (ACT) {
          const float4 z = cur_p[it];
          const bool nx = act && !(z.x > 0.f), ny = act && !(z.y > 0.f), nz = act && !(z.z > 0.f), nw = act && !(z.w > 0.f);
          // fp64 across float4s: the slope gradient is a long signed sum with heavy cancellation
          slope_acc += (double)(((nx ? v.x * z.x : 0.f) + (ny ? v.y * z.y : 0.f)) + ((nz ? v.z * z.z : 0.f) + (nw ? v.w * z.w : 0.f)));
          v.x = nx ? v.x * slope : v.x; v.y = ny ? v.y * slope : v.y; v.z = nz ? v.z * slope : v.z; v.w = nw ? v.w * slope : v.w;
        }
        if (CS) { cs4.x += v.x; cs4.y += v.y; cs4.z += v.z; cs4.w += v.w; }
        buf_st4<GCL_X3_ST_AUX>(rx, pok ? (unsigned)((row * lddx + csub * 4) * 4) : kOOB, v);
      }
    }
    X3_STAMP(7);
  }
#ifdef GCL_STAMPS
  if (lane == 0 && blockIdx.x < 1024)
    for (int i = 0; i < 8; ++i) x3_stamps[(blockIdx.x * 4 + wave) * 8 + i] = stamp_acc[i];
#endif

  // ---- per-block partials ----
  constexpr size_t REC = (size_t)FoP * FiP + FoP + FiP;
  float* out = part_dw + (size_t)blockIdx.x * REC;
  if (has_tile) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)(so * 32 + d_row(r, lane)) * FiP + sc * 32 + li] = dw_hi[r] + dw_lo[r];
  }
  if (!(ACT || DB || CS)) return;  // the dW block is all this launch was asked for besides dX
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem8);  // [2][16][64]: db and colsum partials of the 16 row groups
  {
    float* rdb = red + (wave * 4 + rsub) * 64 + csub * 4;
    if (DB) *reinterpret_cast<float4*>(rdb) = db4;
    if (CS) *reinterpret_cast<float4*>(rdb + 16 * 64) = cs4;
  }
  double* dred = reinterpret_cast<double*>(red + 2 * 16 * 64);
  if (ACT) {
    for (int off = 32; off > 0; off >>= 1) slope_acc += __shfl_down(slope_acc, off, 64);
    if (lane == 0) dred[wave] = slope_acc;
  }
  __syncthreads();
  if (tid < 128) {
    const int which = tid >> 6, c = tid & 63;  // (wave-uniform)
    if (which == 0 ? DB : CS) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += red[(which * 16 + q) * 64 + c];
      if (which == 0) {
        if (part_db && c < FoP) part_db[(size_t)blockIdx.x * REC + c] = s;
      } else {
        if (part_cs) part_cs[(size_t)blockIdx.x * REC + c] = s;
      }
    }
  }
  if (ACT && part_slope && tid == 0) part_slope[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}

// The call that wants both column sums (db and those of dX; with an activation that is everything) and, with
// GCL_X3_BWD_LEAN=0, every call: all of the body, each request tested at run time.
template <int NO>
__global__ __launch_bounds__(256, 2) void linear_x3_bwd_kernel(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ W, const float* __restrict__ P,
    int64_t ldp, const float* __restrict__ in_slope, float* __restrict__ dX, int64_t lddx, int64_t rows, int32_t Fin,
    int32_t Fout, float* __restrict__ part_dw, float* __restrict__ part_db, float* __restrict__ part_cs,
    double* __restrict__ part_slope) {
  linear_x3_bwd_body<NO, true, true, true, true>(dY, lddy, W, P, ldp, in_slope, dX, lddx, rows, Fin, Fout, part_dw, part_db,
                                                 part_cs, part_slope);
}

// Every other combination of requests: the body without the code of what was not asked for (same grid, LDS and records).
template <int NO, bool ACT, bool DB, bool CS, bool YMASK>
__global__ __launch_bounds__(256, 2) void linear_x3_bwd_lean_kernel(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ W, const float* __restrict__ P,
    int64_t ldp, const float* __restrict__ in_slope, float* __restrict__ dX, int64_t lddx, int64_t rows, int32_t Fin,
    int32_t Fout, float* __restrict__ part_dw, float* __restrict__ part_db, float* __restrict__ part_cs,
    double* __restrict__ part_slope) {
  linear_x3_bwd_body<NO, ACT, DB, CS, YMASK>(dY, lddy, W, P, ldp, in_slope, dX, lddx, rows, Fin, Fout, part_dw, part_db,
                                             part_cs, part_slope);
}

int x3_ablate() {  // GCL_ABLATE: timing-only experiments (tools/ablate.sh) - honoured by the diagnostic build only
#ifndef GCL_STAMPS
  return 0;
#endif
  static const int v = gcl::env_int("GCL_ABLATE", 0);
  return v;
}

}  // namespace

#ifdef GCL_STAMPS
// diagnostic builds only: per-wave cycle sums [wave][8] = {loop top, wait loads, commit, issue, mfma, store, ..}
extern "C" int gcl_debug_read_stamps_x3(unsigned long long* host_out, int count) {
  GCL_CHECK_HIP(hipDeviceSynchronize());
  GCL_CHECK_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(x3_stamps), sizeof(unsigned long long) * count));
  return GCL_OK;
}
#endif

namespace gcl {

using namespace plan;
static_assert(kX3FwdLds == 4 * (size_t)kTileB && kX3BwdLds == 6 * (size_t)kImg64B + 64 * 64 * sizeof(float),
              "dense_plan.h states the LDS of these kernels");

// this translation unit's reader of the switches (dense_plan.h): the cached one here, the per-call ones on first use
static DenseSwitches switches() {
  static const bool valu = env_is("GCL_LINEAR_IMPL", "valu");
  DenseSwitches sw;
  sw.valu = valu;
  return sw;
}

int x3_linear_fwd(const X3FwdPlan& p, const float* x, int64_t ldx, int akind, const float* slope, const float* W,
                  const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N, hipStream_t st) {
  if (rows == 0) return GCL_OK;
  const int rc = pick<1, 2>(p.NS, [&](auto NS) {
    return pick<0, 1>(p.SILU, [&](auto SILU) {
      return pick<2, 4>(p.NKS, [&](auto NKS) {
        hipLaunchKernelGGL((linear_x3_fwd_kernel<decltype(NS)::value, decltype(SILU)::value != 0, decltype(NKS)::value>),
                           dim3(p.grid), dim3(256), p.lds, st, x, ldx, slope, akind, W, bias, y, ldy, rows, K, N, x3_ablate());
        return (int)GCL_OK;
      });
    });
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

// ---- the chained forward of an MLP (mlp_x3_chain_kernel) ----
static int x3_chain_launch(const ChainPlan& p, const float* x, int64_t ldx, int64_t rows, const X3Chain& a, hipStream_t st) {
  if (rows == 0) return GCL_OK;
  const int rc = pick<0, 1, 2>(p.L == 3 ? 2 : p.LN, [&](auto V) {  // <L, LN>: (2, false) (2, true) (3, false)
    auto kern = mlp_x3_chain_kernel<decltype(V)::value == 2 ? 3 : 2, decltype(V)::value == 1>;
    GCL_ENSURE_DYN_LDS(kern, p.lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, st, x, ldx, rows, a);
    return (int)GCL_OK;
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int x3_linear_bwd(const BwdAllPlan& p, const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                  const float* in_slope, float* dx, int64_t lddx, int64_t rows, int Fin, int Fout, float* part_dw,
                  float* part_db, float* part_cs, double* part_slope, hipStream_t st) {
  auto go = [&](auto kern) {
    GCL_ENSURE_DYN_LDS(kern, gcl::kLdsBytes);
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(256), p.lds, st, dy, lddy, W, x, ldx, in_slope, dx, lddx, rows, Fin, Fout,
                       part_dw, part_db, part_cs, part_slope);
    return (int)GCL_OK;
  };
  // kX3Lean: <NO, ACT, DB, CS, YMASK> with at most one of DB / CS (both: the full kernel), as one code
  const int want = p.DB ? 1 : p.CS ? 2 : 0;
  const int rc = p.form == BwdAllForm::kX3Full
                     ? pick<1, 2>(p.NO, [&](auto NO) { return go(linear_x3_bwd_kernel<decltype(NO)::value>); })
                     : pick<1, 2>(p.NO, [&](auto NO) {
                         return pick<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11>(want * 4 + p.ACT * 2 + p.YMASK, [&](auto C) {
                           constexpr int c = decltype(C)::value;
                           return go(linear_x3_bwd_lean_kernel<decltype(NO)::value, (c & 2) != 0, c / 4 == 1, c / 4 == 2, (c & 1) != 0>);
                         });
                       });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // namespace gcl

static gcl::plan::ChainCall chain_call(const float* x, int64_t ldx, int64_t rows, int32_t K, int32_t act0, int32_t nlayers,
                                       const float* z0, int64_t ldz0, int32_t N0, const float* z1, int64_t ldz1, int32_t N1,
                                       const float* z2, int64_t ldz2, int32_t N2, const float* gamma, const float* y,
                                       int64_t ldy, const float* stats) {
  using gcl::aligned16;
  return {ldx, rows, K, act0, nlayers, x != nullptr, aligned16(x),
          {z0 != nullptr, z1 != nullptr, z2 != nullptr}, {aligned16(z0), aligned16(z1), aligned16(z2)},
          {ldz0, ldz1, ldz2}, {N0, N1, N2},
          gamma != nullptr, y != nullptr, aligned16(y), stats != nullptr, ((uintptr_t)stats & 7) == 0, ldy};
}

extern "C" int gcl_mlp_fwd_chain_ok(const float* x, int64_t ldx, int64_t rows, int32_t K, int32_t act0, int32_t nlayers,
                                    const float* z0, int64_t ldz0, int32_t N0, const float* z1, int64_t ldz1, int32_t N1,
                                    const float* z2, int64_t ldz2, int32_t N2, const float* gamma, const float* y,
                                    int64_t ldy, const float* stats) {
  return gcl::plan_mlp_chain(chain_call(x, ldx, rows, K, act0, nlayers, z0, ldz0, N0, z1, ldz1, N1, z2, ldz2, N2, gamma, y, ldy,
                                        stats), gcl::switches()).ok
             ? 1
             : 0;
}

extern "C" int gcl_mlp_fwd_chain(const float* x, int64_t ldx, int64_t rows, int32_t K, int32_t act0, const float* slope0,
                                 int32_t nlayers, const float* W0, const float* b0, float* z0, int64_t ldz0, int32_t N0,
                                 const float* W1, const float* b1, const float* slope1, float* z1, int64_t ldz1, int32_t N1,
                                 const float* W2, const float* b2, const float* slope2, float* z2, int64_t ldz2, int32_t N2,
                                 const float* gamma, const float* beta, float eps, float* y, int64_t ldy, float* stats,
                                 gcl_stream_t stream) {
  GCL_CHECK_ARG(x && W0 && z0 && W1 && z1 && (nlayers == 2 || (W2 && z2)), "mlp_fwd_chain: null argument");
  GCL_CHECK_ARG(!gamma || (beta && y && stats), "mlp_fwd_chain: the LayerNorm needs beta, y and stats");
  GCL_CHECK_ARG(act0 != GCL_ACT_PRELU || slope0, "mlp_fwd_chain: GCL_ACT_PRELU needs the slope pointer");
  const gcl::plan::ChainPlan p = gcl::plan_mlp_chain(
      chain_call(x, ldx, rows, K, act0, nlayers, z0, ldz0, N0, z1, ldz1, N1, z2, ldz2, N2, gamma, y, ldy, stats), gcl::switches());
  GCL_CHECK_ARG(p.ok, "mlp_fwd_chain: not a run this kernel takes (gcl_mlp_fwd_chain_ok): launch it per layer");
  X3Chain a = {};
  const float* Ws[3] = {W0, W1, W2};
  const float* bs[3] = {b0, b1, b2};
  const float* sl[3] = {act0 == GCL_ACT_PRELU ? slope0 : nullptr, slope1, slope2};
  float* zs[3] = {z0, z1, z2};
  const int64_t ldz[3] = {ldz0, ldz1, ldz2};
  const int32_t Ns[3] = {N0, N1, N2};
  int32_t Kk = K;
  for (int k = 0; k < nlayers; ++k) {
    a.W[k] = Ws[k]; a.bias[k] = bs[k]; a.slope[k] = sl[k]; a.Z[k] = zs[k]; a.ldz[k] = ldz[k];
    a.K[k] = Kk; a.N[k] = Ns[k];
    Kk = Ns[k];
  }
  a.gamma = gamma; a.beta = beta; a.Y = y; a.ldy = ldy; a.stats = stats; a.eps = eps;
  return gcl::x3_chain_launch(p, x, ldx, rows, a, (hipStream_t)stream);
}
