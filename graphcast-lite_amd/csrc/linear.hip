// Dense per-node transforms  y = act(x) W^T + b  and their gradients.
//
// Replaces nn.Linear (+ preceding nn.PReLU) of MLP.forward (src/models.py:106-109) and the `lin`
// GEMM inside GCNConv / GATConv (src/models.py:419,425).  These are tall-skinny contractions
// (rows = B*n up to ~1.4M, K,N <= 128): at fp32 they sit at 16-32 flop/B, i.e. at or above the
// HBM ridge, so they run on the matrix cores with the EXACT-fp32 instruction
// v_mfma_f32_32x32x2_f32 (an fp32 FMA chain in k order; same peak as the fp32 VALU but one operand
// register per lane and no VALU pressure).  A plain VALU implementation of the same contract is
// kept (GCL_LINEAR_IMPL=valu) as an in-library cross-check for the MFMA operand layouts.
//
// Operand layouts of v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md §3):
//   A: lane l holds A[i = l&31][k = l>>5]      B: lane l holds B[k = l>>5][j = l&31]
//   D: lane l, reg r holds D[i = (r&3) + 8*(r>>2) + 4*(l>>5)][j = l&31]
#include "common.h"
#include "mfma_io.h"
#include "x3.h"

namespace {

using namespace gcl::mfma_io;  // f32x16, d_row, buffer loads / stores, zero4 (mfma_io.h)
using namespace gcl::plan;     // the dispatch plans and the constants they share with the kernels (dense_plan.h)

#include "gemm_tile.h"  // also EPI_BIAS / EPI_DX and GCL_ST_AUX

// A/B switch while tuning (kernel argument `abl` bit 8 = keep the per-tile block barriers of round 1)
#define gcl_lin_sync() ((abl & 8) != 0)

// ---------------------------------------------------------------------------------------------
// Y[r, j] = sum_k act(X[r,k]) * Wl[j,k]   with Wl[j,k] = TRANS ? W[k*ldw + j] : W[j*ldw + k]
//   EPI_BIAS: + bias[j]
//   EPI_DX  : * PReLU'(Z[r,j]) and the per-block sum of value*min(0,Z) goes to slope_part[block]
// Block = blockDim.x/64 waves, each wave owns 32 rows of a tile; persistent over tiles.  The weight
// panel is staged once per block into LDS with an odd row stride (conflict-free ds_read_b32 for the
// 32-lanes-same-k fragment reads).  Row tiles are software-pipelined through registers: the global
// loads of tile t+1 are issued before the MFMA loop of tile t and committed to LDS (with the
// activation applied) after it, so HBM latency hides under the matrix work instead of being paid
// once per tile.  KT = compile-time bound on K (size of the prefetch register array).
// ---------------------------------------------------------------------------------------------
// (lin_min_waves, the waves per SIMD the register allocator must leave room for: dense_plan.h)
// wide panels (NS >= 4) fill the LDS with one block per CU, i.e. one wave per SIMD: give those
// instantiations the whole register file and fetch Z before the MFMA loop instead of after it
constexpr bool lin_zpre(int NS, int EPI) { return EPI == 1 && NS >= 4; }

template <int NS, int EPI, int KT, bool VEC>
__global__ __launch_bounds__(256, lin_min_waves(NS, KT)) void linear_mfma_kernel(const float* __restrict__ X, int64_t ldx,
                                                          const float* __restrict__ in_slope,
                                                          const float* __restrict__ W, int32_t ldw, int32_t trans,
                                                          const float* __restrict__ bias, float* __restrict__ Y,
                                                          int64_t ldy, int64_t rows, int32_t K, int32_t N,
                                                          const float* __restrict__ Z, int64_t ldz,
                                                          const float* __restrict__ z_slope,
                                                          double* __restrict__ slope_part, int32_t akind,
                                                          int32_t abl) {
  // abl: timing-only ablation bits of tools/ablate.sh (0 in the product): 1 = drop the stores (empty
  // window), 2 = skip the MFMA loop, 4 = loads read the zero page.  Runtime values: codegen is unchanged.
  extern __shared__ __align__(16) float smem[];
  const int KE = (K + 3) & ~3;        // K padded to a multiple of 4 (two MFMA k-steps per 8-B read)
  const int KP = KE + 2;              // even stride with KP/2 odd: conflict-free ds_read_b64 fragments
  float* Wl = smem;                   // [NS*32][KP]
  float* Xl = smem + (size_t)NS * 32 * KP;  // [waves][32][KP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = blockDim.x;
  const int TM = (NT >> 6) * 32;  // rows per tile

  // weight panel: 8 independent loads in flight per thread before the first LDS write (a load -> wait ->
  // write loop costs one L2 round trip per element and that latency is paid by every block's first tile)
  for (int base = 0; base < NS * 32 * KE; base += NT * 8) {
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * NT + tid;
      const int j = idx / KE, k = idx - j * KE;
      const bool ok = (idx < NS * 32 * KE) && (j < N) && (k < K);
      const float* src = ok ? (trans ? W + (int64_t)k * ldw + j : W + (int64_t)j * ldw + k)
                            : reinterpret_cast<const float*>(zero4);
      wv[u] = *src;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * NT + tid;
      const int j = idx / KE, k = idx - j * KE;
      if (idx < NS * 32 * KE) Wl[j * KP + k] = wv[u];
    }
  }
  // akind: activation of X (EPI_BIAS) or of Z (EPI_DX); PReLU reads its slope from in_slope / z_slope
  const float slope = in_slope ? *in_slope : 1.f;
  const bool act = EPI == EPI_BIAS && akind != gcl::kActNone;
  const bool silu = akind == gcl::kActSilu;
  float* Xw = Xl + (size_t)wave * 32 * KP;
  const int64_t ntiles = (rows + TM - 1) / TM;
  double slope_acc = 0.0;  // fp64: the slope gradient is a long signed sum with heavy cancellation
  const float zs = (EPI == EPI_DX && z_slope) ? *z_slope : 1.f;

  // Staging map of a wave's 32 x K tile (no divisions).  VEC: a row is KT/4 float4 columns, a
  // wave-instruction covers 64/(KT/4) rows; scalar: a row is KT columns, KT/64 instructions per row.
  constexpr int CPR = VEC ? KT / 4 : KT;                  // columns (float4 or float) per row slot
  constexpr int RPI = CPR >= 64 ? 1 : 64 / CPR;           // rows per wave-instruction
  constexpr int IPR = CPR >= 64 ? CPR / 64 : 1;           // instructions per row
  constexpr int NIT = (32 / RPI) * IPR;                   // wave-instructions per tile
  const int rsub = (CPR >= 64) ? 0 : lane / CPR;
  const int csub = (CPR >= 64) ? lane : lane % CPR;
  float pre[VEC ? NIT * 4 : NIT];
  const int64_t rows_ld = (abl & 4) ? 0 : rows;
  auto issue = [&](int64_t tile) {  // rows past the end (and tiles past the last) read the zero page
    const int64_t r0 = tile * TM + wave * 32;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int64_t row = r0 + (it / IPR) * RPI + rsub;
      const int c = csub + 64 * (it % IPR);
      if (VEC) {
        const bool ok = (c * 4 < K) && (row < rows_ld);
        const float4* p = ok ? reinterpret_cast<const float4*>(X + row * ldx + c * 4) : zero4;
        const float4 v = *p;
        pre[4 * it] = v.x; pre[4 * it + 1] = v.y; pre[4 * it + 2] = v.z; pre[4 * it + 3] = v.w;
      } else {
        const bool ok = (c < K) && (row < rows_ld);
        const float* p = ok ? X + row * ldx + c : reinterpret_cast<const float*>(zero4);
        pre[it] = *p;
      }
    }
  };
  // Activation while committing: PReLU and "none" share one branch-free form (x > 0 ? x : x * a with a = 1 for
  // none: exact); SiLU is a block-uniform variant of the whole commit, not a branch per element.
  const float pa = (act && !silu) ? slope : 1.f;
  auto commit = [&]() {
    if (act && silu) {
#pragma unroll
      for (int q = 0; q < (VEC ? NIT * 4 : NIT); ++q) pre[q] = gcl::silu_f(pre[q]);
    } else {
#pragma unroll
      for (int q = 0; q < (VEC ? NIT * 4 : NIT); ++q) pre[q] = pre[q] > 0.f ? pre[q] : pre[q] * pa;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int r = (it / IPR) * RPI + rsub;
      const int c = csub + 64 * (it % IPR);
      if (VEC) {
        if (c * 4 < KE) {
          float2* d = reinterpret_cast<float2*>(Xw + r * KP + c * 4);
          d[0] = make_float2(pre[4 * it], pre[4 * it + 1]);
          d[1] = make_float2(pre[4 * it + 2], pre[4 * it + 3]);
        }
      } else {
        if (c < KE) Xw[r * KP + c] = pre[it];  // zero beyond K
      }
    }
  };

  // bias of this lane's columns (loaded once, outside the tile loop)
  float bj[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int j = s * 32 + (lane & 31);
    bj[s] = (EPI == EPI_BIAS && bias && j < N) ? bias[j] : 0.f;
  }
  const bool has_z = (EPI == EPI_DX) && (Z != nullptr);

  issue(blockIdx.x);
  __syncthreads();  // the weight panel is staged; from here on every wave only touches ITS rows of Xl
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // No block barrier inside the loop: a wave's staging rows are private to it and LDS operations of one
    // wave complete in order, so the waves of a block (and of the other blocks on the CU) drift apart and one
    // wave's MFMA chain overlaps the others' loads, LDS commits and stores.
    if (!gcl_lin_sync()) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    else __syncthreads();
    commit();
    if (gcl_lin_sync()) __syncthreads();
    issue(t + gridDim.x);  // unconditional: an empty window past the last tile returns zeros

    const int64_t r0 = t * TM;
    const int64_t nr = (rows - r0) < TM ? (rows - r0) : TM;
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(Y + r0 * ldy, (abl & 1) ? 0 : win_bytes(nr, ldy, N));
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(has_z ? Z + r0 * ldz : Y, has_z ? win_bytes(nr, ldz, N) : 0);

    f32x16 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;

    constexpr bool ZPRE = lin_zpre(NS, EPI);
    float zpre[ZPRE ? NS : 1][16];
    if (ZPRE) {  // Z of this tile: in flight during the MFMA loop
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int j = s * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = wave * 32 + d_row(r, lane);
          zpre[ZPRE ? s : 0][r] = buf_ld1(rz, (j < N) ? (unsigned)((rr * ldz + j) * 4) : kOOB);
        }
      }
    }

    // k-step pair q covers k = 4q..4q+3: lane half h reads the 8 bytes k = 4q+2h, 4q+2h+1 and
    // feeds .x to the first MFMA (k = 4q | 4q+2) and .y to the second (k = 4q+1 | 4q+3); A and B
    // use the same assignment.  Fragments of pair q+1 are read before the MFMAs of pair q issue.
    const float* ap = Xw + (lane & 31) * KP + 2 * (lane >> 5);
    const float* bp = Wl + (lane & 31) * KP + 2 * (lane >> 5);
    const int nq = (abl & 2) ? 0 : (KE >> 2);
    float2 a_c = *reinterpret_cast<const float2*>(ap);
    float2 b_c[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) b_c[s] = *reinterpret_cast<const float2*>(bp + s * 32 * KP);
    for (int q = 0; q < nq; ++q) {
      // reads one pair ahead; the last iteration re-reads pair nq-1 (in range, unused)
      const int qn = (q + 1 < nq) ? q + 1 : q;
      const float2 a_n = *reinterpret_cast<const float2*>(ap + qn * 4);
      float2 b_n[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) b_n[s] = *reinterpret_cast<const float2*>(bp + s * 32 * KP + qn * 4);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.x, b_c[s].x, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.y, b_c[s].y, acc[s], 0, 0, 0);
      a_c = a_n;
#pragma unroll
      for (int s = 0; s < NS; ++s) b_c[s] = b_n[s];
    }

    // epilogue: lane owns column j = s*32 + (lane&31) and 16 rows; all accesses unconditional
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int j = s * 32 + (lane & 31);
      const bool jok = j < N;
      if (EPI == EPI_DX) {
        float zv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = wave * 32 + d_row(r, lane);
          if (ZPRE) zv[r] = zpre[ZPRE ? s : 0][r];
          else zv[r] = buf_ld1(rz, jok ? (unsigned)((rr * ldz + j) * 4) : kOOB);  // 0 when absent / out of range
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = wave * 32 + d_row(r, lane);
          float v = acc[s][r];
          if (silu) {  // block-uniform
            v *= has_z ? gcl::dsilu_f(zv[r]) : 1.f;
          } else {
            const bool neg = has_z && !(zv[r] > 0.f);
            slope_acc += neg ? (double)(v * zv[r]) : 0.0;
            v = neg ? v * zs : v;
          }
          buf_st1<GCL_ST_AUX>(ry, jok ? (unsigned)((rr * ldy + j) * 4) : kOOB, v);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = wave * 32 + d_row(r, lane);
          buf_st1<GCL_ST_AUX>(ry, jok ? (unsigned)((rr * ldy + j) * 4) : kOOB, acc[s][r] + bj[s]);
        }
      }
    }
  }

  if (EPI == EPI_DX && slope_part) {
    for (int off = 32; off > 0; off >>= 1) slope_acc += __shfl_down(slope_acc, off, 64);
    __syncthreads();
    double* dred = reinterpret_cast<double*>(smem);
    if (lane == 0) dred[wave] = slope_acc;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int wv = 0; wv < (NT >> 6); ++wv) tot += dred[wv];
      slope_part[blockIdx.x] = tot;
    }
  }
}

// Simple VALU implementation of the same contract (cross-check; one thread per output element).
template <int EPI>
__global__ __launch_bounds__(256) void linear_valu_kernel(const float* __restrict__ X, int64_t ldx,
                                                          const float* __restrict__ in_slope,
                                                          const float* __restrict__ W, int32_t ldw, int32_t trans,
                                                          const float* __restrict__ bias, float* __restrict__ Y,
                                                          int64_t ldy, int64_t rows, int32_t K, int32_t N,
                                                          const float* __restrict__ Z, int64_t ldz,
                                                          const float* __restrict__ z_slope,
                                                          double* __restrict__ slope_part, int32_t akind) {
  __shared__ double red[4];
  const float slope = in_slope ? *in_slope : 1.f;
  const bool act = EPI == EPI_BIAS && akind != gcl::kActNone;
  const float zs = (EPI == EPI_DX && z_slope) ? *z_slope : 1.f;
  double slope_acc = 0.0;
  const int64_t total = rows * N;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t r = idx / N;
    const int j = (int)(idx - r * N);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      float xv = X[r * ldx + k];
      if (act) xv = gcl::act_f(xv, slope, akind);
      const float wv = trans ? W[(int64_t)k * ldw + j] : W[(int64_t)j * ldw + k];
      acc = fmaf(xv, wv, acc);
    }
    if (EPI == EPI_BIAS) {
      if (bias) acc += bias[j];
    } else if (Z) {
      const float z = Z[r * ldz + j];
      if (akind == gcl::kActSilu) {
        acc *= gcl::dsilu_f(z);
      } else if (!(z > 0.f)) {  // (NaN takes the slope branch, as in the forward and in torch)
        slope_acc += (double)(acc * z);
        acc *= zs;
      }
    }
    Y[r * ldy + j] = acc;
  }
  if (EPI == EPI_DX && slope_part) {
    for (int off = 32; off > 0; off >>= 1) slope_acc += __shfl_down(slope_acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = slope_acc;
    __syncthreads();
    if (threadIdx.x == 0) slope_part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  }
}

// ---------------------------------------------------------------------------------------------
// dW partials:  P[block][o][c] = sum_{r in block's rows} dY[r,o] * act(X[r,c])   (+ db partials)
// A tall-skinny contraction over rows.  Each block walks its row range in 64-row steps: the dY and
// act(X) rows of a step are fetched with 16-B loads into registers one step ahead (software
// pipeline), committed to LDS, and the 4 waves run v_mfma_f32_32x32x2_f32 with A = dY^T and B = X
// fragments read from LDS (lanes 0-31 read 32 consecutive channels of row k, lanes 32-63 of row
// k+1: conflict-free).  The 32x32 output tiles are split over the waves as a WO x WC grid; wave
// (wo,wc) owns o-slabs {wo, wo+WO, ..} x c-slabs {wc, wc+WC, ..} (TO x TC accumulators), so no
// cross-wave reduction is needed.  One partial tile set per block, reduced by reduce_parts_kernel.
// ---------------------------------------------------------------------------------------------
// (kDwRT = 64 rows per step: dense_plan.h)
template <int NO, int NC>
struct DwCfg {
  static constexpr int WO = NO >= 4 ? 4 : NO;         // waves along the output-channel slabs
  static constexpr int WC = 4 / WO;                   // waves along the input-channel slabs
  static constexpr int TO = NO / WO;                  // o-slabs per wave
  static constexpr int TC = (NC + WC - 1) / WC;       // c-slabs per wave
  static constexpr int PRE = 2 * (NO + NC);           // float4 staging registers per thread
  static constexpr int FoutP = NO * 32, FinP = NC * 32;
  static constexpr int min_waves = (PRE <= 8 && TO * TC <= 2) ? 3 : (PRE <= 16 && TO * TC <= 4) ? 2 : 1;
};

template <int NO, int NC, bool VEC>
__global__ __launch_bounds__(256, (DwCfg<NO, NC>::min_waves)) void dw_mfma_kernel(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ X, int64_t ldx,
    const float* __restrict__ in_slope, float* __restrict__ part, float* __restrict__ dbpart, int64_t rows,
    int32_t Fin_all, int32_t Fout, int64_t rows_per_block, int32_t akind, int64_t tile_stride) {
  using Cfg = DwCfg<NO, NC>;
  // blockIdx.y = 128-column chunk of the input features (one launch covers a whole wide dW)
  const int ct = blockIdx.y;
  X += (int64_t)ct * 128;
  part += (int64_t)ct * tile_stride;
  if (ct != 0) dbpart = nullptr;
  const int Fin = (Fin_all - ct * 128) < 128 ? (Fin_all - ct * 128) : 128;
  constexpr int WO = Cfg::WO, WC = Cfg::WC, TO = Cfg::TO, TC = Cfg::TC, PRE = Cfg::PRE;
  constexpr int FoutP = Cfg::FoutP, FinP = Cfg::FinP;
  extern __shared__ __align__(16) float smem[];
  float* Yl = smem;                          // [kDwRT][FoutP]
  float* Xl = smem + (size_t)kDwRT * FoutP;  // [kDwRT][FinP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int wo = wave % WO, wc = wave / WO;
  const float slope = in_slope ? *in_slope : 1.f;
  const bool act = akind != gcl::kActNone;
  const int64_t rb = (int64_t)blockIdx.x * rows_per_block;
  const int64_t re = min(rows, rb + rows_per_block);
  const int nrows = (int)(re - rb);

  f32x16 acc[TO][TC];
#pragma unroll
  for (int a = 0; a < TO; ++a)
#pragma unroll
    for (int c = 0; c < TC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
  float dbacc[TO];
#pragma unroll
  for (int a = 0; a < TO; ++a) dbacc[a] = 0.f;

  // Staging map of a 64-row step (no divisions): thread = (row slot rs = tid/8, column group
  // cg = tid%8); it owns rows rs and rs+32 and the float4 columns cg + 8*j of dY (j < NO) and of
  // X (j < NC).  8 consecutive lanes read 128 contiguous bytes.  All loads are unconditional:
  // rows past the block's range and columns past F read the zero page.
  const int rs = tid >> 3, cg = tid & 7;
  float4 pre[PRE];
  const float* ybase = dY + rb * lddy;
  const float* xbase = X + rb * ldx;
  auto ld_slot = [&](const float* base, int rr, int c4, int64_t ld, int F) -> float4 {
    const bool ok = rr < nrows;
    const float* z = reinterpret_cast<const float*>(zero4);
    const float* src = base + (int64_t)rr * ld + c4;
    if (VEC) return *reinterpret_cast<const float4*>((ok && c4 < F) ? src : z);
    float4 v;
    v.x = *((ok && c4 < F) ? src : z);
    v.y = *((ok && c4 + 1 < F) ? src + 1 : z);
    v.z = *((ok && c4 + 2 < F) ? src + 2 : z);
    v.w = *((ok && c4 + 3 < F) ? src + 3 : z);
    return v;
  };
  auto issue = [&](int rel0) {
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int j = it >> 1;
      const int rr = rel0 + rs + 32 * (it & 1);
      if (j < NO) pre[it] = ld_slot(ybase, rr, (cg + 8 * j) * 4, lddy, Fout);
      else pre[it] = ld_slot(xbase, rr, (cg + 8 * (j - NO)) * 4, ldx, Fin);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int j = it >> 1;
      const int r = rs + 32 * (it & 1);
      float4 v = pre[it];
      if (j < NO) {
        *reinterpret_cast<float4*>(Yl + r * FoutP + (cg + 8 * j) * 4) = v;
      } else {
        if (act) {
          v.x = gcl::act_f(v.x, slope, akind); v.y = gcl::act_f(v.y, slope, akind);
          v.z = gcl::act_f(v.z, slope, akind); v.w = gcl::act_f(v.w, slope, akind);
        }
        *reinterpret_cast<float4*>(Xl + r * FinP + (cg + 8 * (j - NO)) * 4) = v;
      }
    }
  };

  issue(0);
  for (int rel0 = 0; rel0 < nrows; rel0 += kDwRT) {
    __syncthreads();
    commit();
    __syncthreads();
    issue(rel0 + kDwRT);  // unconditional (zeros past the end)
    const float* yp = Yl + lk * FoutP + li;
    const float* xp = Xl + lk * FinP + li;
    float av[TO], bv[TC];
#pragma unroll
    for (int a = 0; a < TO; ++a) av[a] = yp[(wo + a * WO) * 32];
#pragma unroll
    for (int c = 0; c < TC; ++c) {
      const int sc = wc + c * WC;
      bv[c] = (sc < NC) ? xp[sc * 32] : 0.f;
    }
    for (int k = 0; k < kDwRT; k += 2) {
      // fragments of the next row pair, read before this pair's MFMAs issue (last: re-read)
      const int kn = (k + 2 < kDwRT) ? k + 2 : k;
      float an[TO], bn[TC];
#pragma unroll
      for (int a = 0; a < TO; ++a) an[a] = yp[kn * FoutP + (wo + a * WO) * 32];
#pragma unroll
      for (int c = 0; c < TC; ++c) {
        const int sc = wc + c * WC;
        bn[c] = (sc < NC) ? xp[kn * FinP + sc * 32] : 0.f;
      }
#pragma unroll
      for (int a = 0; a < TO; ++a) {
        dbacc[a] += av[a];
#pragma unroll
        for (int c = 0; c < TC; ++c)
          acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[c], acc[a][c], 0, 0, 0);
      }
#pragma unroll
      for (int a = 0; a < TO; ++a) av[a] = an[a];
#pragma unroll
      for (int c = 0; c < TC; ++c) bv[c] = bn[c];
    }
  }

  float* out = part + (size_t)blockIdx.x * FoutP * FinP;
#pragma unroll
  for (int a = 0; a < TO; ++a) {
    const int so = wo + a * WO;
#pragma unroll
    for (int c = 0; c < TC; ++c) {
      const int sc = wc + c * WC;
      if (sc < NC) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          out[(size_t)(so * 32 + d_row(r, lane)) * FinP + sc * 32 + li] = acc[a][c][r];
      }
    }
    if (dbpart && wc == 0) {
      const float d = dbacc[a] + __shfl_xor(dbacc[a], 32, 64);
      if (lane < 32) dbpart[(size_t)blockIdx.x * FoutP + so * 32 + lane] = d;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Fused backward of  y = act(x) W^T (+ b):  one pass over dY and the pre-activation input P.
//   dX[r,c]  = (sum_o dY[r,o] W[o,c]) * PReLU'(P[r,c])          -> global (raw buffer stores)
//   dW[o,c] += sum_r dY[r,o] act(P[r,c])                         -> per-block partial tiles
//   db[o]   += sum_r dY[r,o],  cs[c] += sum_r dX[r,c],  dslope += sum dX_preact * min(0,P)
// Traffic per call: read dY + read P + write dX (600 MB at 786k x 64) instead of the 1600 MB the
// separate dx / dW / colsum launches move, because P doubles as Z (PReLU') and as X (dW), and dY
// is read once.  One 4-wave block per CU (LDS ~84 KB at 64x64), one wave per SIMD, explicit
// register prefetch of the next tile during the ~8k MFMA cycles of the current one.
//   LDS: Wt[FiP][KPo] (W transposed, for dX), dYl[128][KPo] (row-major: A of dX as 8-B fragments,
//   A' of dW as channel-contiguous 4-B fragments), Pl[128][FiP] (pre-activation; PReLU is applied
//   when the B' fragment is formed, PReLU' in the dX epilogue).
// Constraints (else the caller falls back to the separate kernels): Fout <= 64, Fin <= 96,
// Fout % 4 == Fin % 4 == 0, 16-B aligned rows.
// ---------------------------------------------------------------------------------------------
template <int NO, int NC>
__global__ __launch_bounds__(256, 1) void linear_bwd_fused_kernel(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ W, const float* __restrict__ P,
    int64_t ldp, const float* __restrict__ in_slope, float* __restrict__ dX, int64_t lddx, int64_t rows, int32_t Fin,
    int32_t Fout, float* __restrict__ part_dw, float* __restrict__ part_db, float* __restrict__ part_cs,
    double* __restrict__ part_slope) {
  constexpr int FoP = NO * 32, FiP = NC * 32;
  constexpr int KPo = FoP + 2;             // even stride, KPo/2 odd
  constexpr int TM = 128;
  constexpr int NT = NO * NC;              // dW tiles
  constexpr int TPW = (NT + 3) / 4;        // dW tiles per wave
  constexpr int CY = FoP / 4;              // float4 columns of a dY row (8 or 16)
  constexpr int CP = NC == 3 ? 32 : FiP / 4;  // float4 column slots of a P row (power of two)
  constexpr int RY = 64 / CY, RP = 64 / CP;   // rows per wave-instruction
  constexpr int NY = 32 / RY, NP = 32 / RP;   // wave-instructions per 32-row slice
  extern __shared__ __align__(16) float smem[];
  float* Wt = smem;                         // [FiP][KPo]
  float* dYl = Wt + FiP * KPo;              // [TM][KPo]
  float* Pl = dYl + TM * KPo;               // [TM][FiP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;

  for (int idx = tid; idx < FiP * FoP; idx += 256) {  // Wt[c][o] = W[o][c], zero padded
    const int c = idx / FoP, o = idx - c * FoP;
    Wt[c * KPo + o] = (c < Fin && o < Fout) ? W[(int64_t)o * Fin + c] : 0.f;
  }
  const bool act = in_slope != nullptr;
  const float slope = act ? *in_slope : 1.f;
  const int64_t ntiles = (rows + TM - 1) / TM;

  f32x16 dw[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) dw[q][r] = 0.f;
  float dbacc[TPW], cs[NC];
#pragma unroll
  for (int q = 0; q < TPW; ++q) dbacc[q] = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < NC; ++s2) cs[s2] = 0.f;
  double slope_acc = 0.0;

  const int ysub = lane / CY, ycol = lane % CY, psub = lane / CP, pcol = lane % CP;
  float4 pre[NY + NP];
  const float4* zero = zero4;
  auto issue = [&](int64_t tile) {
    const int64_t r0 = tile * TM + wave * 32;
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int64_t row = r0 + it * RY + ysub;
      const bool ok = (ycol * 4 < Fout) && (row < rows);
      pre[it] = *(ok ? reinterpret_cast<const float4*>(dY + row * lddy + ycol * 4) : zero);
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int64_t row = r0 + it * RP + psub;
      const bool ok = (pcol * 4 < Fin) && (row < rows);
      pre[NY + it] = *(ok ? reinterpret_cast<const float4*>(P + row * ldp + pcol * 4) : zero);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int r = wave * 32 + it * RY + ysub;
      float2* d = reinterpret_cast<float2*>(dYl + r * KPo + ycol * 4);
      const float4 v = pre[it];
      d[0] = make_float2(v.x, v.y);
      d[1] = make_float2(v.z, v.w);
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int r = wave * 32 + it * RP + psub;
      const float4 v = pre[NY + it];
      if (pcol * 4 < FiP) *reinterpret_cast<float4*>(Pl + r * FiP + pcol * 4) = v;
    }
  };

  issue(blockIdx.x);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();
    commit();
    __syncthreads();
    issue(t + gridDim.x);

    const int64_t r0 = t * TM;
    const int64_t nr = (rows - r0) < TM ? (rows - r0) : TM;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(dX + r0 * lddx, win_bytes(nr, lddx, Fin));

    // ---- dX slice of this wave: [32 x Fin] = dYl[32 rows] (K = Fout) x Wt ----
    f32x16 acc[NC];
#pragma unroll
    for (int s2 = 0; s2 < NC; ++s2)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[s2][r] = 0.f;
    {
      const float* ap = dYl + (wave * 32 + li) * KPo + 2 * lk;
      const float* bp = Wt + li * KPo + 2 * lk;
      constexpr int nq = FoP / 4;
      float2 a_c = *reinterpret_cast<const float2*>(ap);
      float2 b_c[NC];
#pragma unroll
      for (int s2 = 0; s2 < NC; ++s2) b_c[s2] = *reinterpret_cast<const float2*>(bp + s2 * 32 * KPo);
#pragma unroll 2
      for (int q = 0; q < nq; ++q) {
        const int qn = (q + 1 < nq) ? q + 1 : q;
        const float2 a_n = *reinterpret_cast<const float2*>(ap + qn * 4);
        float2 b_n[NC];
#pragma unroll
        for (int s2 = 0; s2 < NC; ++s2) b_n[s2] = *reinterpret_cast<const float2*>(bp + s2 * 32 * KPo + qn * 4);
#pragma unroll
        for (int s2 = 0; s2 < NC; ++s2)
          acc[s2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.x, b_c[s2].x, acc[s2], 0, 0, 0);
#pragma unroll
        for (int s2 = 0; s2 < NC; ++s2)
          acc[s2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.y, b_c[s2].y, acc[s2], 0, 0, 0);
        a_c = a_n;
#pragma unroll
        for (int s2 = 0; s2 < NC; ++s2) b_c[s2] = b_n[s2];
      }
    }
    // epilogue: PReLU' from the LDS copy of P, slope / column-sum accumulation; branch-free (all
    // 16 Z reads of a slab are issued together, masks are selects, stores are unconditional)
#pragma unroll
    for (int s2 = 0; s2 < NC; ++s2) {
      const int j = s2 * 32 + li;
      const bool jok = j < Fin;
      float zv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) zv[r] = Pl[(wave * 32 + d_row(r, lane)) * FiP + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = wave * 32 + d_row(r, lane);
        float v = acc[s2][r];
        const bool neg = act && !(zv[r] > 0.f);
        slope_acc += neg ? (double)(v * zv[r]) : 0.0;
        v = neg ? v * slope : v;
        cs[s2] += v;
        buf_st1<GCL_ST_AUX>(rx, jok ? (unsigned)((rr * lddx + j) * 4) : kOOB, v);
      }
    }

    // ---- dW tiles of this wave over all 128 rows of the tile ----
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      const int tix = wave + 4 * q;
      if (tix < NT) {  // wave-uniform
        const int so = tix % NO, sc = tix / NO;
        const float* yp = dYl + lk * KPo + so * 32 + li;
        const float* xp = Pl + lk * FiP + sc * 32 + li;
        constexpr int DP = 4;  // LDS fragments are read 4 row pairs ahead of their MFMAs
        float av[DP], bv[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          av[d] = yp[(2 * d) * KPo];
          bv[d] = xp[(2 * d) * FiP];
        }
        for (int k = 0; k < TM; k += 2 * DP) {
          float an[DP], bn[DP];
#pragma unroll
          for (int d = 0; d < DP; ++d) {
            const int kn = (k + 2 * DP + 2 * d < TM) ? k + 2 * DP + 2 * d : 2 * d;
            an[d] = yp[kn * KPo];
            bn[d] = xp[kn * FiP];
          }
#pragma unroll
          for (int d = 0; d < DP; ++d) {
            const float bx = act ? gcl::prelu_f(bv[d], slope) : bv[d];
            if (sc == 0) dbacc[q] += av[d];
            dw[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[d], bx, dw[q], 0, 0, 0);
          }
#pragma unroll
          for (int d = 0; d < DP; ++d) {
            av[d] = an[d];
            bv[d] = bn[d];
          }
        }
      }
    }
  }

  // ---- per-block partials ----
  constexpr size_t REC = (size_t)FoP * FiP + FoP + FiP;  // per-block record: [dW | db | colsum]
  float* out = part_dw + (size_t)blockIdx.x * REC;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int tix = wave + 4 * q;
    if (tix < NT) {
      const int so = tix % NO, sc = tix / NO;
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(size_t)(so * 32 + d_row(r, lane)) * FiP + sc * 32 + li] = dw[q][r];
      if (part_db && sc == 0) {
        const float d = dbacc[q] + __shfl_xor(dbacc[q], 32, 64);
        if (lane < 32) part_db[(size_t)blockIdx.x * REC + so * 32 + lane] = d;
      }
    }
  }
  __syncthreads();  // LDS is free: reuse it for the cross-wave column sums and the slope partial
  float* red = smem;  // [4][FiP]
#pragma unroll
  for (int s2 = 0; s2 < NC; ++s2) {
    const float v = cs[s2] + __shfl_xor(cs[s2], 32, 64);
    if (lane < 32) red[wave * FiP + s2 * 32 + lane] = v;
  }
  for (int off = 32; off > 0; off >>= 1) slope_acc += __shfl_down(slope_acc, off, 64);
  double* dred = reinterpret_cast<double*>(smem + 4 * FiP);
  if (lane == 0) dred[wave] = slope_acc;
  __syncthreads();
  if (part_cs)
    for (int c = tid; c < FiP; c += 256)
      part_cs[(size_t)blockIdx.x * REC + c] = (red[c] + red[FiP + c]) + (red[2 * FiP + c] + red[3 * FiP + c]);
  if (part_slope && tid == 0) part_slope[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}

// ---------------------------------------------------------------------------------------------
// Fused backward, 64-wide input panel (Fin in 33..64), 64-row tiles: 50 KB of LDS per block, so
// THREE blocks (12 waves) share a CU instead of one - the loads of one block hide behind the MFMAs
// of the others.  Waves are (row group rg = w&1, column slab sg = w>>1): wave (rg,sg) computes the
// dX slice rows 32rg.. x columns 32sg.., and dW tile w (of NO x 2) over the tile's 64 rows.
// Same partial-record layout and outputs as linear_bwd_fused_kernel.
// ---------------------------------------------------------------------------------------------
template <int NO>
__global__ __launch_bounds__(256, 3) void linear_bwd_fused64_kernel(
    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ W, const float* __restrict__ P,
    int64_t ldp, const float* __restrict__ in_slope, float* __restrict__ dX, int64_t lddx, int64_t rows, int32_t Fin,
    int32_t Fout, float* __restrict__ part_dw, float* __restrict__ part_db, float* __restrict__ part_cs,
    double* __restrict__ part_slope) {
  constexpr int NC = 2;
  constexpr int FoP = NO * 32, FiP = NC * 32;
  constexpr int KPo = FoP + 2;
  constexpr int TM = 64;
  constexpr int NT = NO * NC;
  constexpr int CY = FoP / 4, CP = FiP / 4;     // float4 columns per row (8|16, 16)
  constexpr int RY = 64 / CY, RP = 64 / CP;     // rows per wave-instruction
  constexpr int NY = 16 / RY, NP = 16 / RP;     // wave-instructions per 16-row slice
  extern __shared__ __align__(16) float smem[];
  float* Wt = smem;               // [FiP][KPo]
  float* dYl = Wt + FiP * KPo;    // [TM][KPo]
  float* Pl = dYl + TM * KPo;     // [TM][FiP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int rg = wave & 1, sg = wave >> 1;

  for (int idx = tid; idx < FiP * FoP; idx += 256) {
    const int c = idx / FoP, o = idx - c * FoP;
    Wt[c * KPo + o] = (c < Fin && o < Fout) ? W[(int64_t)o * Fin + c] : 0.f;
  }
  const bool act = in_slope != nullptr;
  const float slope = act ? *in_slope : 1.f;
  const int64_t ntiles = (rows + TM - 1) / TM;

  f32x16 dw;
#pragma unroll
  for (int r = 0; r < 16; ++r) dw[r] = 0.f;
  float dbacc = 0.f, cs = 0.f;
  double slope_acc = 0.0;
  const bool has_tile = wave < NT;
  const int so = wave % NO, sc = wave / NO;

  const int ysub = lane / CY, ycol = lane % CY, psub = lane / CP, pcol = lane % CP;
  float4 pre[NY + NP];
  const float4* zero = zero4;
  auto issue = [&](int64_t tile) {
    const int64_t r0 = tile * TM + wave * 16;
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int64_t row = r0 + it * RY + ysub;
      const bool ok = (ycol * 4 < Fout) && (row < rows);
      pre[it] = *(ok ? reinterpret_cast<const float4*>(dY + row * lddy + ycol * 4) : zero);
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int64_t row = r0 + it * RP + psub;
      const bool ok = (pcol * 4 < Fin) && (row < rows);
      pre[NY + it] = *(ok ? reinterpret_cast<const float4*>(P + row * ldp + pcol * 4) : zero);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < NY; ++it) {
      const int r = wave * 16 + it * RY + ysub;
      float2* d = reinterpret_cast<float2*>(dYl + r * KPo + ycol * 4);
      const float4 v = pre[it];
      d[0] = make_float2(v.x, v.y);
      d[1] = make_float2(v.z, v.w);
    }
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int r = wave * 16 + it * RP + psub;
      *reinterpret_cast<float4*>(Pl + r * FiP + pcol * 4) = pre[NY + it];
    }
  };

  issue(blockIdx.x);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();
    commit();
    __syncthreads();
    issue(t + gridDim.x);

    const int64_t r0 = t * TM;
    const int64_t nr = (rows - r0) < TM ? (rows - r0) : TM;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(dX + r0 * lddx, win_bytes(nr, lddx, Fin));

    // ---- dX slice: rows 32rg.., columns 32sg.. ----
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    {
      const float* ap = dYl + (rg * 32 + li) * KPo + 2 * lk;
      const float* bp = Wt + (sg * 32 + li) * KPo + 2 * lk;
      constexpr int nq = FoP / 4;
      float2 a_c = *reinterpret_cast<const float2*>(ap);
      float2 b_c = *reinterpret_cast<const float2*>(bp);
#pragma unroll 4
      for (int q = 0; q < nq; ++q) {
        const int qn = (q + 1 < nq) ? q + 1 : q;
        const float2 a_n = *reinterpret_cast<const float2*>(ap + qn * 4);
        const float2 b_n = *reinterpret_cast<const float2*>(bp + qn * 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.x, b_c.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_c.y, b_c.y, acc, 0, 0, 0);
        a_c = a_n;
        b_c = b_n;
      }
    }
    {
      const int j = sg * 32 + li;
      const bool jok = j < Fin;
      float zv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) zv[r] = Pl[(rg * 32 + d_row(r, lane)) * FiP + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = rg * 32 + d_row(r, lane);
        float v = acc[r];
        const bool neg = act && !(zv[r] > 0.f);
        slope_acc += neg ? (double)(v * zv[r]) : 0.0;
        v = neg ? v * slope : v;
        cs += v;
        buf_st1<GCL_ST_AUX>(rx, jok ? (unsigned)((rr * lddx + j) * 4) : kOOB, v);
      }
    }

    // ---- dW tile of this wave over the 64 rows of the tile ----
    if (has_tile) {  // wave-uniform
      const float* yp = dYl + lk * KPo + so * 32 + li;
      const float* xp = Pl + lk * FiP + sc * 32 + li;
      float av = yp[0], bv = xp[0];
#pragma unroll 4
      for (int k = 0; k < TM; k += 2) {
        const int kn = (k + 2 < TM) ? k + 2 : k;
        const float an = yp[kn * KPo];
        const float bn = xp[kn * FiP];
        const float bx = act ? gcl::prelu_f(bv, slope) : bv;
        dbacc += av;
        dw = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bx, dw, 0, 0, 0);
        av = an;
        bv = bn;
      }
    }
  }

  constexpr size_t REC = (size_t)FoP * FiP + FoP + FiP;
  float* out = part_dw + (size_t)blockIdx.x * REC;
  if (has_tile) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)(so * 32 + d_row(r, lane)) * FiP + sc * 32 + li] = dw[r];
    if (part_db && sc == 0) {
      const float d = dbacc + __shfl_xor(dbacc, 32, 64);
      if (lane < 32) part_db[(size_t)blockIdx.x * REC + so * 32 + lane] = d;
    }
  }
  __syncthreads();
  float* red = smem;  // [4][32]
  {
    const float v = cs + __shfl_xor(cs, 32, 64);
    if (lane < 32) red[wave * 32 + lane] = v;
  }
  for (int off = 32; off > 0; off >>= 1) slope_acc += __shfl_down(slope_acc, off, 64);
  double* dred = reinterpret_cast<double*>(smem + 4 * 32);
  if (lane == 0) dred[wave] = slope_acc;
  __syncthreads();
  if (part_cs && tid < FiP) {
    const int s2 = tid >> 5, c = tid & 31;  // column slab s2 is held by waves 2*s2 (rg 0) and 2*s2+1 (rg 1)
    part_cs[(size_t)blockIdx.x * REC + tid] = red[(2 * s2) * 32 + c] + red[(2 * s2 + 1) * 32 + c];
  }
  if (part_slope && tid == 0) part_slope[blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}

// Wt[c][o] = W[o*ldw + c]  (o < R, c < Cn): lets the dX contraction read its weights k-contiguously
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ W, int64_t ldw, float* __restrict__ Wt,
                                                        int32_t R, int32_t Cn) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int o0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int i = ty; i < 32; i += 8) {
    const int o = o0 + i, c = c0 + tx;
    tile[i][tx] = (o < R && c < Cn) ? W[(int64_t)o * ldw + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, o = o0 + tx;
    if (c < Cn && o < R) Wt[(int64_t)c * R + o] = tile[tx][i];
  }
}

__global__ void reduce_scalar_kernel(const double* __restrict__ part, int32_t nparts, float* __restrict__ out) {
  // single wave; fixed order => deterministic
  double s = 0.0;
  for (int p = threadIdx.x; p < nparts; p += 64) s += part[p];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) *out += (float)s;
}

// Up to 3 output segments reduced in ONE launch: segment g covers `count[g]` consecutive floats of
// every partial record starting at offset `poff[g]`; element e of it goes to out[g][(e / pld) * ldo
// + e % pld] when (e % pld) < cols (partial tiles are padded to pld columns).  16 threads split
// the partial records of one element, combined through LDS in a fixed order.
using RedSeg = gcl_reduce_seg;  // (acc: add into out (1) or overwrite it (0): every destination has its own flag)
__global__ __launch_bounds__(256) void reduce_multi_kernel(const float* __restrict__ part, int32_t nparts,
                                                           int64_t pstride, RedSeg s0, RedSeg s1, RedSeg s2,
                                                           const double* __restrict__ spart, int32_t ns,
                                                           float* __restrict__ sout) {
  if (spart && blockIdx.x == gridDim.x - 1) {  // one extra block: the scalar (PReLU slope) partials, fixed order
    if (threadIdx.x < 64) {
      double t = 0.0;
      for (int p = threadIdx.x; p < ns; p += 64) t += spart[p];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (threadIdx.x == 0) *sout += (float)t;
    }
    return;
  }
  __shared__ float red[16][17];
  const int e16 = threadIdx.x & 15, g = threadIdx.x >> 4;
  int idx = blockIdx.x * 16 + e16;
  RedSeg sg = s0;
  if (idx >= s0.count) {
    idx -= s0.count;
    sg = s1;
    if (idx >= s1.count) {
      idx -= s1.count;
      sg = s2;
    }
  }
  const bool ok = idx < sg.count;
  float s = 0.f;
  if (ok)
    for (int p = g; p < nparts; p += 16) s += part[(size_t)p * pstride + sg.poff + idx];
  red[g][e16] = s;
  __syncthreads();
  if (g == 0 && ok) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += red[q][e16];
    const int i = idx / sg.pld, j = idx - i * sg.pld;
    if (j < sg.cols) {
      float* o = sg.out + (size_t)i * sg.ldo + j;
      *o = sg.acc ? *o + tot : tot;
    }
  }
}

// Same contract, 16-byte loads: a block reduces 32 consecutive floats of the record (8 lanes x float4 =
// one 128-B line per partial record) with 32 groups of lanes striding over the records, then a
// fixed-order combine through LDS.  Needs pstride, every poff and every count to be multiples of 4.
__device__ __forceinline__ void reduce4_block(const float* __restrict__ part, int32_t nparts, int64_t pstride,
                                              const RedSeg& s0, const RedSeg& s1, const RedSeg& s2, int blk);

__global__ __launch_bounds__(256) void reduce_multi4_kernel(const float* __restrict__ part, int32_t nparts,
                                                            int64_t pstride, RedSeg s0, RedSeg s1, RedSeg s2,
                                                            const double* __restrict__ spart, int32_t ns,
                                                            float* __restrict__ sout) {
  if (spart && blockIdx.x == gridDim.x - 1) {  // one extra block: the scalar (PReLU slope) partials, fixed order
    if (threadIdx.x < 64) {
      double t = 0.0;
      for (int p = threadIdx.x; p < ns; p += 64) t += spart[p];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (threadIdx.x == 0) *sout += (float)t;
    }
    return;
  }
  reduce4_block(part, nparts, pstride, s0, s1, s2, blockIdx.x);
}

__device__ __forceinline__ void reduce4_block(const float* __restrict__ part, int32_t nparts, int64_t pstride,
                                              const RedSeg& s0, const RedSeg& s1, const RedSeg& s2, int blk) {
  __shared__ float red[32][33];
  const int l8 = threadIdx.x & 7, g = threadIdx.x >> 3;
  int idx = blk * 32 + l8 * 4;  // first of this lane's 4 elements, in the concatenated segments
  RedSeg sg = s0;
  if (idx >= s0.count) {
    idx -= s0.count;
    sg = s1;
    if (idx >= s1.count) {
      idx -= s1.count;
      sg = s2;
    }
  }
  const bool ok = idx < sg.count;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    const float* base = part + sg.poff + idx;
    int p = g;
    for (; p + 96 < nparts; p += 128) {  // four records in flight per lane
      const float4 a = *reinterpret_cast<const float4*>(base + (size_t)p * pstride);
      const float4 b = *reinterpret_cast<const float4*>(base + (size_t)(p + 32) * pstride);
      const float4 c = *reinterpret_cast<const float4*>(base + (size_t)(p + 64) * pstride);
      const float4 d = *reinterpret_cast<const float4*>(base + (size_t)(p + 96) * pstride);
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
      s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
      s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
      s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
    }
    for (; p < nparts; p += 32) {
      const float4 a = *reinterpret_cast<const float4*>(base + (size_t)p * pstride);
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
  }
  red[g][l8 * 4] = s.x; red[g][l8 * 4 + 1] = s.y; red[g][l8 * 4 + 2] = s.z; red[g][l8 * 4 + 3] = s.w;
  __syncthreads();
  if (threadIdx.x < 32) {
    // element threadIdx.x of the block: recompute its segment position (its lane group's idx + offset)
    int e = blk * 32 + threadIdx.x;
    RedSeg so = s0;
    if (e >= s0.count) {
      e -= s0.count;
      so = s1;
      if (e >= s1.count) {
        e -= s1.count;
        so = s2;
      }
    }
    if (e < so.count) {
      float tot = 0.f;
#pragma unroll
      for (int q = 0; q < 32; ++q) tot += red[q][threadIdx.x];
      const int i = e / so.pld, j = e - i * so.pld;
      if (j < so.cols) {
        float* o = so.out + (size_t)i * so.ldo + j;
        *o = so.acc ? *o + tot : tot;
      }
    }
  }
}

// picks the 16-byte variant when the record layout allows it
inline void launch_reduce_multi(const float* part, int nparts, int64_t pstride, const RedSeg& s0, const RedSeg& s1,
                                const RedSeg& s2, hipStream_t st, const double* spart = nullptr,
                                int ns = 0, float* sout = nullptr) {
  const int total = s0.count + s1.count + s2.count;
  const bool vec = (pstride % 4 == 0) && ((s0.poff | s1.poff | s2.poff | s0.count | s1.count | s2.count) % 4 == 0) &&
                   gcl::aligned16(part) && nparts >= 64;
  const unsigned extra = (spart && sout && ns > 0) ? 1u : 0u;  // one more block for the scalar partials
  const double* sp = extra ? spart : nullptr;
  if (vec)
    hipLaunchKernelGGL(reduce_multi4_kernel, dim3((unsigned)gcl::cdiv(total, 32) + extra), dim3(256), 0, st, part, nparts,
                       pstride, s0, s1, s2, sp, ns, sout);
  else
    hipLaunchKernelGGL(reduce_multi_kernel, dim3((unsigned)gcl::cdiv(total, 16) + extra), dim3(256), 0, st, part, nparts,
                       pstride, s0, s1, s2, sp, ns, sout);
}

// Final pass of up to 24 deferred calls in ONE launch (gcl_reduce_jobs): block -> (job, block of the job).
// The scalar (PReLU slope) partials of ALL jobs are summed by one extra block: its four waves take a job each (and loop
// when there are more), every wave forming its job's total exactly as one wave used to (stride 64 over the partials,
// then the shuffle tree); the totals meet in LDS and ONE thread adds them to their destinations job after job, so jobs
// that share a slope parameter still add to it in a fixed order.  The extra block is block 0, the first one dispatched:
// what is left of its chain of memory latencies runs under the body blocks.  (As the LAST block, with one wave walking
// the jobs one after the other, it set the duration of the whole launch: 71 us against 30 us without it,
// tools/reduce_bench.py.)
// 24 jobs of 144 bytes stay inside the 4 KB of kernel arguments.
constexpr int kJobsPerLaunch = 24;
struct RedJobK {
  const float* part;
  int64_t pstride;
  RedSeg s0, s1, s2;
  const double* spart;
  float* sout;
  int32_t nparts, ns, blk0;  // blk0: first block of this job in the launch
};
struct RedJobsK {
  RedJobK j[kJobsPerLaunch];
  int32_t n, sblk;  // sblk: 1 when block 0 is the scalar block (the body blocks follow it), else 0
};
static_assert(sizeof(RedJobsK) <= 4096, "the job table is passed by value: kernel arguments are limited to 4 KB");
static_assert(sizeof(RedSeg) == 32, "gcl_reduce_seg (gcl.h) is the kernels' segment: three of them in the 144 bytes of a job");
__global__ __launch_bounds__(256) void reduce_jobs_kernel(RedJobsK J) {
  const int blk = (int)blockIdx.x - J.sblk;
  if (blk < 0) {  // the extra block: scalar partials
    __shared__ double tot[kJobsPerLaunch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < J.n; q += 4) {  // uniform per wave
      if (!J.j[q].spart) continue;
      // a lane's partials are LOADED twelve at a time (one memory latency for up to 768 of them, not one per partial:
      // under the body blocks' traffic a dependent load takes over a microsecond) and added in the same order
      const double* sp = J.j[q].spart;
      const int ns = J.j[q].ns;
      double t = 0.0;
      for (int base = lane; base < ns; base += 64 * 12) {
        double v[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = (base + 64 * k < ns) ? sp[base + 64 * k] : 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (base + 64 * k < ns) t += v[k];
      }
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0) tot[q] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int q = 0; q < J.n; ++q)  // in job order
        if (J.j[q].spart) *J.j[q].sout += (float)tot[q];
    return;
  }
  int q = 0;
  while (q + 1 < J.n && blk >= J.j[q + 1].blk0) ++q;  // uniform
  const RedJobK& jb = J.j[q];
  reduce4_block(jb.part, jb.nparts, jb.pstride, jb.s0, jb.s1, jb.s2, blk - jb.blk0);
}

}  // namespace

namespace gcl {
int launch_reduce_parts(const float* part, int nparts, int64_t pstride, int pld, float* out, int ldo, int R, int C,
                        int accumulate, hipStream_t st) {
  // one segment of the 16-way reducer: R rows of pld (padded) columns, C of them valid
  RedSeg s0{out, 0, R * pld, pld, C, ldo, accumulate};
  RedSeg none{nullptr, 0, 0, 1, 0, 0, 0};
  launch_reduce_multi(part, nparts, pstride, s0, none, none, st);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
int launch_reduce_parts2(const float* part, int nparts, int64_t pstride, int pld, int off1, float* out0, float* out1,
                         int C, int accumulate, hipStream_t st) {
  RedSeg s0{out0, 0, pld, pld, C, C, accumulate};
  RedSeg s1{out1, off1, pld, pld, C, C, accumulate};
  RedSeg none{nullptr, 0, 0, 1, 0, 0, 0};
  launch_reduce_multi(part, nparts, pstride, s0, s1, none, st);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
// three vectors of one partial record (each padded to pld entries, back to back), each with its own accumulate flag
int launch_reduce_parts3(const float* part, int nparts, int64_t pstride, int pld, float* out0, int acc0, float* out1,
                         int acc1, float* out2, int acc2, int C, hipStream_t st) {
  RedSeg s0{out0, 0, pld, pld, C, C, acc0};
  RedSeg s1{out1, pld, pld, pld, C, C, acc1};
  RedSeg s2{out2, 2 * pld, pld, pld, C, C, acc2};
  launch_reduce_multi(part, nparts, pstride, s0, s1, s2, st);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
}  // namespace gcl

namespace {

int gcl_ablate() {  // GCL_ABLATE: timing-only experiments (tools/ablate.sh) - honoured by the diagnostic build only
#ifndef GCL_STAMPS
  return 0;  // the product library never turns stores / MFMA / loads off, whatever the environment says
#endif
  static const int v = gcl::env_int("GCL_ABLATE", 0);
  return v;
}

// this translation unit's reader of the switches (dense_plan.h): the cached ones here, the per-call ones on first use
DenseSwitches switches() {
  static const bool valu = gcl::env_is("GCL_LINEAR_IMPL", "valu");
  static const int gt_mi = gcl::env_int("GCL_GT_MI", 0);
  DenseSwitches sw;
  sw.valu = valu; sw.gt_mi = gt_mi;
  return sw;
}

template <int EPI>
int launch_valu(const float* X, int64_t ldx, const float* in_slope, const float* W, int ldw, int trans, const float* bias,
                float* Y, int64_t ldy, int64_t rows, int K, int N, const float* Z, int64_t ldz, const float* z_slope,
                double* slope_part, int* nparts, hipStream_t st, int akind) {
  const int grid = (int)gcl::grid_for(rows * N, kValuGridCap);
  hipLaunchKernelGGL((linear_valu_kernel<EPI>), dim3(grid), dim3(256), 0, st, X, ldx, in_slope, W, ldw, trans, bias, Y,
                     ldy, rows, K, N, Z, ldz, z_slope, slope_part, akind);
  GCL_CHECK_LAUNCH();
  if (nparts) *nparts = grid;
  return GCL_OK;
}

template <int EPI>
int launch_linear(const PanelPlan& g, const float* X, int64_t ldx, const float* in_slope, const float* W, int ldw,
                  int trans, const float* bias, float* Y, int64_t ldy, int64_t rows, int K, int N, const float* Z,
                  int64_t ldz, const float* z_slope, double* slope_part, int* nparts, hipStream_t st, int akind) {
  GCL_CHECK_ARG(g.range_ok, "linear: unsupported K=%d N=%d (K<=256, N<=256)", K, N);
  GCL_CHECK_ARG(g.vec_ok, "linear: K=%d > 128 needs 16-B aligned rows (ld %% 4 == 0)", K);
  GCL_CHECK_ARG(g.valid(), "linear: K=%d N=%d needs %zu B of LDS (>160 KiB)", K, N, g.lds);
  // <KT, VEC>: (64, t) (64, f) (128, t) (128, f) (256, t) - K > 128 has 16-byte rows (vec_ok)
  const int rc = pick<1, 2, 4, 8>(g.NS, [&](auto NS) {
    return pick<0, 1, 2, 3, 4>(g.KT == 256 ? 4 : (g.KT == 128 ? 2 : 0) + (g.vec ? 0 : 1), [&](auto KV) {
      constexpr int kv = decltype(KV)::value;
      auto kern = linear_mfma_kernel<decltype(NS)::value, EPI, kv == 4 ? 256 : kv >= 2 ? 128 : 64, kv == 4 || !(kv & 1)>;
      GCL_ENSURE_DYN_LDS(kern, gcl::kLdsBytes);
      hipLaunchKernelGGL(kern, dim3(g.grid), dim3(g.waves * 64), g.lds, st, X, ldx, in_slope, W, ldw, trans, bias, Y, ldy,
                         rows, K, N, Z, ldz, z_slope, slope_part, akind, gcl_ablate());
      return (int)GCL_OK;
    });
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  if (nparts) *nparts = g.grid;
  return GCL_OK;
}

template <int EPI>
int launch_gemm(const DensePlan& p, const float* X, int64_t ldx, int akind, const float* slope, const float* W, int64_t ldw,
                const float* bias, float* Y, int64_t ldy, int64_t rows, int K, int N, const float* Z, int64_t ldz,
                const float* add, int64_t ldadd, double* slope_part, int* nparts, hipStream_t st) {
  const TilePlan& g = p.tile;
  GCL_CHECK_ARG((K % 4 == 0) && (ldx % 4 == 0) && gcl::aligned16(X), "dense: wide shapes need K %% 4 == 0 and 16-B aligned rows (K=%d ldx=%lld)", K, (long long)ldx);
  GCL_CHECK_ARG((ldw % 4 == 0) && gcl::aligned16(W) && (!p.trans || N % 4 == 0), "dense: wide shapes need a 16-B aligned weight block (ldw=%lld N=%d)", (long long)ldw, N);
  auto go = [&](auto kern) {
    GCL_ENSURE_DYN_LDS(kern, gcl::kLdsBytes);
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), p.tile_lds, st, X, ldx, akind, slope, W, ldw, bias, Y, ldy, rows, K, N,
                       Z, ldz, add, ldadd, slope_part, g.nt, g.total, g.per_xcd);
    return (int)GCL_OK;
  };
  const int rc = p.form == DenseForm::kTileX3 ? go(gemm_tile_x3_kernel<EPI>) : pick<0, 1>(p.trans, [&](auto T) {
    return pick<1, 2>(g.mi, [&](auto MI) { return go(gemm_tile_kernel<EPI, decltype(T)::value != 0, decltype(MI)::value>); });
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  if (nparts) *nparts = (int)g.grid;
  return GCL_OK;
}

}  // namespace

extern "C" size_t gcl_colsum_ws_bytes(int64_t, int32_t);
extern "C" int gcl_colsum(const float*, int64_t, int64_t, int32_t, float*, int32_t, void*, size_t, gcl_stream_t);

static int check_act(const char* who, int act, const float* slope) {
  GCL_CHECK_ARG(act == GCL_ACT_NONE || act == GCL_ACT_PRELU || act == GCL_ACT_SILU, "%s: unknown activation %d", who, act);
  GCL_CHECK_ARG(act != GCL_ACT_PRELU || slope, "%s: GCL_ACT_PRELU needs the slope pointer", who);
  return GCL_OK;
}

extern "C" int gcl_dense_fwd(const float* x, int64_t ldx, int32_t act, const float* slope, const float* W, int64_t ldw,
                             const float* bias, const float* addend, int64_t ldadd, float* y, int64_t ldy,
                             int64_t rows, int32_t Fin, int32_t Fout, gcl_stream_t stream) {
  GCL_CHECK_ARG(x && W && y, "dense_fwd: null argument");
  GCL_CHECK_ARG(rows >= 0 && Fin >= 1 && Fout >= 1 && ldx >= Fin && ldy >= Fout && ldw >= Fin && (!addend || ldadd >= Fout),
                "dense_fwd: bad shape rows=%lld ldx=%lld ldy=%lld ldw=%lld", (long long)rows, (long long)ldx,
                (long long)ldy, (long long)ldw);
  if (int rc = check_act("dense_fwd", act, slope)) return rc;
  const DenseCall c{rows, Fin, Fout, !addend && ldw == Fin, (Fin % 4 == 0) && (ldx % 4 == 0) && gcl::aligned16(x),
                    (ldw % 4 == 0) && gcl::aligned16(W)};
  const DensePlan p = plan_dense_fwd(c, ldx, ldy, gcl::aligned16(x), gcl::aligned16(y), act, switches());
  hipStream_t st = (hipStream_t)stream;
  const float* sl = act == GCL_ACT_PRELU ? slope : nullptr;
  if (rows == 0) return GCL_OK;
  switch (p.form) {
    case DenseForm::kX3: return gcl::x3_linear_fwd(p.x3, x, ldx, act, sl, W, bias, y, ldy, rows, Fin, Fout, st);
    case DenseForm::kValu:
      return launch_valu<EPI_BIAS>(x, ldx, sl, W, Fin, 0, bias, y, ldy, rows, Fin, Fout, nullptr, 0, nullptr, nullptr, nullptr, st, act);
    case DenseForm::kPanel:
      return launch_linear<EPI_BIAS>(p.panel, x, ldx, sl, W, Fin, 0, bias, y, ldy, rows, Fin, Fout, nullptr, 0, nullptr, nullptr,
                                     nullptr, st, act);
    default:
      return launch_gemm<EPI_BIAS>(p, x, ldx, act, sl, W, ldw, bias, y, ldy, rows, Fin, Fout, nullptr, 0, addend, ldadd, nullptr,
                                   nullptr, st);
  }
}

extern "C" int gcl_linear_fwd(const float* x, int64_t ldx, const float* in_slope, const float* W, const float* bias,
                              float* y, int64_t ldy, int64_t rows, int32_t Fin, int32_t Fout, gcl_stream_t stream) {
  return gcl_dense_fwd(x, ldx, in_slope ? GCL_ACT_PRELU : GCL_ACT_NONE, in_slope, W, Fin, bias, nullptr, 0, y, ldy, rows,
                       Fin, Fout, stream);
}

extern "C" size_t gcl_linear_bwd_ws_bytes(int64_t rows, int32_t Fin, int32_t Fout) {
  return dense_bwd_ws_bytes(rows, Fin, Fout, switches());
}

extern "C" int gcl_dense_bwd_dx(const float* dy, int64_t lddy, const float* W, int64_t ldw, const float* z, int64_t ldz,
                                int32_t act, const float* slope, float* d_slope, const float* addend, int64_t ldadd,
                                float* dx, int64_t lddx, int64_t rows, int32_t Fin, int32_t Fout, void* ws,
                                size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(dy && W && dx, "dense_bwd_dx: null argument");
  GCL_CHECK_ARG(lddy >= Fout && lddx >= Fin && ldw >= Fin && (!addend || ldadd >= Fin), "dense_bwd_dx: leading dimension too small");
  if (int rc = check_act("dense_bwd_dx", act, slope)) return rc;
  GCL_CHECK_ARG(act == GCL_ACT_NONE || (z && ldz >= Fin), "dense_bwd_dx: activation given without its pre-activation z");
  hipStream_t st = (hipStream_t)stream;
  const float* sl = act == GCL_ACT_PRELU ? slope : nullptr;
  const DenseCall c{rows, Fout, Fin, !addend && ldw == Fin, (Fout % 4 == 0) && (lddy % 4 == 0) && gcl::aligned16(dy),
                    (ldw % 4 == 0) && gcl::aligned16(W)};
  const DensePlan p = plan_dense_bwd_dx(c, ws ? ws_bytes : 0, gcl::aligned16(ws), switches());
  double* slope_part = nullptr;
  if (sl && d_slope) {
    GCL_CHECK_ARG(ws && ws_bytes >= p.slope_cap * sizeof(double) && gcl::aligned16(ws), "dense_bwd_dx: workspace too small");
    slope_part = (double*)ws;
  }
  if (rows == 0) return GCL_OK;
  int nparts = 0, rc;
  const float* zz = act == GCL_ACT_NONE ? nullptr : z;
  if (p.form == DenseForm::kValu) {
    rc = launch_valu<EPI_DX>(dy, lddy, nullptr, W, Fin, 1, nullptr, dx, lddx, rows, Fout, Fin, zz, ldz, sl, slope_part, &nparts, st, act);
  } else if (p.form == DenseForm::kPanel) {
    rc = launch_linear<EPI_DX>(p.panel, dy, lddy, nullptr, W, Fin, 1, nullptr, dx, lddx, rows, Fout, Fin, zz, ldz, sl, slope_part,
                               &nparts, st, act);
  } else if (p.transpose_first) {
    float* Wt = reinterpret_cast<float*>(static_cast<char*>(ws) + p.wt_off_bytes);
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)gcl::cdiv(Fin, 32), (unsigned)gcl::cdiv(Fout, 32)), dim3(256), 0, st,
                       W, ldw, Wt, Fout, Fin);
    rc = launch_gemm<EPI_DX>(p, dy, lddy, act, sl, Wt, Fout, nullptr, dx, lddx, rows, Fout, Fin, zz, ldz, addend, ldadd,
                             slope_part, &nparts, st);
  } else {
    rc = launch_gemm<EPI_DX>(p, dy, lddy, act, sl, W, ldw, nullptr, dx, lddx, rows, Fout, Fin, zz, ldz, addend, ldadd,
                             slope_part, &nparts, st);
  }
  if (rc) return rc;
  if (slope_part && nparts > 0) {
    hipLaunchKernelGGL(reduce_scalar_kernel, dim3(1), dim3(64), 0, st, slope_part, nparts, d_slope);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}

extern "C" int gcl_linear_bwd_dx(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                                 const float* in_slope, float* d_in_slope, float* dx, int64_t lddx, int64_t rows,
                                 int32_t Fin, int32_t Fout, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(!in_slope || (x && ldx >= Fin), "linear_bwd_dx: in_slope given without the forward input x");
  return gcl_dense_bwd_dx(dy, lddy, W, Fin, in_slope ? x : nullptr, ldx, in_slope ? GCL_ACT_PRELU : GCL_ACT_NONE,
                          in_slope, d_in_slope, nullptr, 0, dx, lddx, rows, Fin, Fout, ws, ws_bytes, stream);
}

// dW for <= 256 outputs and any number of inputs: ONE launch whose grid.y walks the 128-column input
// chunks (dY is re-read once per chunk), then one partial reduction per chunk
static int dw_block(const float* dy, int64_t lddy, const float* x, int64_t ldx, int akind, const float* in_slope,
                    float* dW, int64_t lddw, float* db, int64_t rows, int32_t Fin, int32_t Fout, int32_t accumulate,
                    void* ws, hipStream_t st, gcl_reduce_job* job = nullptr) {
  const DwPlan p = plan_dw(rows, Fin, Fout, (lddy % 4 == 0) && (ldx % 4 == 0) && gcl::aligned16(dy) && gcl::aligned16(x));
  float* part = (float*)ws + p.part_off;
  float* dbpart = (float*)ws + p.dbpart_off;
  int rc = pick<1, 2, 4, 8>(p.NO, [&](auto NO) {
    return pick<1, 2, 3, 4>(p.NC, [&](auto NC) {
      return pick<0, 1>(p.vec, [&](auto V) {
        auto kern = dw_mfma_kernel<decltype(NO)::value, decltype(NC)::value, decltype(V)::value != 0>;
        GCL_ENSURE_DYN_LDS(kern, gcl::kLdsBytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)p.nblk, (unsigned)p.nct), dim3(256), p.lds, st, dy, lddy, x, ldx, in_slope, part,
                           db ? dbpart : nullptr, rows, Fin, Fout, p.rpb, akind, p.tile_stride);
        return (int)GCL_OK;
      });
    });
  });
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  // input chunk c: its records start c * tile_stride floats into `part`
  auto chunk = [&](int c) {
    return RedSeg{dW + c * 128, (int32_t)(c * p.tile_stride), Fout * p.FinP, p.FinP, std::min(Fin - c * 128, 128), (int32_t)lddw,
                  accumulate ? 1 : 0};
  };
  // deferred (job[0]: the dW tiles, job[1]: db - they are two partial buffers): only when the immediate passes below
  // are ONE launch for dW and both take the 16-byte reducer, which is the only one the queue has
  if (job && p.may_defer && gcl::aligned16(part) && gcl::aligned16(dbpart)) {
    job[0].part = part;
    job[0].pstride = p.rec;
    job[0].nparts = (int32_t)p.nblk;
    for (int c = 0; c < p.nct; ++c) job[0].seg[c] = chunk(c);
    if (db) {
      job[1].part = dbpart;
      job[1].pstride = p.FoutP;
      job[1].nparts = (int32_t)p.nblk;
      job[1].seg[0] = RedSeg{db, 0, p.FoutP, p.FoutP, Fout, Fout, accumulate ? 1 : 0};
    }
    return GCL_OK;
  }
  // final pass: the input chunks of a wide layer three to a launch (one segment each) - a 256-wide layer used to end
  // in two of these launches per call
  const RedSeg none{nullptr, 0, 0, 1, 0, 0, 0};
  for (int ct = 0; ct < p.nct; ct += 3) {
    RedSeg seg[3] = {none, none, none};
    for (int q = 0; q < 3 && ct + q < p.nct; ++q) {
      GCL_CHECK_ARG(below_2_31((ct + q) * p.tile_stride), "dense_bwd_dw: partial workspace offset overflows");
      seg[q] = chunk(ct + q);
    }
    launch_reduce_multi(part, (int)p.nblk, p.rec, seg[0], seg[1], seg[2], st);
    GCL_CHECK_LAUNCH();
  }
  if (db) return gcl::launch_reduce_parts(dbpart, (int)p.nblk, (int64_t)p.FoutP, p.FoutP, db, Fout, 1, Fout, accumulate, st);
  return GCL_OK;
}

static int dense_bwd_dw_impl(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t act,
                             const float* slope, float* dW, int64_t lddw, float* db, int64_t rows, int32_t Fin,
                             int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream,
                             gcl_reduce_job* job) {
  if (job) memset(job, 0, 2 * sizeof(*job));
  if (Fout > 256) job = nullptr;  // several launches share the workspace: each reduces on the spot
  GCL_CHECK_ARG(dy && x && dW, "dense_bwd_dw: null argument");
  GCL_CHECK_ARG(lddy >= Fout && ldx >= Fin && lddw >= Fin, "dense_bwd_dw: leading dimension too small");
  GCL_CHECK_ARG(Fin >= 1 && Fout >= 1, "dense_bwd_dw: bad shape");
  GCL_CHECK_ARG(lddw < (1 << 30), "dense_bwd_dw: lddw too large");
  if (int rc = check_act("dense_bwd_dw", act, slope)) return rc;
  GCL_CHECK_ARG(ws && ws_bytes >= gcl_linear_bwd_ws_bytes(rows, Fin, Fout), "dense_bwd_dw: workspace too small");
  const float* sl = act == GCL_ACT_PRELU ? slope : nullptr;
  // wide layers: <= 256 outputs per launch, every 128-column input chunk inside it (grid.y)
  for (int o0 = 0; o0 < Fout; o0 += 256) {
    const int fo = Fout - o0 < 256 ? Fout - o0 : 256;
    int rc = dw_block(dy + o0, lddy, x, ldx, act, sl, dW + (int64_t)o0 * lddw, lddw, db ? db + o0 : nullptr, rows, Fin,
                      fo, accumulate, ws, (hipStream_t)stream, job);
    if (rc) return rc;
  }
  return GCL_OK;
}

extern "C" int gcl_dense_bwd_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t act,
                                const float* slope, float* dW, int64_t lddw, float* db, int64_t rows, int32_t Fin,
                                int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  return dense_bwd_dw_impl(dy, lddy, x, ldx, act, slope, dW, lddw, db, rows, Fin, Fout, accumulate, ws, ws_bytes, stream,
                           nullptr);
}

extern "C" int gcl_dense_bwd_dw_deferred(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t act,
                                         const float* slope, float* dW, int64_t lddw, float* db, int64_t rows,
                                         int32_t Fin, int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes,
                                         gcl_stream_t stream, gcl_reduce_job* job) {
  GCL_CHECK_ARG(job, "dense_bwd_dw_deferred: null job");
  return dense_bwd_dw_impl(dy, lddy, x, ldx, act, slope, dW, lddw, db, rows, Fin, Fout, accumulate, ws, ws_bytes, stream,
                           job);
}

extern "C" int gcl_linear_bwd_dw_deferred(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                                          const float* in_slope, float* dW, float* db, int64_t rows, int32_t Fin,
                                          int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes,
                                          gcl_stream_t stream, gcl_reduce_job* job) {
  GCL_CHECK_ARG(job, "linear_bwd_dw_deferred: null job");
  return dense_bwd_dw_impl(dy, lddy, x, ldx, in_slope ? GCL_ACT_PRELU : GCL_ACT_NONE, in_slope, dW, Fin, db, rows, Fin, Fout,
                           accumulate, ws, ws_bytes, stream, job);
}

extern "C" int gcl_linear_bwd_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* in_slope,
                                 float* dW, float* db, int64_t rows, int32_t Fin, int32_t Fout, int32_t accumulate,
                                 void* ws, size_t ws_bytes, gcl_stream_t stream) {
  return gcl_dense_bwd_dw(dy, lddy, x, ldx, in_slope ? GCL_ACT_PRELU : GCL_ACT_NONE, in_slope, dW, Fin, db, rows, Fin,
                          Fout, accumulate, ws, ws_bytes, stream);
}

// the fused form's records, or what the separate kernels (dW + dx, then the column sums) need of the same buffer
extern "C" size_t gcl_linear_bwd_all_ws_bytes(int64_t rows, int32_t Fin, int32_t Fout) {
  return std::max({fused_layout(Fin, Fout).bytes, gcl_linear_bwd_ws_bytes(rows, Fin, Fout), gcl_colsum_ws_bytes(rows, Fin)});
}

static int bwd_all_impl(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                        const float* in_slope, float* d_in_slope, float* dx, int64_t lddx, float* dW,
                        float* db, float* colsum_dx, int64_t rows, int32_t Fin, int32_t Fout,
                        int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream, gcl_reduce_job* job) {
  if (job) memset(job, 0, sizeof(*job));
  GCL_CHECK_ARG(dy && W && x && dx && dW, "linear_bwd_all: null argument");
  GCL_CHECK_ARG(ws && ws_bytes >= gcl_linear_bwd_all_ws_bytes(rows, Fin, Fout), "linear_bwd_all: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  // every destination has its own accumulate bit: dW, db and colsum_dx usually belong to DIFFERENT
  // parameters (colsum_dx is the bias gradient of the layer below) with different .grad states
  const int acc_dw = (accumulate & GCL_ACC_DW) ? 1 : 0, acc_db = (accumulate & GCL_ACC_DB) ? 1 : 0,
            acc_cs = (accumulate & GCL_ACC_COLSUM) ? 1 : 0;
  const BwdAllCall c{rows, lddy, ldx, lddx, Fin, Fout, gcl::aligned16(dy), gcl::aligned16(x), gcl::aligned16(dx), dx != nullptr,
                     in_slope != nullptr, db != nullptr, colsum_dx != nullptr};
  const BwdAllPlan p = plan_bwd_all(c, switches());
  if (p.form == BwdAllForm::kSeparate) {
    int rc;
    if (db && acc_db != acc_dw) {  // separate kernels share one flag between dW and db: split the call
      rc = gcl_linear_bwd_dw(dy, lddy, x, ldx, in_slope, dW, nullptr, rows, Fin, Fout, acc_dw, ws, ws_bytes, stream);
      if (rc) return rc;
      rc = gcl_colsum(dy, lddy, rows, Fout, db, acc_db, ws, ws_bytes, stream);
    } else {
      rc = gcl_linear_bwd_dw(dy, lddy, x, ldx, in_slope, dW, db, rows, Fin, Fout, acc_dw, ws, ws_bytes, stream);
    }
    if (rc) return rc;
    rc = gcl_linear_bwd_dx(dy, lddy, W, in_slope ? x : nullptr, ldx, in_slope, d_in_slope, dx, lddx, rows, Fin, Fout,
                           ws, ws_bytes, stream);
    if (rc) return rc;
    if (colsum_dx) rc = gcl_colsum(dx, lddx, rows, Fin, colsum_dx, acc_cs, ws, ws_bytes, stream);
    return rc;  // (nothing deferred: job stays empty)
  }
  float* part_dw = (float*)ws;
  float* part_db = db ? part_dw + p.db_off : nullptr;
  float* part_cs = colsum_dx ? part_dw + p.cs_off : nullptr;
  const bool want_slope = in_slope && d_in_slope;
  double* part_sl = want_slope ? (double*)(((uintptr_t)ws + p.slope_off_bytes + 15) & ~(uintptr_t)15) : nullptr;
  auto go = [&](auto kern, bool raise_lds) {
    if (raise_lds) GCL_ENSURE_DYN_LDS(kern, gcl::kLdsBytes);
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(256), p.lds, st, dy, lddy, W, x, ldx, in_slope, dx, lddx, rows, Fin, Fout, part_dw,
                       part_db, part_cs, part_sl);
    return (int)GCL_OK;
  };
  int rc;
  if (p.form == BwdAllForm::kFused128)
    rc = pick<1, 2>(p.NO, [&](auto NO) {
      return pick<1, 2, 3>(p.NC, [&](auto NC) { return go(linear_bwd_fused_kernel<decltype(NO)::value, decltype(NC)::value>, true); });
    });
  else if (p.form == BwdAllForm::kFused64)
    rc = pick<1, 2>(p.NO, [&](auto NO) { return go(linear_bwd_fused64_kernel<decltype(NO)::value>, false); });  // 50 KB: below the default limit
  else
    rc = gcl::x3_linear_bwd(p, dy, lddy, W, x, ldx, in_slope, dx, lddx, rows, Fin, Fout, part_dw, part_db, part_cs, part_sl, st);
  if (rc) return rc;
  GCL_CHECK_LAUNCH();
  // one launch reduces the three parts of the records
  RedSeg s0{dW, 0, Fout * p.FiP, p.FiP, Fin, Fin, acc_dw};
  RedSeg s1{db, p.db_off, db ? Fout : 0, p.FoP, Fout, 0, acc_db};
  RedSeg s2{colsum_dx, p.cs_off, colsum_dx ? Fin : 0, p.FiP, Fin, 0, acc_cs};
  if (job) {
    // deferred: describe the final pass instead of launching it.  db / colsum segments are widened to their padded
    // lengths (cols still limits what is written) so that every job takes the 16-byte reducer.
    s1.count = db ? p.FoP : 0;
    s2.count = colsum_dx ? p.FiP : 0;
    job->part = part_dw;
    job->nparts = p.nblk;
    job->pstride = p.rec;
    job->seg[0] = s0; job->seg[1] = s1; job->seg[2] = s2;
    job->spart = part_sl;
    job->ns = want_slope ? p.nblk : 0;
    job->sout = want_slope ? d_in_slope : nullptr;
    return GCL_OK;
  }
  // + the slope partials (one extra block of the same launch)
  launch_reduce_multi(part_dw, p.nblk, p.rec, s0, s1, s2, st, part_sl, p.nblk, d_in_slope);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_linear_bwd_all(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                                  const float* in_slope, float* d_in_slope, float* dx, int64_t lddx, float* dW,
                                  float* db, float* colsum_dx, int64_t rows, int32_t Fin, int32_t Fout,
                                  int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  return bwd_all_impl(dy, lddy, W, x, ldx, in_slope, d_in_slope, dx, lddx, dW, db, colsum_dx, rows, Fin, Fout,
                      accumulate, ws, ws_bytes, stream, nullptr);
}

extern "C" int gcl_linear_bwd_all_deferred(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                                           const float* in_slope, float* d_in_slope, float* dx, int64_t lddx,
                                           float* dW, float* db, float* colsum_dx, int64_t rows, int32_t Fin,
                                           int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes,
                                           gcl_stream_t stream, gcl_reduce_job* job) {
  GCL_CHECK_ARG(job, "linear_bwd_all_deferred: null job");
  return bwd_all_impl(dy, lddy, W, x, ldx, in_slope, d_in_slope, dx, lddx, dW, db, colsum_dx, rows, Fin, Fout,
                      accumulate, ws, ws_bytes, stream, job);
}

extern "C" int gcl_reduce_jobs(const gcl_reduce_job* jobs, int32_t n, gcl_stream_t stream) {
  GCL_CHECK_ARG(n >= 0 && (jobs || n == 0), "reduce_jobs: null argument");
  hipStream_t st = (hipStream_t)stream;
  // the running index is carried ACROSS launches: skipped (empty) jobs do not count towards the 24 of a launch, so
  // restarting at base + 24 would reduce the jobs behind a skipped one twice
  for (int32_t q = 0; q < n;) {
    RedJobsK J;
    memset(&J, 0, sizeof(J));
    int nb = 0, cnt = 0;
    bool any_slope = false;
    for (; q < n && cnt < kJobsPerLaunch; ++q) {
      const gcl_reduce_job& g = jobs[q];
      if (g.nparts <= 0) continue;  // that call reduced on the spot
      GCL_CHECK_ARG(g.part && g.pstride % 4 == 0 && gcl::aligned16(g.part), "reduce_jobs: bad partial buffer");
      RedJobK& k = J.j[cnt];
      k.part = g.part;
      k.pstride = g.pstride;
      RedSeg* ss[3] = {&k.s0, &k.s1, &k.s2};
      int total = 0;
      for (int t = 0; t < 3; ++t) {
        GCL_CHECK_ARG((g.seg[t].poff | g.seg[t].count) % 4 == 0, "reduce_jobs: segment not 16-byte granular");
        *ss[t] = g.seg[t];
        if (!ss[t]->out) ss[t]->count = 0;   // unused segment
        if (ss[t]->pld <= 0) ss[t]->pld = 1;  // (a zeroed job: the kernel divides by it)
        total += ss[t]->count;
      }
      k.spart = g.spart;
      k.sout = g.sout;
      k.nparts = g.nparts;
      k.ns = g.ns;
      k.blk0 = nb;
      any_slope = any_slope || (g.spart && g.sout && g.ns > 0);
      if (!(g.spart && g.sout && g.ns > 0)) k.spart = nullptr;
      nb += (int)gcl::cdiv(total, 32);
      ++cnt;
    }
    if (cnt == 0) continue;
    J.n = cnt;
    J.sblk = any_slope ? 1 : 0;
    hipLaunchKernelGGL(reduce_jobs_kernel, dim3((unsigned)nb + (any_slope ? 1u : 0u)), dim3(256), 0, st, J);
    GCL_CHECK_LAUNCH();
  }
  return GCL_OK;
}
