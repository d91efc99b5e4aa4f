// Shared helpers for libgcl_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/gcl.h"

namespace gcl {

void set_error(const char* fmt, ...);

#define GCL_CHECK_ARG(cond, ...)        \
  do {                                  \
    if (!(cond)) {                      \
      gcl::set_error(__VA_ARGS__);      \
      return GCL_EINVAL;                \
    }                                   \
  } while (0)

#define GCL_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      gcl::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return GCL_EHIP;                                                                   \
    }                                                                                    \
  } while (0)

#define GCL_CHECK_LAUNCH()                                                     \
  do {                                                                         \
    hipError_t _e = hipGetLastError();                                         \
    if (_e != hipSuccess) {                                                    \
      gcl::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
      return GCL_EHIP;                                                         \
    }                                                                          \
  } while (0)

// Raise the dynamic-LDS limit of kernel `kern` to `bytes` (gcl::ensure_dyn_lds); on failure, return its error code.
#define GCL_ENSURE_DYN_LDS(kern, bytes)                                   \
  do {                                                                    \
    const int _rc = gcl::ensure_dyn_lds((const void*)(kern), (bytes));    \
    if (_rc) return _rc;                                                  \
  } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// blocks of 256 threads for `total` items, at most `cap` of them (grid-stride loops beyond)
inline unsigned grid_for(int64_t total, int cap = 4096) {
  int64_t nb = cdiv(total > 0 ? total : 1, 256);
  return (unsigned)(nb > cap ? cap : nb);
}

// Environment switches: an integer (`dflt` when unset), and whether a string switch is set to `value`.  Each call
// site decides when it reads its switch (once per process in a function-local static, per graph or per call).
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline bool env_is(const char* name, const char* value) {
  const char* e = getenv(name);
  return e && strcmp(e, value) == 0;
}

namespace plan {
// Run-time value -> template constant: calls f(std::integral_constant<int, V>) for the V of Vs... equal to v.
template <int... Vs, class F>
int pick(int v, F&& f) {
  int rc = GCL_EINVAL;
  if (!((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...)) set_error("dispatch: no kernel for %d", v);
  return rc;
}
}  // namespace plan

constexpr int kWave = 64;     // CDNA wavefront
constexpr int kNumXCD = 8;    // MI355X: 8 XCDs, blocks are dealt round-robin over them
constexpr int kNumCU = 256;
constexpr int kLdsBytes = 160 * 1024;  // LDS of one CU
constexpr int kEll = 8;      // stride of the ELL prefix arrays
constexpr int kHeavy = 64;   // rows with more edges than this get a whole block
constexpr int kHaloRec = 16;             // edge records per row held in registers (one per lane of a 16-lane row group)
constexpr int kHaloMore = 1 << 17;       // flag in slot 15: the row has more than 16 edges (finish from the CSR arrays)
constexpr int kHaloSkip = 1 << 16;       // flag in slot 15: heavy row, done by agg_heavy_kernel (do not store)
constexpr int kHaloPosMask = 0xFFFF;

__device__ __forceinline__ float prelu_f(float x, float a) { return x > 0.f ? x : a * x; }
// Activation kinds of the dense kernels (GCL_ACT_* of gcl.h).  SiLU: x * sigmoid(x).
constexpr int kActNone = 0, kActPrelu = 1, kActSilu = 2;
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
__device__ __forceinline__ float act_f(float x, float a, int kind) { return kind == kActSilu ? silu_f(x) : prelu_f(x, a); }
// d act(z) / dz
__device__ __forceinline__ float dsilu_f(float z) {
  const float s = sigmoid_f(z);
  return s * (1.f + z * (1.f - s));
}

// Exact rounding: a value passed through here is opaque to the optimiser (an empty asm volatile), so a product is
// rounded on its own and cannot be contracted into the add that follows.  hipcc builds with -ffp-contract=fast, which
// fuses even through __fmul_rn / __dmul_rn and ignores `#pragma clang fp contract`.  This is what keeps the kernels
// that promise torch's CPU results bit for bit (nudging, regrid, blend, MOS) and the two Adam steps in agreement.
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ double rounded(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The float64 bilinear value of a cell: src[n00], src[n00 + 1], src[n00 + nlat], src[n00 + nlat + 1] (rows of ld
// elements) times w[0 .. 3], every product rounded on its own and added left to right - scipy's order of the four
// corners.  The FIRST PRODUCT STARTS THE SUM, so four -0.0 corners give -0.0.  The position-form kernels (live, wrf,
// multires, downscale) start from acc = 0.0 instead, where 0.0 + (-0.0) is +0.0: the two forms are not interchangeable.
template <typename T>
__device__ __forceinline__ double cell_corner_sum(const T* src, int64_t ld, int64_t n00, int32_t nlat, const double* w) {
  double acc = rounded((double)src[n00 * ld] * w[0]);
  acc = acc + rounded((double)src[(n00 + 1) * ld] * w[1]);
  acc = acc + rounded((double)src[(n00 + nlat) * ld] * w[2]);
  acc = acc + rounded((double)src[(n00 + nlat + 1) * ld] * w[3]);
  return acc;
}

// sum over the 64 lanes of a wave, in a fixed butterfly order (every lane gets the sum)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// Contiguous spans of fp16 values that start off a 16-byte boundary (the dataset and downscaler kernels stage a tile in
// LDS and move it with these).  kThreads is the block size of the calling kernel, which every thread of the block
// enters: the body is dealt over kThreads threads, the head goes to threads 0 .. 6 and the tail to threads 64 .. 70
// (another wave than the head's), so a block needs two waves.
// n halves from get(k) to dst, which may start anywhere: the 16-byte aligned body as 16-byte stores, the at most seven
// halves either side of it one by one.
template <int kThreads, class Get>
__device__ __forceinline__ void store_span(uint16_t* dst, int n, Get get) {
  static_assert(kThreads >= 128 && kThreads % 64 == 0, "store_span: whole waves, and the tail goes to the second");
  const int tid = threadIdx.x;
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 1);
  head = head < n ? head : n;
  const int nvec = (n - head) >> 3;
  for (int i = tid; i < nvec; i += kThreads) {
    const int k = head + 8 * i;
    union { uint4 q; uint16_t h[8]; } u;
#pragma unroll
    for (int m = 0; m < 8; ++m) u.h[m] = get(k + m);
    *reinterpret_cast<uint4*>(dst + k) = u.q;
  }
  const int done = head + 8 * nvec;
  if (tid < head) dst[tid] = get(tid);
  if (tid >= 64 && tid - 64 < n - done) dst[done + tid - 64] = get(done + tid - 64);
}

// n halves from src (any alignment) into lds[0 .. n), 16-byte loads over the aligned body
template <int kThreads>
__device__ __forceinline__ void load_span(const uint16_t* __restrict__ src, int n, uint16_t* lds) {
  static_assert(kThreads >= 128 && kThreads % 64 == 0, "load_span: whole waves, and the tail goes to the second");
  const int tid = threadIdx.x;
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 1);
  head = head < n ? head : n;
  const int nvec = (n - head) >> 3;
  for (int i = tid; i < nvec; i += kThreads) {
    const int k = head + 8 * i;
    union { uint4 q; uint16_t h[8]; } u;
    u.q = *reinterpret_cast<const uint4*>(src + k);
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[k + m] = u.h[m];
  }
  const int done = head + 8 * nvec;
  if (tid < head) lds[tid] = src[tid];
  if (tid >= 64 && tid - 64 < n - done) lds[done + tid - 64] = src[done + tid - 64];
}

// One element of torch.optim.Adam (no amsgrad, no maximize), src/main.py:212: the update of gcl_adam_step and
// gcl_adam_step_groups, written once so that both round identically.  hipcc may contract a product into the add that
// follows it, and does so differently in a scalar and a float4 loop; `rounded` pins every product so that no
// contraction depends on the loop shape.  The rounding is the one the scalar loop always had: every product and sum
// rounded on its own, the final `p - step * ratio` one fused multiply-add.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps,
                                          float wd, float bc1, float bc2_sqrt, float gscale) {
  float gi = rounded(g * gscale);
  if (wd != 0.f) gi += rounded(wd * p);
  const float mi = rounded(b1 * m) + rounded((1.f - b1) * gi);
  const float vi = rounded(b2 * v) + rounded(rounded((1.f - b2) * gi) * gi);
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = __builtin_fmaf(-(lr / bc1), mi / denom, p);
}

// out[i*ldo + j] (+)= sum_p part[p*pstride + i*pld + j], i < R, j < C (parallel over partials, fixed order)
int launch_reduce_parts(const float* part, int nparts, int64_t pstride, int pld, float* out, int ldo, int R, int C,
                        int accumulate, hipStream_t st);
// two vectors of one partial record in ONE launch: out0[j] (+)= sum_p part[p*pstride + j],
// out1[j] (+)= sum_p part[p*pstride + off1 + j], j < C (each vector padded to pld entries in the record)
int launch_reduce_parts2(const float* part, int nparts, int64_t pstride, int pld, int off1, float* out0, float* out1,
                         int C, int accumulate, hipStream_t st);

// Kernels that ask for more than 64 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised first.
// The attribute belongs to the (function, DEVICE) pair, so the "already done" record is kept per device: a process
// that drives several GPUs (or a later hipSetDevice) sets it again where it is still missing.
int ensure_dyn_lds(const void* func, size_t bytes);

int launch_reduce_parts3(const float* part, int nparts, int64_t pstride, int pld, float* out0, int acc0, float* out1,
                         int acc1, float* out2, int acc2, int C, hipStream_t st);

}  // namespace gcl

// Source-tile ("halo") layout of one CSR direction: the rows are cut into tiles of T consecutive rows and each
// tile carries the list of DISTINCT source rows its edges read, so a block stages every source once in LDS
// (LDS-DMA row gather) and forms the sums from LDS (csrc/aggregate.hip, agg_halo_kernel).  Built on the host
// when the graph is created, and only when the tiling shares sources well enough to pay (graph.hip).
struct gcl_halo {
  int32_t T = 0, ntiles = 0;
  int32_t smax = 0;          // rows of a tile image: T own rows + the largest halo count (rounded up to 8); row `smax` is the zero row
  int32_t* list = nullptr;   // [ntiles * (smax - T)] sources of a tile OUTSIDE the tile (its halo), ascending, padded by repeating the last
  int32_t* cnt = nullptr;    // [ntiles] halo entries to stage (multiple of 8)
  int32_t* rec = nullptr;    // [n * 16 * 2] {image position | flags (slot 15), weight bits} of the first 16 edges of a row
                             // (GCL_GRAPH_GAT, transposed direction: the edge's forward CSR slot instead of the weight)
  int32_t* opos = nullptr;   // [E'] image position of every CSR slot (rows with more than 16 edges)
};

// Device-side graph arrays (owned by the handle).
struct gcl_graph {
  int32_t n = 0;
  int64_t e = 0;  // E'
  int32_t kind = 0;
  int32_t max_in_deg = 0;
  int32_t max_out_deg = 0;
  int32_t *rowptr = nullptr, *col = nullptr, *eperm = nullptr;
  int32_t *trowptr = nullptr, *tcol = nullptr, *tslot = nullptr;
  float *w = nullptr, *tw = nullptr;
  // fixed-stride prefix of every row (first kEll edges in CSR order; padding: col = row, w = 0)
  int32_t *ecol = nullptr, *tecol = nullptr, *teslot = nullptr;  // teslot: forward slot of a transposed prefix edge
  float *ew = nullptr, *tew = nullptr;
  int32_t ell_width = 8, tell_width = 8;  // how many prefix entries the kernels read unconditionally
  int32_t ell_cover = 8, tell_cover = 8;  // smallest of {2,4,8} covering >= 98 % of the rows (the one-kernel GCN layer)
  // rows with more than kHeavy edges: skipped by the row-group kernel, done by one block each
  int32_t *heavy = nullptr, *theavy = nullptr;
  int32_t n_heavy = 0, n_theavy = 0;
  // source-tile layouts: [direction: 0 forward, 1 transpose][0: T = 64, 1: T = 32]; T == 0 when not built
  gcl_halo halo[2][2];
  // Processing order of the per-edge kernels on large graphs: order16[d][k] = the k-th 16-row group to be processed.
  // A group is placed right after the LAST group it reads from (self-loops aside), so on the bipartite encoder /
  // decoder graphs a block of mesh rows runs while the grid rows it gathers are still in the XCD's L2 (and the other
  // way round for the transposed graph); nullptr on graphs small enough for the L2 anyway.  [0] forward, [1] transpose.
  int32_t* order16[2] = {nullptr, nullptr};
  int32_t n_order16 = 0;
  // host copy of the PyG-order edge list with loops (for export / prune)
  int64_t* h_edges = nullptr;  // [2, e]
};
