// Device I/O helpers shared by the matrix-core kernels: linear.hip, gemm_tile.h, linear_x3.hip, gcn_layer.hip.
//
// The accumulator of v_mfma_f32_32x32x2_f32 and of v_mfma_f32_32x32x16_bf16 holds, in lane l, register r,
//   D[i = (r&3) + 8*(r>>2) + 4*(l>>5)][j = l&31]
#pragma once
#include "common.h"

namespace gcl {
namespace mfma_io {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// accumulator row of register `reg` in lane `lane` (see above)
__device__ __forceinline__ int d_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Raw buffer access (hardware range check): loads beyond num_records return 0, stores are dropped.
// Keeping every global access UNCONDITIONAL keeps the kernels free of divergent branches, which is
// what lets hipcc emit counted s_waitcnt vmcnt(N) (CDNA counts loads and stores in one in-order
// counter; a branch around a store forces vmcnt(0) and serialises the whole store stream).
constexpr unsigned kOOB = 0x80000000u;  // offset that is out of range for every descriptor we build
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int64_t nbytes) {
  const int64_t cap = 0x7FFFFF00;
  const int n = (int)(nbytes < 0 ? 0 : (nbytes > cap ? cap : nbytes));
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}
// bytes of a [nrows x F] window with row stride ld (last row counted only up to F)
__device__ __forceinline__ int64_t win_bytes(int64_t nrows, int64_t ld, int F) {
  return nrows > 0 ? ((nrows - 1) * ld + F) * 4 : 0;
}
__device__ __forceinline__ float buf_ld1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_float4(__builtin_bit_cast(float, v.x), __builtin_bit_cast(float, v.y), __builtin_bit_cast(float, v.z),
                     __builtin_bit_cast(float, v.w));
}
// AUX: cache-policy bits of the store (2 = non-temporal); each kernel file passes its own
template <int AUX>
__device__ __forceinline__ void buf_st1(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void buf_st2(__amdgpu_buffer_rsrc_t r, unsigned off, float2 v) {
  typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
  const u32x2_t u = {__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y)};
  __builtin_amdgcn_raw_buffer_store_b64(u, r, off, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void buf_st4(__amdgpu_buffer_rsrc_t r, unsigned off, float4 v) {
  u32x4 u = {__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y), __builtin_bit_cast(unsigned, v.z),
             __builtin_bit_cast(unsigned, v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(u, r, off, 0, AUX);
}

// Zero page for masked loads: an out-of-range lane reads from here instead of branching around
// its load (pointer select + unconditional plain load keeps global_load_dwordx4 and no branch).
// One per translation unit.
static __device__ float4 zero4[1];

}  // namespace mfma_io
}  // namespace gcl
