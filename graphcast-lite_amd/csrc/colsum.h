// Two-stage float64 column sums with a fixed order, shared by the scorers (verify.hip, maps.hip, eval_step.hip,
// predict.hip, region_train.hip).
//
// Stage 1 sums fixed chunks of rows: a block's row lanes each add their rows in ascending order, and one lane adds the
// lanes in ascending order (lanes_to_part).  Stage 2 adds a column's chunks: every thread takes the partials tid,
// tid + nthreads, .. in ascending order (strided_sum, wave_strided_sum), then the threads are added in a fixed tree
// (block_tree_sum) or butterfly (gcl::wave_sum).  No atomics anywhere.
//
// The chunking is a function of the row count n only - never of the column count, the batch or the launch.  A column's
// result therefore depends on its own data and n: a per-horizon slice scored alone gives the same bits as inside the
// full forecast, and a result repeats bit for bit from run to run.  Changing a constant below changes every score's
// last bits, in every file at once.
//
// Every loop over the NS sums has a compile-time trip count and is fully unrolled: a runtime index into a register
// array is what sends these kernels to scratch.
#pragma once
#include "common.h"

namespace gcl {

constexpr int kColTile = 32;     // columns per block of a partial kernel
constexpr int kRowLanes = 8;     // row lanes of a chunk: 256 threads = 32 columns x 8 row lanes
constexpr int kMaxChunks = 512;  // chunks of rows per column
constexpr int kMinChunkRows = 64;

__host__ __device__ inline int chunk_rows(int n) {
  const int r = (n + kMaxChunks - 1) / kMaxChunks;
  return r < kMinChunkRows ? kMinChunkRows : r;
}
__host__ __device__ inline int num_chunks(int n) { return n <= 0 ? 0 : (n + chunk_rows(n) - 1) / chunk_rows(n); }

// The tail of a partial kernel; every thread of the block calls it (the barrier is unconditional).  Thread tid stores
// its NS sums; a writer - the first of `nlanes` lanes that sit `stride` threads apart - then adds lanes 1 .. nlanes - 1
// to its own in ascending order and stores sum s at dst[s * sstride].  dst is read by writers only.
template <int NS, int T>
__device__ __forceinline__ void lanes_to_part(double (&red)[NS][T], const double (&acc)[NS], int tid, int nlanes,
                                              int stride, bool writer, double* dst, int64_t sstride) {
#pragma unroll
  for (int s = 0; s < NS; ++s) red[s][tid] = acc[s];
  __syncthreads();
  if (writer) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      double v = red[s][tid];
      for (int l = 1; l < nlanes; ++l) v += red[s][tid + l * stride];
      dst[s * sstride] = v;
    }
  }
}

// src[tid] + src[tid + 256] + .. in ascending order, from 0.0: a thread's share of one sum's partials.
__device__ __forceinline__ double strided_sum(const double* __restrict__ src, int64_t nparts, int tid) {
  double v = 0.0;
  for (int64_t j = tid; j < nparts; j += 256) v += src[j];
  return v;
}

// The 128 -> 1 tree over the 256 threads of a block, each of which has stored red[s][tid]: on return red[s][0] holds
// the sum of row s and every thread may read it.
template <int NS>
__device__ __forceinline__ void block_tree_sum(double (&red)[NS][256], int tid) {
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int s = 0; s < NS; ++s) red[s][tid] += red[s][tid + w];
    }
    __syncthreads();
  }
}

// One wave: S[s] = the sum of src[s * nchunk + 0 .. nchunk).  Lane `lane` adds its chunks lane, lane + 64, .. in
// ascending order - the NS sums advance together so that their loads overlap; they are independent, so the interleaving
// does not touch their bits - then the fixed butterfly over the lanes (every lane gets the sums).
template <int NS>
__device__ __forceinline__ void wave_strided_sum(const double* __restrict__ src, int nchunk, int lane, double (&S)[NS]) {
  constexpr int kUnroll = NS <= 4 ? 4 : 2;  // at most 16 loads in flight: more costs the 7-sum caller a wave of occupancy
#pragma unroll
  for (int s = 0; s < NS; ++s) S[s] = 0.0;
#pragma unroll kUnroll
  for (int j = lane; j < nchunk; j += 64) {
#pragma unroll
    for (int s = 0; s < NS; ++s) S[s] += src[(int64_t)s * nchunk + j];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) S[s] = wave_sum(S[s]);
}

}  // namespace gcl
