// torch.optim.Adam with parameter groups over the flat parameter bucket (src/main.py:190-211): a per-parameter learning
// rate, active flag and step counter, all on the device, so the update sits inside a captured hipGraph.
//
// The bucket pads every parameter to a multiple of 64 floats, so each 64-float chunk belongs to one parameter and a
// chunk -> parameter map finds it; the 16 lanes of a chunk take the same branch.  A frozen parameter (torch: grad is
// None) is skipped whole: its p, m, v and step are neither read nor written.  The element update is `adam_elem`, the
// expression of `gcl_adam_step`, so one group with every parameter active is bit-equal to it at the same step.
#include <math.h>

#include "common.h"

namespace {

// bias corrections of every active parameter from its own step (double, as gcl_adam_step computes them on the host)
__global__ __launch_bounds__(256) void adam_groups_tick_kernel(const int32_t* __restrict__ active,
                                                               int32_t* __restrict__ step, float2* __restrict__ bc,
                                                               int32_t P, float b1, float b2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P || !active[i]) return;
  const int t = step[i] + 1;
  step[i] = t;
  bc[i] = make_float2((float)(1.0 - pow((double)b1, (double)t)), (float)sqrt(1.0 - pow((double)b2, (double)t)));
}

// one float4 per lane and iteration: 16 lanes per chunk, 28 B of HBM traffic per active element
__global__ __launch_bounds__(256) void adam_groups_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                          float4* __restrict__ m, float4* __restrict__ v, int64_t n4,
                                                          const int32_t* __restrict__ chunk_param,
                                                          const int32_t* __restrict__ active,
                                                          const float* __restrict__ lr,
                                                          const float2* __restrict__ bc, float b1, float b2, float eps,
                                                          float wd, float gscale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int pi = chunk_param[i >> 4];
    if (!active[pi]) continue;
    const float l = lr[pi];
    const float2 c = bc[pi];
    float4 pv = p[i], mv = m[i], vv = v[i];
    const float4 gv = g[i];
    gcl::adam_elem(pv.x, gv.x, mv.x, vv.x, l, b1, b2, eps, wd, c.x, c.y, gscale);
    gcl::adam_elem(pv.y, gv.y, mv.y, vv.y, l, b1, b2, eps, wd, c.x, c.y, gscale);
    gcl::adam_elem(pv.z, gv.z, mv.z, vv.z, l, b1, b2, eps, wd, c.x, c.y, gscale);
    gcl::adam_elem(pv.w, gv.w, mv.w, vv.w, l, b1, b2, eps, wd, c.x, c.y, gscale);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
  }
}

}  // namespace

extern "C" int gcl_adam_step_groups(float* p, const float* g, float* m, float* v, int64_t count,
                                    const int32_t* chunk_param, int32_t num_params, const int32_t* active,
                                    const float* lr, int32_t* step, float* bc, float beta1, float beta2, float eps,
                                    float weight_decay, float grad_scale, gcl_stream_t stream) {
  GCL_CHECK_ARG(p && g && m && v && chunk_param && active && lr && step && bc, "adam_groups: null argument");
  GCL_CHECK_ARG(count >= 0 && count % 64 == 0 && num_params >= 0,
                "adam_groups: count must be a multiple of 64 (count=%lld)", (long long)count);
  GCL_CHECK_ARG(gcl::aligned16(p) && gcl::aligned16(g) && gcl::aligned16(m) && gcl::aligned16(v) &&
                    (reinterpret_cast<uintptr_t>(bc) & 7) == 0,
                "adam_groups: p, g, m, v must be 16-B aligned and bc 8-B aligned");
  if (num_params == 0 || count == 0) return GCL_OK;  // nothing to update: no step is counted either
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_groups_tick_kernel, dim3((unsigned)gcl::cdiv(num_params, 256)), dim3(256), 0, st, active,
                     step, (float2*)bc, num_params, beta1, beta2);
  const int64_t n4 = count / 4;  // one lane per float4 up to 2048 blocks, grid-stride beyond
  hipLaunchKernelGGL(adam_groups_kernel, dim3(gcl::grid_for(n4, 2048)), dim3(256), 0, st, (float4*)p, (const float4*)g,
                     (float4*)m, (float4*)v, n4, chunk_param, active, lr, (const float2*)bc, beta1, beta2, eps,
                     weight_decay, grad_scale);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
