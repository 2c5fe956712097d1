// Test-only probe of v_mfma_f32_4x4x1_16b_f32's lane layout (tests/test_gpu_mfma4x4_probe.py): one
// wave, one MFMA on caller-chosen per-lane operands, the four result registers written out per
// lane. conv_small.hip's ragged-tail path relies on block b = l / 4 taking its row i from lane
// 4 b + i of the first operand and its column j from lane 4 b + j of the second, and on lane l's
// result register i being row i, column l % 4 of block l / 4.
#include "krrn_common.h"

namespace {

__global__ __launch_bounds__(64) void mfma4x4_probe_kernel(const float* a, const float* b, const float* c, float* d) {
  const int l = threadIdx.x;
  f32x4 acc = *reinterpret_cast<const f32x4*>(c + 4 * l);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[l], b[l], acc, 0, 0, 0);
  *reinterpret_cast<f32x4*>(d + 4 * l) = acc;
}

}  // namespace

KRRN_API int krrn_mfma4x4_probe_f32(const float* a, const float* b, const float* c, float* d, void* stream) {
  if (!a || !b || !c || !d) return KRRN_EARG;
  if (!krrn_aligned16(c) || !krrn_aligned16(d)) return KRRN_EALIGN;
  hipLaunchKernelGGL(mfma4x4_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a, b, c, d);
  return krrn_launch_status();
}
