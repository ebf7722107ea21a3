// Fused multi-tensor Adam: ONE kernel launch updates every parameter tensor.
//
// The host packs [p_ptr[i], g_ptr[i], m_ptr[i], v_ptr[i]] x nt, the
// cumulative-numel table and one step entry per tensor into a single int64
// device buffer (6 * nt entries); the kernel grid-strides over the total
// element count and binary-searches the table (log2(nt) steps) to locate each
// element's tensor. All math fp32:
//   g += wd * p;  m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g
//   p -= lr / (1 - b1^k) * m / (sqrt(v / (1 - b2^k)) + eps)
// with k the tensor's OWN step count (torch.optim.Adam keeps one per
// parameter: a parameter whose gradients start late is at a lower k).
#include "common.h"
#include "kernels.h"

namespace dr {

// 1 - beta^k.  powf and __powf are the same OCML routine under HIP (no fast
// variant is substituted without -ffast-math), so host-step and device-step
// bias factors come from equally accurate code.
__device__ __forceinline__ float adam_bias(float beta, int64_t k) {
  return 1.f - powf(beta, (float)k);
}

// STEP_DEV = true: the step counter lives in device memory (incremented by a
// captured device op between replays), so bias correction stays exact inside
// a hipGraph-captured training step; host-arg bias factors would be frozen
// at their capture-time values.
//
// Step column of the table (meta[5 * nt + i]):
//   STEP_DEV = false: tensor i's step k_i; `common` is the step the by-value
//     bias factors were computed for on the host.
//   STEP_DEV = true: tensor i's lag behind the device counter, k_i = *step_ptr
//     - lag_i, fixed when the table is built; `common` is 0.
// A thread keeps the bias factors of the last entry it met and recomputes them
// only when the entry changes, so with one step for all tensors (the usual
// case) there is no transcendental inside the loop.
template <bool STEP_DEV>
__global__ void fused_adam_kernel(const int64_t* __restrict__ meta, int nt,
                                  int64_t total, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, float bias_c1,
                                  float bias_c2, int64_t common,
                                  const int* __restrict__ step_ptr,
                                  const float* __restrict__ lr_ptr) {
  int64_t counter = 0;
  if (STEP_DEV) {
    // step counter AND learning rate live in device memory so a captured
    // replay keeps exact bias correction and follows LR schedules (the
    // host updates the scalar between replays; a by-value lr would be
    // frozen at its capture-time value)
    counter = *step_ptr;
    bias_c1 = adam_bias(beta1, counter);
    bias_c2 = adam_bias(beta2, counter);
    lr = *lr_ptr;
  }
  int64_t cur = common;  // step entry bias_c1 / bias_c2 belong to
  const int64_t* p_ptrs = meta;
  const int64_t* g_ptrs = meta + nt;
  const int64_t* m_ptrs = meta + 2 * nt;
  const int64_t* v_ptrs = meta + 3 * nt;
  const int64_t* cum = meta + 4 * nt;  // cum[i] = end offset of tensor i (nt entries)
  const int64_t* steps = meta + 5 * nt;

  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    // binary search: first i with cum[i] > idx
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (cum[mid] > idx) hi = mid; else lo = mid + 1;
    }
    const int i = lo;
    const int64_t base = (i == 0) ? 0 : cum[i - 1];
    const int64_t off = idx - base;
    const int64_t entry = steps[i];
    if (entry != cur) {
      const int64_t k = STEP_DEV ? counter - entry : entry;
      bias_c1 = adam_bias(beta1, k);
      bias_c2 = adam_bias(beta2, k);
      cur = entry;
    }

    float* p = reinterpret_cast<float*>(p_ptrs[i]) + off;
    const float* g = reinterpret_cast<const float*>(g_ptrs[i]) + off;
    float* m = reinterpret_cast<float*>(m_ptrs[i]) + off;
    float* v = reinterpret_cast<float*>(v_ptrs[i]) + off;

    float grad = *g;
    float pv = *p;
    if (weight_decay != 0.f) grad += weight_decay * pv;
    float mv = beta1 * (*m) + (1.f - beta1) * grad;
    float vv = beta2 * (*v) + (1.f - beta2) * grad * grad;
    *m = mv;
    *v = vv;
    float denom = sqrtf(vv / bias_c2) + eps;
    *p = pv - (lr / bias_c1) * mv / denom;
  }
}

// grid-stride over all elements, at least one block
static dim3 adam_grid(int64_t total) {
  return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((total + 255) / 256, 4096), 1));
}

}  // namespace dr

// Entry contracts: kernels.h.
extern "C" {

int dr_fused_adam(const int64_t* meta, int nt, int64_t total, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step,
                  hipStream_t stream) {
  float bias_c1 = 1.f - powf(beta1, (float)step);
  float bias_c2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL((dr::fused_adam_kernel<false>), dr::adam_grid(total), dim3(256),
                     0, stream, meta, nt, total, lr, beta1, beta2, eps, weight_decay,
                     bias_c1, bias_c2, step, nullptr, nullptr);
  return (int)hipGetLastError();
}

int dr_fused_adam_dev(const int64_t* meta, int nt, int64_t total,
                      const float* lr_ptr, float beta1, float beta2, float eps,
                      float weight_decay, const int* step_ptr, hipStream_t stream) {
  hipLaunchKernelGGL((dr::fused_adam_kernel<true>), dr::adam_grid(total), dim3(256),
                     0, stream, meta, nt, total, 0.f, beta1, beta2, eps, weight_decay,
                     0.f, 0.f, (int64_t)0, step_ptr, lr_ptr);
  return (int)hipGetLastError();
}

}  // extern "C"
