// Shared helpers for the deeprest_amd CDNA4 (gfx950) kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>
#include <stdint.h>
#include <algorithm>

#define DR_WAVE 64  // CDNA wavefront width (gfx950)

namespace dr {

// ---- bf16 <-> f32 (bit ops; RNE rounding on store) ----
__device__ __forceinline__ float bf2f(uint16_t x) {
  union { uint32_t u; float f; } v;
  v.u = static_cast<uint32_t>(x) << 16;
  return v.f;
}

__device__ __forceinline__ uint16_t f2bf(float f) {
  // single v_cvt_pk_bf16_f32 (RNE) — the manual add/shift form costs 3 VALU
  __hip_bfloat16 b = __float2bfloat16(f);
  return *reinterpret_cast<uint16_t*>(&b);
}

// two f32 -> packed 2x bf16 in one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t f2bf2(float lo, float hi) {
  __hip_bfloat162 b2 = __float22bfloat162_rn(make_float2(lo, hi));
  return *reinterpret_cast<uint32_t*>(&b2);
}

// generic load/store as float for T in {float, bf16-as-ushort}
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<uint16_t>(const uint16_t* p) { return bf2f(*p); }

template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<uint16_t>(uint16_t* p, float v) { *p = f2bf(v); }

// ---- packed 4-column IO: one 8 B (bf16) / 16 B (f32) op per row per lane ----
__device__ __forceinline__ void ld4(const uint16_t* p, float v[4]) {
  uint2 u = *reinterpret_cast<const uint2*>(p);
  v[0] = bf2f((uint16_t)(u.x & 0xffff));
  v[1] = bf2f((uint16_t)(u.x >> 16));
  v[2] = bf2f((uint16_t)(u.y & 0xffff));
  v[3] = bf2f((uint16_t)(u.y >> 16));
}
__device__ __forceinline__ void ld4(const float* p, float v[4]) {
  float4 u = *reinterpret_cast<const float4*>(p);
  v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
}
__device__ __forceinline__ void st4(uint16_t* p, const float v[4]) {
  uint2 u;
  u.x = f2bf2(v[0], v[1]);
  u.y = f2bf2(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = u;
}
__device__ __forceinline__ void st4(float* p, const float v[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- wave reductions (64-wide) ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, DR_WAVE);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, DR_WAVE));
  return v;
}

// reduce within contiguous 16-lane groups (MFMA C-layout row groups)
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, DR_WAVE);
  return v;
}

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, DR_WAVE));
  return v;
}

// Gate nonlinearities on v_exp_f32 + v_rcp_f32 (1 ulp each), 4-5 instructions.
// __fdividef is a full IEEE division on this target without -ffast-math
// (2 v_div_scale + v_rcp + 6 FMA/mul + v_div_fmas + v_div_fixup); the
// hardware reciprocal moves a result in its last fp32 bit at most a few ulp,
// far below the bf16 rounding every consumer applies.
__device__ __forceinline__ float sigmoidf_(float x) {
  // exp(-x) -> inf for x << 0 gives rcp(inf) = 0
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}

__device__ __forceinline__ float tanhf_(float x) {
  // clamp so exp never overflows into inf * 0 = NaN; tanh(+-15) is +-1 in
  // f32, here to within the reciprocal's ulp
  float xc = fminf(fmaxf(x, -15.f), 15.f);
  float e = __expf(2.f * xc);
  return (e - 1.f) * __builtin_amdgcn_rcpf(e + 1.f);
}

// ---- MFMA fragment types (gfx950) ----
using f32x4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;   // 4 VGPRs: A/B frag of 16x16x32
using s16x8 = __attribute__((ext_vector_type(8))) short;

}  // namespace dr
