// Host-side launch helpers shared by the .hip files.  Grid and LDS arithmetic
// stay in the file that owns the kernel; a launch function returns the
// hipError_t of its set-up or launch (hipGetLastError() right after the
// launch), and the entries hand it on as kernels.h says.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>  // std::true_type / integral_constant tags at the call sites

namespace dr {

// run f with the IO element type as a tag: f(TypeTag<uint16_t>) or <float>
template <typename T> struct TypeTag { using type = T; };
template <typename F>
static hipError_t with_io_type(int is_bf16, F&& f) {
  return is_bf16 ? f(TypeTag<uint16_t>{}) : f(TypeTag<float>{});
}

// Raises a kernel's dynamic-LDS limit.  Each launch function keeps the result
// in a function-local static: set once per instantiation (thread-safe, and
// only for the variant that runs), a failure is returned by every later call.
// Once per process, not per device: a second device used by the same process
// would launch without the attribute.
template <typename K>
static hipError_t allow_lds(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace dr
