// Host-side helpers shared by the HIP translation units: early return on a HIP error, and typed device allocation.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// in a function that returns hipError_t: hand the first error to the caller
#define SAA_HIP_TRY(expr)            \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

namespace saa {

// count elements of T (at least one, so that an empty mesh still gets a valid pointer)
template <typename T>
hipError_t dev_alloc(T **p, size_t count) {
  return hipMalloc(reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T));
}

}  // namespace saa
