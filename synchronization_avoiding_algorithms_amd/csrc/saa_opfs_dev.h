// What the finite-strain element passes (saa_opfs.hip: force and energy) and the tangent passes (saa_optan.hip) share on the
// device: the material numbers and the two inversion counter words.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace saa {

namespace {

constexpr int kSvk = 1, kNeo = 2;

// one inverted element of step `step`: cnt[0] += 1, cnt[1] = min(cnt[1], step)
__device__ __forceinline__ void opfs_count(unsigned long long *cnt, int64_t step) {
  atomicAdd(cnt, 1ull);
  atomicMin(cnt + 1, static_cast<unsigned long long>(step));
}

}  // namespace

}  // namespace saa
