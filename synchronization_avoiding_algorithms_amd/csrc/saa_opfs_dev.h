// What the finite-strain element passes (saa_opfs.hip: force and energy), the tangent passes (saa_optan.hip) and the stress
// recovery (saa_stress_fs.hip) share on the device: the material numbers, the two inversion counter words and the
// cancellation-free y - log1p(y) of the neo-Hooke energy.  HIP translation units only.
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

// y - log1p(y) of y > -1, log1p_y = log1p(y) as the caller has it.  Below |y| = 1/16 the difference cancels (relative error
// 2 eps/|y|): there the series y^2 (1/2 - y/3 + ... - y^13/15) by Horner's rule, whose first dropped term is 2^-59 of y^2/2.
__device__ __forceinline__ double opfs_x_minus_log1p(double y, double log1p_y) {
  if (!(fabs(y) < 0.0625)) return y - log1p_y;
  double p = -1.0 / 15.0;
  p = p * y + 1.0 / 14.0;
  p = p * y - 1.0 / 13.0;
  p = p * y + 1.0 / 12.0;
  p = p * y - 1.0 / 11.0;
  p = p * y + 1.0 / 10.0;
  p = p * y - 1.0 / 9.0;
  p = p * y + 1.0 / 8.0;
  p = p * y - 1.0 / 7.0;
  p = p * y + 1.0 / 6.0;
  p = p * y - 1.0 / 5.0;
  p = p * y + 1.0 / 4.0;
  p = p * y - 1.0 / 3.0;
  p = p * y + 0.5;
  return y * y * p;
}

}  // namespace

}  // namespace saa
