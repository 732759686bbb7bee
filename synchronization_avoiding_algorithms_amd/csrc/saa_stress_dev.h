// Device-side pieces shared by the kernels on the saa_operator handle: the (sum, max, argmax) reduction of the stress
// recovery of both element orders (saa_stress.hip, saa_stress_p2.hip; max_merge also in the element bound of
// saa_modal.hip), six-double rows, and the compliance form of the stress error.  HIP translation units only; everything is
// inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"
#include "saa_modal_op.h"

namespace saa {

// better = larger value, on ties the smaller index; NaN never wins (both comparisons are false on a NaN, so a NaN candidate
// is dropped and the sentinel (-1, INT32_MAX) of an idle lane loses to every value)
__device__ __forceinline__ void max_merge(double &v, int32_t &i, double ov, int32_t oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// butterfly over the 64 lanes of a wave: every lane ends with the wave's (sum, max, argmax)
__device__ __forceinline__ void wave_reduce(double &s, double &v, int32_t &i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    const double ov = __shfl_xor(v, off, 64);
    const int32_t oi = __shfl_xor(i, off, 64);
    max_merge(v, i, ov, oi);
  }
}

// The workgroup's partial of column j from its lanes' (w, best, arg): wave_partial puts the waves' results into LDS, once
// per column; fold_partials, once per kernel, adds them in wave order ((w0 + w1) + w2) + w3 and writes [column][workgroup].
struct PartialLds {
  double w[kModalMaxColumns][kWaves], best[kModalMaxColumns][kWaves];
  int32_t arg[kModalMaxColumns][kWaves];
};

__device__ __forceinline__ void wave_partial(PartialLds &l, int32_t j, double w, double best, int32_t arg) {
  wave_reduce(w, best, arg);
  if ((threadIdx.x & 63) == 0) {
    l.w[j][threadIdx.x >> 6] = w;
    l.best[j][threadIdx.x >> 6] = best;
    l.arg[j][threadIdx.x >> 6] = arg;
  }
}

__device__ __forceinline__ void fold_partials(PartialLds &l, int32_t m, double *__restrict__ part_w,
                                              double *__restrict__ part_vm, int32_t *__restrict__ part_idx) {
  __syncthreads();
  const int32_t j = threadIdx.x;
  if (j < m) {
    double w = l.w[j][0], best = l.best[j][0];
    int32_t arg = l.arg[j][0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      w += l.w[j][k];
      max_merge(best, arg, l.best[j][k], l.arg[j][k]);
    }
    part_w[(int64_t)j * gridDim.x + blockIdx.x] = w;
    part_vm[(int64_t)j * gridDim.x + blockIdx.x] = best;
    part_idx[(int64_t)j * gridDim.x + blockIdx.x] = arg;
  }
}

// six consecutive doubles; wide = the address is 16-byte aligned (three 16-byte accesses instead of six 8-byte ones)
__device__ __forceinline__ void load6(const double *__restrict__ p, bool wide, double t[6]) {
  if (wide) {  // (uniform branch)
    const double2 *q = reinterpret_cast<const double2 *>(p);
    const double2 a = q[0], b = q[1], c = q[2];
    t[0] = a.x, t[1] = a.y, t[2] = b.x, t[3] = b.y, t[4] = c.x, t[5] = c.y;
  } else {
#pragma unroll
    for (int c = 0; c < 6; ++c) t[c] = p[c];
  }
}

__device__ __forceinline__ void store6(double *__restrict__ p, bool wide, const double t[6]) {
  if (wide) {  // (uniform branch)
    double2 *q = reinterpret_cast<double2 *>(p);
    q[0] = make_double2(t[0], t[1]);
    q[1] = make_double2(t[2], t[3]);
    q[2] = make_double2(t[4], t[5]);
  } else {
#pragma unroll
    for (int c = 0; c < 6; ++c) p[c] = t[c];
  }
}

// t^T C t with C = D^-1 (commons.py:25-31, engineering shear), split as |dev t|^2 / (2 mu) + tr(t)^2 / (3 (3 lambda + 2 mu)):
// half_imu = 1 / (2 mu), cvol = 1 / (3 (3 lambda + 2 mu)).  A sum of squares: the one-bracket form t.t - lambda / (3 lambda +
// 2 mu) tr^2 cancels on a pressure-dominated t and loses lambda / mu times the rounding (4e-10 at nu = 0.499999).  The normal
// part of |dev t|^2 is ((t0 - t1)^2 + (t1 - t2)^2 + (t2 - t0)^2) / 3.
__device__ __forceinline__ double compliance_form(const double t[6], double half_imu, double cvol) {
  const double tr = t[0] + t[1] + t[2];
  const double d01 = t[0] - t[1], d12 = t[1] - t[2], d20 = t[2] - t[0];
  return half_imu * ((1.0 / 3.0) * (d01 * d01 + d12 * d12 + d20 * d20) + 2.0 * (t[3] * t[3] + t[4] * t[4] + t[5] * t[5])) +
         cvol * (tr * tr);
}

}  // namespace saa
