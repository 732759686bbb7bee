// The point law of the finite-strain tangent, shared on the device by the tangent element passes (saa_optan.hip) and the
// element bound of the tangent (saa_opdt.hip): what of the material a derivative needs at a displacement gradient, and dP of
// one direction from it.  HIP translation units only; everything is inlined into its caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_opfs_dev.h"

namespace saa {

namespace {

// what of the material at the displacement gradient h the derivative needs.  SVK: a = F = I + h, b = S.  Neo-Hooke: a = F^-T,
// c = mu - lam ln J (b is not used).  false: neo-Hooke and !(det F > 0); nothing is then to be used.
template <int MAT>
__device__ __forceinline__ bool optan_state(const double h[3][3], double lam, double mu, double a[3][3], double b[3][3], double &c) {
  if (MAT == kSvk) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = i; k < 3; ++k) {
        b[i][k] = 0.5 * ((h[i][k] + h[k][i]) + (h[0][i] * h[0][k] + h[1][i] * h[1][k] + h[2][i] * h[2][k]));
        b[k][i] = b[i][k];
      }
    const double ltr = lam * (b[0][0] + b[1][1] + b[2][2]), mu2 = 2.0 * mu;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b[i][k] = mu2 * b[i][k] + (i == k ? ltr : 0.0);  // S
        a[i][k] = h[i][k] + (i == k ? 1.0 : 0.0);        // F
      }
    c = 0.0;
    return true;
  }
  double A[3][3];
  A[0][0] = h[1][1] * h[2][2] - h[1][2] * h[2][1];
  A[0][1] = h[1][2] * h[2][0] - h[1][0] * h[2][2];
  A[0][2] = h[1][0] * h[2][1] - h[1][1] * h[2][0];
  A[1][0] = h[0][2] * h[2][1] - h[0][1] * h[2][2];
  A[1][1] = h[0][0] * h[2][2] - h[0][2] * h[2][0];
  A[1][2] = h[0][1] * h[2][0] - h[0][0] * h[2][1];
  A[2][0] = h[0][1] * h[1][2] - h[0][2] * h[1][1];
  A[2][1] = h[0][2] * h[1][0] - h[0][0] * h[1][2];
  A[2][2] = h[0][0] * h[1][1] - h[0][1] * h[1][0];
  const double rest = (A[0][0] + A[1][1] + A[2][2]) + (h[0][0] * A[0][0] + h[0][1] * A[0][1] + h[0][2] * A[0][2]);
  const double x = (h[0][0] + h[1][1] + h[2][2]) + rest;
  const double J = 1.0 + x;
  if (!(J > 0.0)) return false;
  c = mu - lam * log1p(x);
  const double rJ = 1.0 / J;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[i][k] = (i == k ? 1.0 : 0.0) + ((A[i][k] - h[k][i]) - (i == k ? rest : 0.0)) * rJ;
  return true;
}

// dP of the direction dh at the state (a, b, c) of optan_state
template <int MAT>
__device__ __forceinline__ void optan_dstress(const double a[3][3], const double b[3][3], double c, const double dh[3][3],
                                              double lam, double mu, double dP[3][3]) {
  if (MAT == kSvk) {
    // dE = (dh + dh^T + h^T dh + dh^T h)/2 = (F^T dh + dh^T F)/2, symmetric: upper triangle, mirrored
    double dS[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = i; k < 3; ++k) {
        dS[i][k] = 0.5 * ((a[0][i] * dh[0][k] + a[1][i] * dh[1][k] + a[2][i] * dh[2][k]) +
                          (dh[0][i] * a[0][k] + dh[1][i] * a[1][k] + dh[2][i] * a[2][k]));
        dS[k][i] = dS[i][k];
      }
    const double ltr = lam * (dS[0][0] + dS[1][1] + dS[2][2]), mu2 = 2.0 * mu;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dS[i][k] = mu2 * dS[i][k] + (i == k ? ltr : 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        dP[i][k] = (dh[i][0] * b[0][k] + dh[i][1] * b[1][k] + dh[i][2] * b[2][k]) +
                   (a[i][0] * dS[0][k] + a[i][1] * dS[1][k] + a[i][2] * dS[2][k]);
    return;
  }
  // M = F^-T dh^T, t = F^-T : dh = tr M, dP = mu dh + c M F^-T + lam t F^-T
  double M[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) M[i][k] = a[i][0] * dh[k][0] + a[i][1] * dh[k][1] + a[i][2] * dh[k][2];
  const double lt = lam * (M[0][0] + M[1][1] + M[2][2]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      dP[i][k] = mu * dh[i][k] + (c * (M[i][0] * a[0][k] + M[i][1] * a[1][k] + M[i][2] * a[2][k]) + lt * a[i][k]);
}

}  // namespace

}  // namespace saa
