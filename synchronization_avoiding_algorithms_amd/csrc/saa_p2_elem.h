// Device-side pieces of the quadratic (10-node) tetrahedron shared by saa_p2.hip and saa_opstep.hip: the compile-time
// shape-function tables of the two quadrature rules, the element gather, the Jacobian and its inverse.  HIP translation
// units only; everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal_op.h"

namespace saa {

namespace {

// Shape functions and parametric derivatives of the 10-node tetrahedron at NQ points, evaluated by the compiler.
template <int NQ>
struct Rule {
  double w[NQ];
  double N[NQ][10];
  double dN[NQ][10][3];
};

template <int NQ>
constexpr Rule<NQ> make_rule(const double (&xi)[NQ][3], const double (&w)[NQ]) {
  Rule<NQ> r{};
  constexpr int ea[6] = {0, 1, 0, 0, 1, 2}, eb[6] = {1, 2, 2, 3, 3, 3};
  constexpr double dl[4][3] = {{-1.0, -1.0, -1.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int q = 0; q < NQ; ++q) {
    const double L[4] = {1.0 - xi[q][0] - xi[q][1] - xi[q][2], xi[q][0], xi[q][1], xi[q][2]};
    r.w[q] = w[q];
    for (int a = 0; a < 4; ++a) {
      r.N[q][a] = L[a] * (2.0 * L[a] - 1.0);
      for (int j = 0; j < 3; ++j) r.dN[q][a][j] = (4.0 * L[a] - 1.0) * dl[a][j];
    }
    for (int k = 0; k < 6; ++k) {
      r.N[q][4 + k] = 4.0 * L[ea[k]] * L[eb[k]];
      for (int j = 0; j < 3; ++j) r.dN[q][4 + k][j] = 4.0 * (L[eb[k]] * dl[ea[k]][j] + L[ea[k]] * dl[eb[k]][j]);
    }
  }
  return r;
}

// Gauss_Legendre(2) of Tools/Qudrature.py:6-12: four points, weights 1/24
constexpr Rule<4> make_rule4() {
  constexpr double a = 0.5854101966249685, b = 0.1381966011250105;
  constexpr double xi[4][3] = {{a, b, b}, {b, a, b}, {b, b, a}, {b, b, b}};
  constexpr double w[4] = {0.25 / 6, 0.25 / 6, 0.25 / 6, 0.25 / 6};
  return make_rule<4>(xi, w);
}

// Gauss_Legendre(4) of Tools/Qudrature.py:21-45: the six edge mid-points and two orbits of four points
constexpr Rule<14> make_rule14() {
  constexpr double a1 = 0.6984197043243866, b1 = 0.1005267652252045, a2 = 0.0568813795204234, b2 = 0.3143728734931922;
  constexpr double w0 = 0.0190476190476190 / 6.0, w1 = 0.0885898247429807 / 6.0, w2 = 0.1328387466855907 / 6.0;
  constexpr double xi[14][3] = {{0.0, 0.5, 0.5}, {0.5, 0.0, 0.5}, {0.5, 0.5, 0.0}, {0.5, 0.0, 0.0}, {0.0, 0.5, 0.0},
                                {0.0, 0.0, 0.5}, {a1, b1, b1},   {b1, b1, b1},   {b1, b1, a1},   {b1, a1, b1},
                                {a2, b2, b2},   {b2, b2, b2},   {b2, b2, a2},   {b2, a2, b2}};
  constexpr double w[14] = {w0, w0, w0, w0, w0, w0, w1, w1, w1, w1, w2, w2, w2, w2};
  return make_rule<14>(xi, w);
}

// Node ids and coordinates of element e, and its 30 free-dof bits (bit 3a + c set: dof c of node a is free).
__device__ __forceinline__ uint32_t load_element10(const double *__restrict__ xyz, const int32_t *__restrict__ cells,
                                                   const double *__restrict__ free_mask, int64_t e, int32_t v[10],
                                                   double p[10][3]) {
  uint32_t bits = 0;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    v[a] = cells[10 * e + a];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[a][c] = xyz[3 * (int64_t)v[a] + c];
      if (free_mask && free_mask[3 * (int64_t)v[a] + c] != 0.0) bits |= 1u << (3 * a + c);
    }
  }
  return bits;
}

// J[i][j] = sum_a p[a][i] dN[a][j] at point Q of rule R (zeros of the table skipped at compile time)
template <int NQ>
__device__ __forceinline__ void jacobian10(const Rule<NQ> &R, int q, const double p[10][3], double J[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 10; ++a)
        if (R.dN[q][a][j] != 0.0) s += p[a][i] * R.dN[q][a][j];
      J[i][j] = s;
    }
}

__device__ __forceinline__ double det3(const double J[3][3]) {
  return J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
}

// G = J^-1 (so that grad N_a = dN_a/dxi G, Mat_construction.py:42), returns detJ
__device__ __forceinline__ double inverse3(const double J[3][3], double G[3][3]) {
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
               c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
  const double r = 1.0 / det;
  G[0][0] = c00 * r;
  G[1][0] = c01 * r;
  G[2][0] = c02 * r;
  G[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r;
  G[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r;
  G[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r;
  G[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r;
  G[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r;
  G[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r;
  return det;
}

}  // namespace

}  // namespace saa
