// gfx950 kernels of the quadratic (10-node, p = 2) tetrahedron on the saa_operator handle, and the load vector and the
// diagonals of either order.
//
// The element is the reference's (Tools/Shape_function_Deriv.py:9-47): barycentric L = (1 - xi - eta -
// zeta, xi, eta, zeta), vertex functions L_a (2 L_a - 1), edge functions 4 L_a L_b on the edges (0,1), (1,2), (0,2),
// (0,3), (1,3), (2,3) - VTK's cell type 24.  The geometry is isoparametric: J[i][j] = sum_a x_a[i] dN_a/dxi_j from all ten
// nodes at every quadrature point (Shape_function_Deriv.py:60-67), detJ signed like the reference's.
//
//  * K: Local_MKF / Local_K_coronary with deg == 2 (Tools/Mat_construction.py:23-119): the 4-point rule Gauss_Legendre(2).
//  * M: the 14-point rule Gauss_Legendre(4), NOT the reference's 4-point rule, whose 30 x 30 element mass has rank 12 (four
//    points x three components) and whose assembled mass is singular.
//  * load: Fe of Local_MKF, sum_q w_q detJ_q N_a(xi_q) f, with the K rule.
//
// Structure of the apply, as in saa_modal.hip: an element pass (one element per lane) writes each element's contributions
// to scratch [column][10 e + corner][3]; the node pass of saa_modal.hip (node_sum_kernel, through modal_node_sum) sums a
// node's entries in ascending element order through the node -> (element, corner) CSR.  No float atomics anywhere.
//
// Register shape of the element pass.  Thirty coordinates, thirty displacements and thirty force accumulators per lane
// would be 90 fp64 = 180 VGPRs, with the thirty physical gradients of a point 120 fp64 = 240 VGPRs, before any temporary:
// no room at two waves per SIMD (256 registers per lane).  Instead the geometry is reduced once per element to what the
// columns need - the inverse Jacobian and w detJ at the 4 points of K (40 fp64), or rho w detJ at the 14 points of M (14
// fp64) - and the coordinates are dropped; a column then STREAMS its ten nodal displacements through the parametric
// gradients sum_a u_a (x) dN_a/dxi of the four points (36 fp64), turns them into T_q = w detJ sigma_q J_q^-T (36 fp64 in
// place), and writes node a's force sum_q T_q dN_a/dxi(q) as it is formed.  Neither the displacements nor the forces of
// an element exist as arrays; the thirty physical gradients per point never exist at all.  All shape-function tables are
// compile-time constants and their zeros are skipped at compile time (the vertex functions' derivatives have one or three
// nonzeros, an edge function's value vanishes at 3 to 5 of the 6 mid-edge points of the 14-point rule).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "saa_modal.h"
#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_p2.h"
#include "saa_p2_elem.h"

namespace saa {

// K element pass, order 2: out layout [column][30 e + 3 corner + component].
__global__ void __launch_bounds__(kThreads) p2_apply_k_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                              const int32_t *__restrict__ cells,
                                                              const double *__restrict__ free_mask, double lam, double mu,
                                                              const double *__restrict__ x, int64_t ldx,
                                                              double *__restrict__ out) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double G[4][3][3], wd[4];
  uint32_t bits;
  {
    double p[10][3];
    bits = load_element10(xyz, cells, free_mask, e, v, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double J[3][3];
      jacobian10(R, q, p, J);
      wd[q] = R.w[q] * inverse3(J, G[q]);
    }
  }
  const int64_t stride = 30 * (int64_t)n_elems;
  for (int32_t j = 0; j < m; ++j) {
    const double *xj = x + j * ldx;
    // parametric gradients of the column at the four points: T[q][i][k] = sum_a u_a[i] dN_a/dxi_k(q)
    double T[4][3][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) T[q][i][k] = 0.0;
#pragma unroll
    for (int a = 0; a < 10; ++a) {
      double u[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double xv = xj[3 * (int64_t)v[a] + i];
        u[i] = (bits >> (3 * a + i)) & 1u ? xv : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (R.dN[q][a][k] != 0.0) T[q][i][k] += u[i] * R.dN[q][a][k];
    }
    // H = grad u = T G, sigma = lam tr(H) I + mu (H + H^T) (commons.py:25-31), T <- w detJ sigma G^T
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double h[3][3], s[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = T[q][i][0] * G[q][0][k] + T[q][i][1] * G[q][1][k] + T[q][i][2] * G[q][2][k];
      const double ltr = lam * (h[0][0] + h[1][1] + h[2][2]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[i][k] = wd[q] * (mu * (h[i][k] + h[k][i]) + (i == k ? ltr : 0.0));
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) T[q][i][k] = s[i][0] * G[q][k][0] + s[i][1] * G[q][k][1] + s[i][2] * G[q][k][2];
    }
    // f_a[i] = sum_q sum_k T[q][i][k] dN_a/dxi_k(q)
    double *o = out + j * stride + 30 * e;
#pragma unroll
    for (int a = 0; a < 10; ++a)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double f = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (R.dN[q][a][k] != 0.0) f += T[q][i][k] * R.dN[q][a][k];
        o[3 * a + i] = f;
      }
  }
}

// M element pass, order 2 (14-point rule): out layout as above.
__global__ void __launch_bounds__(kThreads) p2_apply_m_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                              const int32_t *__restrict__ cells,
                                                              const double *__restrict__ free_mask, double rho,
                                                              const double *__restrict__ x, int64_t ldx,
                                                              double *__restrict__ out) {
  constexpr Rule<14> R = make_rule14();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double wd[14];
  uint32_t bits;
  {
    double p[10][3];
    bits = load_element10(xyz, cells, free_mask, e, v, p);
#pragma unroll
    for (int q = 0; q < 14; ++q) {
      double J[3][3];
      jacobian10(R, q, p, J);
      wd[q] = rho * R.w[q] * det3(J);
    }
  }
  const int64_t stride = 30 * (int64_t)n_elems;
  for (int32_t j = 0; j < m; ++j) {
    const double *xj = x + j * ldx;
    double val[14][3];  // rho w detJ u(xi_q)
#pragma unroll
    for (int q = 0; q < 14; ++q) val[q][0] = val[q][1] = val[q][2] = 0.0;
#pragma unroll
    for (int a = 0; a < 10; ++a) {
      double u[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double xv = xj[3 * (int64_t)v[a] + i];
        u[i] = (bits >> (3 * a + i)) & 1u ? xv : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 14; ++q)
        if (R.N[q][a] != 0.0) {
#pragma unroll
          for (int i = 0; i < 3; ++i) val[q][i] += R.N[q][a] * u[i];
        }
    }
#pragma unroll
    for (int q = 0; q < 14; ++q)
#pragma unroll
      for (int i = 0; i < 3; ++i) val[q][i] *= wd[q];
    double *o = out + j * stride + 30 * e;
#pragma unroll
    for (int a = 0; a < 10; ++a)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double f = 0.0;
#pragma unroll
        for (int q = 0; q < 14; ++q)
          if (R.N[q][a] != 0.0) f += R.N[q][a] * val[q][i];
        o[3 * a + i] = f;
      }
  }
}

// Load, order 2: out[30 e + 3 a + c] = f_c sum_q w_q detJ_q N_a(xi_q) with the K rule.
__global__ void __launch_bounds__(kThreads) p2_load_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                           const int32_t *__restrict__ cells, double fx, double fy, double fz,
                                                           double *__restrict__ out) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double p[10][3], wd[4];
  load_element10(xyz, cells, nullptr, e, v, p);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double J[3][3];
    jacobian10(R, q, p, J);
    wd[q] = R.w[q] * det3(J);
  }
  double *o = out + 30 * e;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += wd[q] * R.N[q][a];
    o[3 * a] = s * fx;
    o[3 * a + 1] = s * fy;
    o[3 * a + 2] = s * fz;
  }
}

// diag(K), order 2: K_e[(a,A),(a,A)] = sum_q w detJ (lam g_A^2 + mu (|g|^2 + g_A^2)), g = dN_a/dxi J^-1.
__global__ void __launch_bounds__(kThreads) p2_diag_k_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                             const int32_t *__restrict__ cells, double lam, double mu,
                                                             double *__restrict__ out) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double G[4][3][3], wd[4];
  {
    double p[10][3];
    load_element10(xyz, cells, nullptr, e, v, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double J[3][3];
      jacobian10(R, q, p, J);
      wd[q] = R.w[q] * inverse3(J, G[q]);
    }
  }
  double *o = out + 30 * e;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    double d[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double g[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double s = 0.0;
#pragma unroll
        for (int jj = 0; jj < 3; ++jj)
          if (R.dN[q][a][jj] != 0.0) s += R.dN[q][a][jj] * G[q][jj][k];
        g[k] = s;
      }
      const double g2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] += wd[q] * (lam * g[k] * g[k] + mu * (g2 + g[k] * g[k]));
    }
    o[3 * a] = d[0];
    o[3 * a + 1] = d[1];
    o[3 * a + 2] = d[2];
  }
}

// diag(M), order 2: rho sum_q w detJ N_a^2 with the 14-point rule, the same on a node's three dofs.
__global__ void __launch_bounds__(kThreads) p2_diag_m_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                             const int32_t *__restrict__ cells, double rho,
                                                             double *__restrict__ out) {
  constexpr Rule<14> R = make_rule14();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double p[10][3], wd[14];
  load_element10(xyz, cells, nullptr, e, v, p);
#pragma unroll
  for (int q = 0; q < 14; ++q) {
    double J[3][3];
    jacobian10(R, q, p, J);
    wd[q] = rho * R.w[q] * det3(J);
  }
  double *o = out + 30 * e;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 14; ++q)
      if (R.N[q][a] != 0.0) s += wd[q] * (R.N[q][a] * R.N[q][a]);
    o[3 * a] = o[3 * a + 1] = o[3 * a + 2] = s;
  }
}

// Load and diagonals of the linear element: f V/4 (the 4-point rule is exact), V (lam g_A^2 + mu (|g|^2 + g_A^2)) (the closed
// form of steady.stiffness_diagonal) and rho V/10; out_* layout [12 e + 3 corner + component], any may be null.
__global__ void __launch_bounds__(kThreads) p1_load_diag_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                const int32_t *__restrict__ tets, double fx, double fy,
                                                                double fz, double lam, double mu, double rho,
                                                                double *__restrict__ out_f, double *__restrict__ out_k,
                                                                double *__restrict__ out_m) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[4];
  double g[4][3];
  const double vol = element_gradients(xyz, tets, e, v, g) / 6.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double g2 = g[a][0] * g[a][0] + g[a][1] * g[a][1] + g[a][2] * g[a][2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (out_f) out_f[12 * e + 3 * a + c] = 0.25 * vol * (c == 0 ? fx : c == 1 ? fy : fz);
      if (out_k) out_k[12 * e + 3 * a + c] = vol * (lam * g[a][c] * g[a][c] + mu * (g2 + g[a][c] * g[a][c]));
      if (out_m) out_m[12 * e + 3 * a + c] = rho * vol / 10.0;
    }
  }
}

namespace {

// scratch of `m` columns of 3 * (nodes per element) * n_elems doubles
hipError_t ensure_scratch(const ModalOp *op, double **buf, int32_t *cap, int32_t m) {
  if (*cap >= m) return hipSuccess;
  if (*buf) {
    SAA_HIP_TRY(hipDeviceSynchronize());  // (a launch still reading the old buffer)
    SAA_HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
  }
  const size_t count = static_cast<size_t>(op->order == 2 ? 30 : 12) * static_cast<size_t>(op->n_elems) * static_cast<size_t>(m);
  SAA_HIP_TRY(hipMalloc(reinterpret_cast<void **>(buf), (count ? count : 1) * sizeof(double)));
  *cap = m;
  return hipSuccess;
}

dim3 elem_grid(const ModalOp *op) { return dim3(static_cast<unsigned>((op->n_elems + kThreads - 1) / kThreads)); }

}  // namespace

int modal_order(const ModalOp *op) { return op->order; }

hipError_t p2_apply(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *kx, double *mx, int64_t ldy) {
  if (kx) SAA_HIP_TRY(ensure_scratch(op, &op->scratch_k, &op->cap_k, m));
  if (mx) SAA_HIP_TRY(ensure_scratch(op, &op->scratch_m, &op->cap_m, m));
  const int64_t stride = 30 * static_cast<int64_t>(op->n_elems);
  if (op->n_elems > 0) {
    if (kx)
      hipLaunchKernelGGL(p2_apply_k_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                         op->free_mask, op->lam, op->mu, x, ldx, op->scratch_k);
    if (mx)
      hipLaunchKernelGGL(p2_apply_m_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                         op->free_mask, op->rho, x, ldx, op->scratch_m);
    SAA_HIP_TRY(hipGetLastError());
  }
  if (kx) SAA_HIP_TRY(modal_node_sum(op, m, op->scratch_k, stride, kx, ldy));
  if (mx) SAA_HIP_TRY(modal_node_sum(op, m, op->scratch_m, stride, mx, ldy));
  return hipSuccess;
}

hipError_t operator_scratch(ModalOp *op, int32_t m, double **buf) {
  SAA_HIP_TRY(ensure_scratch(op, &op->scratch_k, &op->cap_k, m));
  *buf = op->scratch_k;
  return hipSuccess;
}

hipError_t p2_elem_pass_k(ModalOp *op, const double *x, double *contrib) {
  if (op->n_elems == 0) return hipSuccess;
  hipLaunchKernelGGL(p2_apply_k_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, 1, op->xyz, op->tets,
                     op->free_mask, op->lam, op->mu, x, static_cast<int64_t>(0), contrib);
  return hipGetLastError();
}

hipError_t operator_load(ModalOp *op, double fx, double fy, double fz, double *f) {
  SAA_HIP_TRY(ensure_scratch(op, &op->scratch_k, &op->cap_k, 1));
  if (op->n_elems > 0) {
    if (op->order == 2)
      hipLaunchKernelGGL(p2_load_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets, fx, fy, fz,
                         op->scratch_k);
    else
      hipLaunchKernelGGL(p1_load_diag_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets, fx, fy,
                         fz, 0.0, 0.0, 0.0, op->scratch_k, static_cast<double *>(nullptr), static_cast<double *>(nullptr));
    SAA_HIP_TRY(hipGetLastError());
  }
  return modal_node_sum(op, 1, op->scratch_k, 0, f, 0);
}

hipError_t operator_diagonal(ModalOp *op, double *diag_k, double *diag_m) {
  if (diag_k) SAA_HIP_TRY(ensure_scratch(op, &op->scratch_k, &op->cap_k, 1));
  if (diag_m) SAA_HIP_TRY(ensure_scratch(op, &op->scratch_m, &op->cap_m, 1));
  if (op->n_elems > 0) {
    if (op->order == 2) {
      if (diag_k)
        hipLaunchKernelGGL(p2_diag_k_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets, op->lam,
                           op->mu, op->scratch_k);
      if (diag_m)
        hipLaunchKernelGGL(p2_diag_m_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets, op->rho,
                           op->scratch_m);
    } else {
      hipLaunchKernelGGL(p1_load_diag_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets, 0.0,
                         0.0, 0.0, op->lam, op->mu, op->rho, static_cast<double *>(nullptr), diag_k ? op->scratch_k : nullptr,
                         diag_m ? op->scratch_m : nullptr);
    }
    SAA_HIP_TRY(hipGetLastError());
  }
  if (diag_k) SAA_HIP_TRY(modal_node_sum(op, 1, op->scratch_k, 0, diag_k, 0));
  if (diag_m) SAA_HIP_TRY(modal_node_sum(op, 1, op->scratch_m, 0, diag_m, 0));
  return hipSuccess;
}

}  // namespace saa
