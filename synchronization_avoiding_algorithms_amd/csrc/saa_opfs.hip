// gfx950 kernels of the finite-strain (total-Lagrangian) element pass on the saa_operator handle, either element order, and
// the host side of saa_operator_internal_force, of saa_operator_tangent_apply (whose element passes are saa_optan.hip) and of
// the stepper's material (saa_opstep.h).
//
//  * H = grad_X u and F = I + H at the points of the K rule: order 1 the one constant gradient of element_gradients, order 2
//    H = T G at the four Gauss points exactly as p2_k_column (saa_opstep.hip) forms it.  The first Piola-Kirchhoff stress P
//    takes the place of the linear pass's symmetric sigma and nothing else changes: f_a[i] = sum_q w_q detJ_q sum_k
//    P_q[i][k] dN_a/dX_k(q), sign and detJ convention those of the linear pass of the same order, displacements on Dirichlet
//    dofs masked to 0 on input.
//      St. Venant-Kirchhoff:    E = (H + H^T + H^T H)/2, S = lam tr(E) I + 2 mu E, P = F S, W = lam/2 tr(E)^2 + mu E:E
//      compressible neo-Hooke:  J = det F, P = mu (F - F^-T) + lam ln(J) F^-T, W = mu/2 (F:F - 3) - mu ln J + lam/2 (ln J)^2
//    Both linearise to the handle's K at u = 0.  Neo-Hooke is evaluated from H without forming F (opfs_stress), so that it
//    keeps its digits at any strain, however small, and under a rigid rotation.
//  * The pass writes the [npe e + corner][3] contributions the node passes of saa_modal.hip / saa_opstep.hip sum, so
//    everything downstream of the element pass is what it was.  ENERGY = true also writes energy_elem[e] = sum_q w_q
//    |detJ_q| W(F_q); the stepper launches ENERGY = false only.
//  * Inversion (neo-Hooke only; SVK does not look at J): an element with !(J > 0) at any of its points, NaN included, writes
//    all its contributions (and its energy) as 0 and is counted in two device words - the number of (element, step) events
//    and the lowest step index of one - with integer atomics.  No floating-point atomics; bitwise repeatable.
//  * Order 2 reads the reduced geometry of opstep_geometry_kernel, the component-major [40][n_elems] table and the free-dof
//    bits, which the HANDLE owns (one table per handle, whoever asks first).  There is no recomputing variant.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opfs_dev.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_p2.h"
#include "saa_p2_elem.h"

namespace saa {

namespace {

// P (first Piola-Kirchhoff) and, with ENERGY, W of the material MAT at displacement gradient h.  false: MAT is neo-Hooke and
// !(det F > 0); P and W are then not to be used.
template <int MAT, bool ENERGY>
__device__ __forceinline__ bool opfs_stress(const double h[3][3], double lam, double mu, double P[3][3], double &W) {
  if (MAT == kSvk) {
    double F[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) F[i][k] = h[i][k] + (i == k ? 1.0 : 0.0);
    // E = (h + h^T + h^T h)/2, symmetric: the upper triangle is computed, the lower mirrored
    double E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = i; k < 3; ++k) {
        E[i][k] = 0.5 * ((h[i][k] + h[k][i]) + (h[0][i] * h[0][k] + h[1][i] * h[1][k] + h[2][i] * h[2][k]));
        E[k][i] = E[i][k];
      }
    const double tr = E[0][0] + E[1][1] + E[2][2];
    if (ENERGY) {
      double ee = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) ee += E[i][k] * E[i][k];
      W = 0.5 * lam * tr * tr + mu * ee;
    }
    const double ltr = lam * tr, mu2 = 2.0 * mu;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) E[i][k] = mu2 * E[i][k] + (i == k ? ltr : 0.0);  // S
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) P[i][k] = F[i][0] * E[0][k] + F[i][1] * E[1][k] + F[i][2] * E[2][k];
    return true;
  }
  // Neo-Hooke from h, never from F = I + h: at |h| << 1 the textbook P = mu F + ((lam ln J - mu)/J) cof F is an O(h)
  // difference of O(1) numbers (relative error eps/|h|) and mu tr(h) - mu ln J an O(h^2) difference of O(h) ones
  // (eps/|h|^2).  With A = cof(h) and cof(I + h) = (1 + tr h) I - h^T + A:
  //   J - 1 = tr h + tr A + det h,  ln J = log1p(J - 1),  F^-T - I = (A - h^T - (tr A + det h) I) / J
  //   P = mu (h - (F^-T - I)) + lam ln J (I + (F^-T - I))
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
  const double lnJ = log1p(x);
  const double rJ = 1.0 / J, llj = lam * lnJ;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double G = ((A[i][k] - h[k][i]) - (i == k ? rest : 0.0)) * rJ;
      P[i][k] = mu * (h[i][k] - G) + llj * ((i == k ? 1.0 : 0.0) + G);
    }
  if (ENERGY) {
    // mu/2 (F:F - 3) - mu ln J = mu/2 (tr e - log1p(y)) with e = 2 E = h + h^T + h^T h and y = J^2 - 1 = tr e + tr cof(e) +
    // det e, so mu/2 ((y - log1p(y)) - (tr cof(e) + det e)): through e, which a rigid rotation leaves alone (h:h does not)
    double e[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = i; k < 3; ++k) {
        e[i][k] = (h[i][k] + h[k][i]) + (h[0][i] * h[0][k] + h[1][i] * h[1][k] + h[2][i] * h[2][k]);
        e[k][i] = e[i][k];
      }
    const double c00 = e[1][1] * e[2][2] - e[1][2] * e[1][2], c11 = e[0][0] * e[2][2] - e[0][2] * e[0][2],
                 c22 = e[0][0] * e[1][1] - e[0][1] * e[0][1];
    const double c01 = e[1][2] * e[0][2] - e[0][1] * e[2][2], c02 = e[0][1] * e[1][2] - e[1][1] * e[0][2];
    const double low = (c00 + c11 + c22) + (e[0][0] * c00 + e[0][1] * c01 + e[0][2] * c02);
    const double y = (e[0][0] + e[1][1] + e[2][2]) + low;
    W = 0.5 * mu * (opfs_x_minus_log1p(y, 2.0 * lnJ) - low) + 0.5 * lam * lnJ * lnJ;
  }
  return true;
}

}  // namespace

// Finite-strain element pass, order 1, one column: out[12 e + 3 corner + component].
template <int MAT, bool ENERGY>
__global__ void __launch_bounds__(kThreads) opfs_elem_p1_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                const int32_t *__restrict__ tets, const double *__restrict__ free_mask,
                                                                double lam, double mu, const double *__restrict__ x,
                                                                double *__restrict__ out, double *__restrict__ energy_elem,
                                                                unsigned long long *__restrict__ cnt, int64_t step) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[4];
  double g[4][3];
  const double det = element_gradients(xyz, tets, e, v, g);
  const double vol = det / 6.0;  // signed, like the linear pass
  double u[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) u[a][c] = free_mask[3 * (int64_t)v[a] + c] * x[3 * (int64_t)v[a] + c];
  double h[3][3], P[3][3], W = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) h[i][k] = u[0][i] * g[0][k] + u[1][i] * g[1][k] + u[2][i] * g[2][k] + u[3][i] * g[3][k];
  const bool ok = opfs_stress<MAT, ENERGY>(h, lam, mu, P, W);
  double *o = out + 12 * e;
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0.0;
    if (ENERGY) energy_elem[e] = 0.0;
    opfs_count(cnt, step);
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) P[i][k] *= vol;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[3 * a + i] = P[i][0] * g[a][0] + P[i][1] * g[a][1] + P[i][2] * g[a][2];
  if (ENERGY) energy_elem[e] = fabs(vol) * W;
}

// Finite-strain element pass, order 2, one column, geometry from the table: out[30 e + 3 corner + component].  The body of
// p2_k_column (saa_opstep.hip) with P in the place of sigma; the four points are worked through one at a time, each
// reading its own nine G and its wd, so that F, the strain and the stress of one point only are live next to T.
template <int MAT, bool ENERGY>
__global__ void __launch_bounds__(kThreads, 2) opfs_elem_p2_kernel(int32_t n_elems, const int32_t *__restrict__ cells,
                                                                const double *__restrict__ geom,
                                                                const uint32_t *__restrict__ bits_tab, double lam, double mu,
                                                                const double *__restrict__ x, double *__restrict__ out,
                                                                double *__restrict__ energy_elem,
                                                                unsigned long long *__restrict__ cnt, int64_t step) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  const uint32_t bits = bits_tab[e];
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
    const int64_t va = cells[10 * e + a];
    double u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double xv = x[3 * va + i];
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
  // H = T G, P(H), T <- w detJ P G^T
  bool ok = true;
  double en = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double G[3][3], h[3][3], P[3][3], W = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) G[i][k] = geom[(9 * q + 3 * i + k) * (int64_t)n_elems + e];
    const double wd = geom[(36 + q) * (int64_t)n_elems + e];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) h[i][k] = T[q][i][0] * G[0][k] + T[q][i][1] * G[1][k] + T[q][i][2] * G[2][k];
    ok = opfs_stress<MAT, ENERGY>(h, lam, mu, P, W) && ok;
    if (ENERGY) en += fabs(wd) * W;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) P[i][k] *= wd;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) T[q][i][k] = P[i][0] * G[k][0] + P[i][1] * G[k][1] + P[i][2] * G[k][2];
  }
  double *o = out + 30 * e;
  if (MAT == kNeo && !ok) {
#pragma unroll
    for (int j = 0; j < 30; ++j) o[j] = 0.0;
    if (ENERGY) energy_elem[e] = 0.0;
    opfs_count(cnt, step);
    return;
  }
  // f_a[i] = sum_q sum_k T[q][i][k] dN_a/dxi_k(q)
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
  if (ENERGY) energy_elem[e] = en;
}

namespace {

// the two counter words: 0 events, no step yet (all ones)
hipError_t reset_counters(unsigned long long *cnt, hipStream_t stream) {
  SAA_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), stream));
  return hipMemsetAsync(cnt + 1, 0xff, sizeof(unsigned long long), stream);
}

hipError_t alloc_counters(unsigned long long **cnt, hipStream_t stream) {
  if (*cnt) return hipSuccess;
  SAA_HIP_TRY(dev_alloc(cnt, 2));
  return reset_counters(*cnt, stream);
}

template <int MAT, bool ENERGY>
hipError_t launch(ModalOp *op, const double *x, double *contrib, double *energy_elem, unsigned long long *cnt, int64_t step) {
  if (op->n_elems == 0) return hipSuccess;
  if (op->order == 2)
    hipLaunchKernelGGL((opfs_elem_p2_kernel<MAT, ENERGY>), opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems,
                       op->tets, op->geom, op->bits, op->lam, op->mu, x, contrib, energy_elem, cnt, step);
  else
    hipLaunchKernelGGL((opfs_elem_p1_kernel<MAT, ENERGY>), opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems,
                       op->xyz, op->tets, op->free_mask, op->lam, op->mu, x, contrib, energy_elem, cnt, step);
  return hipGetLastError();
}

hipError_t read_counters(ModalOp *op, const unsigned long long *cnt, int64_t *count, int64_t *first_step) {
  unsigned long long host[2] = {0, ~0ull};
  SAA_HIP_TRY(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipStreamSynchronize(op->stream));
  if (count) *count = static_cast<int64_t>(host[0]);
  if (first_step) *first_step = host[1] == ~0ull ? -1 : static_cast<int64_t>(host[1]);
  return hipSuccess;
}

}  // namespace

hipError_t opfs_element_pass(OpStepper *st, const double *x, double *contrib) {
  ModalOp *op = st->op;
  if (st->material == kSvk) return launch<kSvk, false>(op, x, contrib, nullptr, st->inverted, st->step_index);
  return launch<kNeo, false>(op, x, contrib, nullptr, st->inverted, st->step_index);
}

hipError_t opfs_element_pass_scratch(OpStepper *st, const double *x, double *contrib) {
  ModalOp *op = st->op;
  SAA_HIP_TRY(alloc_counters(&op->fs_count, op->stream));
  SAA_HIP_TRY(reset_counters(op->fs_count, op->stream));
  if (st->material == kSvk) return launch<kSvk, false>(op, x, contrib, nullptr, op->fs_count, 0);
  return launch<kNeo, false>(op, x, contrib, nullptr, op->fs_count, 0);
}

hipError_t operator_internal_force(ModalOp *op, int material, const double *x, double *f, double *energy_elem, int64_t *n_inverted) {
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  if (material == 0) {
    SAA_HIP_TRY(op->order == 2 ? p2_elem_pass_k(op, x, contrib) : modal_elem_pass_k(op, x, contrib));
    SAA_HIP_TRY(modal_node_sum(op, 1, contrib, 0, f, 0));
    if (n_inverted) *n_inverted = 0;
    return hipSuccess;
  }
  SAA_HIP_TRY(operator_geometry(op));
  SAA_HIP_TRY(alloc_counters(&op->fs_count, op->stream));
  SAA_HIP_TRY(reset_counters(op->fs_count, op->stream));
  if (material == kSvk)
    SAA_HIP_TRY(energy_elem ? (launch<kSvk, true>(op, x, contrib, energy_elem, op->fs_count, 0))
                         : (launch<kSvk, false>(op, x, contrib, nullptr, op->fs_count, 0)));
  else
    SAA_HIP_TRY(energy_elem ? (launch<kNeo, true>(op, x, contrib, energy_elem, op->fs_count, 0))
                         : (launch<kNeo, false>(op, x, contrib, nullptr, op->fs_count, 0)));
  SAA_HIP_TRY(modal_node_sum(op, 1, contrib, 0, f, 0));
  if (n_inverted) SAA_HIP_TRY(read_counters(op, op->fs_count, n_inverted, nullptr));
  return hipSuccess;
}

hipError_t operator_tangent_apply(ModalOp *op, int material, const double *u, const double *v, double *kv, int64_t *n_inverted) {
  if (material == 0) return operator_internal_force(op, 0, v, kv, nullptr, n_inverted);
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  SAA_HIP_TRY(operator_geometry(op));
  SAA_HIP_TRY(alloc_counters(&op->fs_count, op->stream));
  SAA_HIP_TRY(reset_counters(op->fs_count, op->stream));
  SAA_HIP_TRY(optan_element_pass(op, material, u, v, contrib, op->fs_count));
  SAA_HIP_TRY(modal_node_sum(op, 1, contrib, 0, kv, 0));
  if (n_inverted) SAA_HIP_TRY(read_counters(op, op->fs_count, n_inverted, nullptr));
  return hipSuccess;
}

hipError_t operator_tangent_apply_block(ModalOp *op, int material, const double *u, int32_t m, const double *v, int64_t ldv,
                                        double *kv, int64_t ldkv, int64_t *n_inverted) {
  if (material == 0) {
    SAA_HIP_TRY(op->order == 2 ? p2_apply(op, m, v, ldv, kv, nullptr, ldkv) : modal_apply(op, m, v, ldv, kv, nullptr, ldkv));
    if (n_inverted) {
      SAA_HIP_TRY(hipStreamSynchronize(op->stream));
      *n_inverted = 0;
    }
    return hipSuccess;
  }
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, m, &contrib));
  SAA_HIP_TRY(operator_geometry(op));
  SAA_HIP_TRY(alloc_counters(&op->fs_count, op->stream));
  SAA_HIP_TRY(reset_counters(op->fs_count, op->stream));
  const int64_t stride = (op->order == 2 ? 30 : 12) * static_cast<int64_t>(op->n_elems);
  SAA_HIP_TRY(optan_block_element_pass(op, material, u, m, v, ldv, contrib, stride, op->fs_count));
  SAA_HIP_TRY(modal_node_sum(op, m, contrib, stride, kv, ldkv));
  if (n_inverted) SAA_HIP_TRY(read_counters(op, op->fs_count, n_inverted, nullptr));
  return hipSuccess;
}

int opstep_material(const OpStepper *st) { return st->material; }

hipError_t opstep_set_material(OpStepper *st, int material) {
  ModalOp *op = st->op;
  if (material != 0) {
    SAA_HIP_TRY(operator_geometry(op));
    SAA_HIP_TRY(alloc_counters(&st->inverted, op->stream));
  }
  st->material = material;
  return opstep_clear_inverted(st);
}

hipError_t opstep_clear_inverted(OpStepper *st) { return st->inverted ? reset_counters(st->inverted, st->op->stream) : hipSuccess; }

hipError_t opstep_inverted(OpStepper *st, int64_t *count, int64_t *first_step) {
  if (!st->inverted) {
    SAA_HIP_TRY(hipStreamSynchronize(st->op->stream));
    if (count) *count = 0;
    if (first_step) *first_step = -1;
    return hipSuccess;
  }
  return read_counters(st->op, st->inverted, count, first_step);
}

void opfs_release(OpStepper *st) {
  if (!st || !st->inverted) return;
  (void)hipSetDevice(st->op->device);
  (void)hipFree(st->inverted);
  st->inverted = nullptr;
}

}  // namespace saa
