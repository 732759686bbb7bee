// gfx950 kernels of the stress recovery, on the saa_operator handle of the modal analysis (same mesh, same geometry).
//
//  * stress_elem_kernel - one element per lane: the geometry once (element_gradients, as in the K apply), then for each
//    of up to 16 columns eps = sum_a B_a u_a (Voigt xx, yy, zz, yz, xz, xy, engineering shear: Mat_construction.py:99-104),
//    sigma = D eps (commons.py:25-31), von Mises and W_e = |V_e| sigma . eps / 2.  Per column the lanes also reduce
//    sum_e W_e and max_e vm_e with its element (lowest index on ties) to one partial per workgroup; stress_final_kernel
//    (one workgroup per column) folds the partials in a fixed order.  No float atomics: every output is bitwise
//    repeatable, and a column's results do not depend on the other columns of the call.
//  * nodal_average_kernel - one (node, column) per lane: the |V_e|-weighted mean of k element components over the
//    node's elements in ascending element order (the node -> (element, corner) CSR of the handle).  |V_e| and the
//    per-node weight sums are computed once per handle (stress_vol_kernel, stress_node_weight_kernel).
// The Dirichlet mask of the handle is not applied: the displacement is read as given.
//
// Shared with saa_stress_p2.hip: the reduction helpers, load6 and compliance_form (saa_stress_dev.h), and on the host
// stress_prepare, stress_reduce_partials and wide_rows (saa_stress.h), which serve the handles of both orders.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_stress.h"
#include "saa_stress_dev.h"
#include "saa_stress_p2.h"

namespace saa {

__global__ void __launch_bounds__(kThreads) stress_vol_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                              const int32_t *__restrict__ tets, double *__restrict__ abs_vol) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[4];
  double g[4][3];
  abs_vol[e] = fabs(element_gradients(xyz, tets, e, v, g)) / 6.0;
}

__global__ void __launch_bounds__(kThreads) stress_node_weight_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                      const int32_t *__restrict__ pairs,
                                                                      const double *__restrict__ abs_vol,
                                                                      double *__restrict__ node_wsum) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes) return;
  double s = 0.0;
  for (int64_t i = offsets[v]; i < offsets[v + 1]; ++i) s += abs_vol[pairs[i] >> 2];
  node_wsum[v] = s;
}

// Element pass: sigma [column][6 e + c], von_mises / energy [column][e] (each may be null); with part_w non-null the
// per-workgroup partials [column][workgroup] of sum W_e and max vm_e.
__global__ void __launch_bounds__(kThreads) stress_elem_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                               const int32_t *__restrict__ tets, double lam, double mu,
                                                               const double *__restrict__ x, int64_t ldx,
                                                               double *__restrict__ sigma, int64_t ld_sigma,
                                                               double *__restrict__ von_mises, double *__restrict__ energy,
                                                               int64_t ld_elem, double *__restrict__ part_w,
                                                               double *__restrict__ part_vm, int32_t *__restrict__ part_idx) {
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  int32_t v[4] = {0, 0, 0, 0};
  double g[4][3] = {};
  double half_vol = 0.0;
  if (valid) half_vol = 0.5 * (fabs(element_gradients(xyz, tets, e, v, g)) / 6.0);
  for (int32_t j = 0; j < m; ++j) {
    double w = 0.0, vm = -1.0;
    if (valid) {
      const double *xj = x + j * ldx;
      double u[4][3];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) u[a][c] = xj[3 * (int64_t)v[a] + c];
      // H = grad u; eps = (Hxx, Hyy, Hzz, Hyz + Hzy, Hxz + Hzx, Hxy + Hyx) = sum_a B_a u_a
      double h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = u[0][i] * g[0][k] + u[1][i] * g[1][k] + u[2][i] * g[2][k] + u[3][i] * g[3][k];
      const double eps[6] = {h[0][0], h[1][1], h[2][2], h[1][2] + h[2][1], h[0][2] + h[2][0], h[0][1] + h[1][0]};
      const double ltr = lam * (eps[0] + eps[1] + eps[2]);
      const double s[6] = {ltr + 2.0 * mu * eps[0], ltr + 2.0 * mu * eps[1], ltr + 2.0 * mu * eps[2],
                           mu * eps[3],             mu * eps[4],             mu * eps[5]};
      // the differences of the normal stresses from the strains: lambda tr(eps) drops out before it can round them
      const double d01 = 2.0 * mu * (eps[0] - eps[1]), d12 = 2.0 * mu * (eps[1] - eps[2]), d20 = 2.0 * mu * (eps[2] - eps[0]);
      vm = sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
      w = half_vol * (s[0] * eps[0] + s[1] * eps[1] + s[2] * eps[2] + s[3] * eps[3] + s[4] * eps[4] + s[5] * eps[5]);
      if (sigma) {
        double *o = sigma + j * ld_sigma + 6 * e;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = s[c];
      }
      if (von_mises) von_mises[j * ld_elem + e] = vm;
      if (energy) energy[j * ld_elem + e] = w;
    }
    if (part_w) wave_partial(lds, j, w, vm, valid ? (int32_t)e : INT32_MAX);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

// One workgroup per column: fixed assignment of the partials to lanes, butterfly, then the waves in order.
__global__ void __launch_bounds__(kThreads) stress_final_kernel(int32_t n_parts, const double *__restrict__ part_w,
                                                                const double *__restrict__ part_vm,
                                                                const int32_t *__restrict__ part_idx,
                                                                double *__restrict__ energy_total,
                                                                double *__restrict__ von_mises_max,
                                                                int32_t *__restrict__ von_mises_argmax) {
  __shared__ double lw[kWaves], lvm[kWaves];
  __shared__ int32_t li[kWaves];
  const int64_t base = (int64_t)blockIdx.x * n_parts;
  double w = 0.0, vm = -1.0;
  int32_t arg = INT32_MAX;
  for (int32_t k = threadIdx.x; k < n_parts; k += kThreads) {
    w += part_w[base + k];
    max_merge(vm, arg, part_vm[base + k], part_idx[base + k]);
  }
  wave_reduce(w, vm, arg);
  if ((threadIdx.x & 63) == 0) {
    lw[threadIdx.x >> 6] = w;
    lvm[threadIdx.x >> 6] = vm;
    li[threadIdx.x >> 6] = arg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) {
      w += lw[k];
      max_merge(vm, arg, lvm[k], li[k]);
    }
    if (energy_total) energy_total[blockIdx.x] = w;
    if (von_mises_max) von_mises_max[blockIdx.x] = arg == INT32_MAX ? 0.0 : vm;
    if (von_mises_argmax) von_mises_argmax[blockIdx.x] = arg == INT32_MAX ? -1 : arg;
  }
}

// Error pass, one element per lane, the columns looped inside.  kNodal: against the piecewise-linear field of the nodal
// values other[column][6 v + c], eta_e^2 = |V_e| / 20 (s^T C s + sum_a delta_a^T C delta_a) with delta_a = other(v_a) -
// sigma_e and s = sum_a delta_a (the exact integral of a quadratic over the tetrahedron); otherwise against the element
// field other[column][6 e + c], eta_e^2 = |V_e| delta^T C delta.  The 24 nodal values per element and column are the only
// reads that do not stream; each is a 48-byte row.  Partials as in stress_elem_kernel (sum, max, lowest argmax).
template <bool kNodal>
__global__ void __launch_bounds__(kThreads) stress_error_kernel(int32_t n_elems, int32_t m, const int32_t *__restrict__ tets,
                                                                const double *__restrict__ abs_vol, double half_imu, double cvol,
                                                                const double *__restrict__ sigma, int64_t ld_sigma,
                                                                const double *__restrict__ other, int64_t ld_other,
                                                                bool wide_sigma, bool wide_other, double *__restrict__ eta2,
                                                                int64_t ld_eta, double *__restrict__ part_w,
                                                                double *__restrict__ part_vm, int32_t *__restrict__ part_idx) {
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  int32_t v[4] = {0, 0, 0, 0};
  double scale = 0.0;
  if (valid) {
    if (kNodal) {
      const int4 t = reinterpret_cast<const int4 *>(tets)[e];  // (hipMalloc'ed by the handle: 16-byte aligned)
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
    scale = kNodal ? abs_vol[e] / 20.0 : abs_vol[e];
  }
  for (int32_t j = 0; j < m; ++j) {
    double w = 0.0, best = -1.0;
    if (valid) {
      double se[6];
      load6(sigma + j * ld_sigma + 6 * e, wide_sigma, se);
      const double *oj = other + j * ld_other;
      double q;
      if (kNodal) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        q = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          double d[6];
          load6(oj + 6 * (int64_t)v[a], wide_other, d);
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            d[c] -= se[c];
            s[c] += d[c];
          }
          q += compliance_form(d, half_imu, cvol);
        }
        q += compliance_form(s, half_imu, cvol);
      } else {
        double d[6];
        load6(oj + 6 * e, wide_other, d);
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] -= se[c];
        q = compliance_form(d, half_imu, cvol);
      }
      w = scale * q;
      best = w;
      if (eta2) eta2[j * ld_eta + e] = w;
    }
    if (part_w) wave_partial(lds, j, w, best, valid ? (int32_t)e : INT32_MAX);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

// Node pass: node[j][K v + c] = sum_{e at v} |V_e| elem[j][K e + c] / node_wsum[v], ascending e.
template <int K>
__global__ void __launch_bounds__(kThreads) nodal_average_kernel(int32_t n_nodes, int32_t m, const int64_t *__restrict__ offsets,
                                                                 const int32_t *__restrict__ pairs,
                                                                 const double *__restrict__ abs_vol,
                                                                 const double *__restrict__ node_wsum,
                                                                 const double *__restrict__ elem, int64_t ld_elem,
                                                                 double *__restrict__ node, int64_t ld_node) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int32_t j = blockIdx.y;  // one column per grid row: m times the lanes of a node-serial loop
  if (v >= n_nodes || j >= m) return;
  const int64_t b = offsets[v], end = offsets[v + 1];
  const double ws = node_wsum[v];
  const double *ej = elem + j * ld_elem;
  double acc[K];
#pragma unroll
  for (int c = 0; c < K; ++c) acc[c] = 0.0;
  for (int64_t i = b; i < end; ++i) {
    const int64_t e = pairs[i] >> 2;
    const double w = abs_vol[e];
    const double *q = ej + K * e;
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] += w * q[c];
  }
  double *o = node + j * ld_node + K * v;
#pragma unroll
  for (int c = 0; c < K; ++c) o[c] = ws > 0.0 ? acc[c] / ws : 0.0;
}

namespace {

int32_t n_parts_of(const ModalOp *op) { return (op->n_elems + kThreads - 1) / kThreads; }

void stress_buffers_free(ModalOp *op) {
  for (void **b : {reinterpret_cast<void **>(&op->abs_vol), reinterpret_cast<void **>(&op->node_wsum),
                   reinterpret_cast<void **>(&op->st_part_w), reinterpret_cast<void **>(&op->st_part_vm),
                   reinterpret_cast<void **>(&op->st_part_idx)}) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
}

// |V_e| and the node weight sums of a linear-element handle (order 2: p2_stress_setup)
hipError_t stress_setup(ModalOp *op) {
  if (op->n_elems > 0)
    hipLaunchKernelGGL(stress_vol_kernel, dim3(static_cast<unsigned>(n_parts_of(op))), dim3(kThreads), 0, op->stream,
                       op->n_elems, op->xyz, op->tets, op->abs_vol);
  SAA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(stress_node_weight_kernel, dim3(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs, op->abs_vol, op->node_wsum);
  return hipGetLastError();
}

}  // namespace

int32_t modal_n_elems(const ModalOp *op) { return op->n_elems; }

hipError_t stress_prepare(ModalOp *op) {
  if (op->st_part_idx) return hipSuccess;
  const size_t parts = static_cast<size_t>(n_parts_of(op)) * kModalMaxColumns;
  hipError_t e = dev_alloc(&op->abs_vol, static_cast<size_t>(op->n_elems));
  if (e == hipSuccess) e = dev_alloc(&op->node_wsum, static_cast<size_t>(op->n_nodes));
  if (e == hipSuccess) e = dev_alloc(&op->st_part_w, parts);
  if (e == hipSuccess) e = dev_alloc(&op->st_part_vm, parts);
  if (e == hipSuccess) e = dev_alloc(&op->st_part_idx, parts);
  if (e == hipSuccess) e = op->order == 2 ? p2_stress_setup(op) : stress_setup(op);
  if (e != hipSuccess) stress_buffers_free(op);
  return e;
}

hipError_t stress_reduce_partials(ModalOp *op, int32_t m, double *total, double *best, int32_t *argbest) {
  hipLaunchKernelGGL(stress_final_kernel, dim3(static_cast<unsigned>(m)), dim3(kThreads), 0, op->stream, n_parts_of(op),
                     op->st_part_w, op->st_part_vm, op->st_part_idx, total, best, argbest);
  return hipGetLastError();
}

hipError_t stress_element(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *sigma, int64_t ld_sigma,
                          double *von_mises, double *energy, int64_t ld_elem, double *energy_total, double *von_mises_max,
                          int32_t *von_mises_argmax) {
  const bool reduce = energy_total || von_mises_max || von_mises_argmax;
  if (!reduce && !sigma && !von_mises && !energy) return hipSuccess;
  SAA_HIP_TRY(stress_prepare(op));
  const int32_t n_parts = n_parts_of(op);
  if (n_parts > 0) {
    hipLaunchKernelGGL(stress_elem_kernel, dim3(static_cast<unsigned>(n_parts)), dim3(kThreads), 0, op->stream, op->n_elems, m,
                       op->xyz, op->tets, op->lam, op->mu, x, ldx, sigma, ld_sigma, von_mises, energy, ld_elem,
                       reduce ? op->st_part_w : nullptr, op->st_part_vm, op->st_part_idx);
    SAA_HIP_TRY(hipGetLastError());
  }
  if (reduce) SAA_HIP_TRY(stress_reduce_partials(op, m, energy_total, von_mises_max, von_mises_argmax));
  return hipSuccess;
}

bool stress_has_compliance(const ModalOp *op) { return op->mu > 0.0 && 3.0 * op->lam + 2.0 * op->mu > 0.0; }

hipError_t stress_error(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, const double *sigma_node, int64_t ld_node,
                        const double *sigma_other, int64_t ld_other, double *eta2, int64_t ld_eta, double *eta2_total,
                        double *eta2_max, int32_t *eta2_argmax) {
  const bool reduce = eta2_total || eta2_max || eta2_argmax;
  if (!reduce && !eta2) return hipSuccess;
  SAA_HIP_TRY(stress_prepare(op));
  const int32_t n_parts = n_parts_of(op);
  if (n_parts > 0) {
    const double half_imu = 0.5 / op->mu, cvol = 1.0 / (3.0 * (3.0 * op->lam + 2.0 * op->mu));
    const double *other = sigma_node ? sigma_node : sigma_other;
    const int64_t ldo = sigma_node ? ld_node : ld_other;
    double *pw = reduce ? op->st_part_w : nullptr;
#define STRESS_ERROR(NODAL)                                                                                           \
  hipLaunchKernelGGL(stress_error_kernel<NODAL>, dim3(static_cast<unsigned>(n_parts)), dim3(kThreads), 0, op->stream, \
                     op->n_elems, m, op->tets, op->abs_vol, half_imu, cvol, sigma, ld_sigma, other, ldo,              \
                     wide_rows(sigma, ld_sigma, m), wide_rows(other, ldo, m), eta2, ld_eta, pw, op->st_part_vm,       \
                     op->st_part_idx)
    if (sigma_node)
      STRESS_ERROR(true);
    else
      STRESS_ERROR(false);
#undef STRESS_ERROR
    SAA_HIP_TRY(hipGetLastError());
  }
  if (reduce) SAA_HIP_TRY(stress_reduce_partials(op, m, eta2_total, eta2_max, eta2_argmax));
  return hipSuccess;
}

hipError_t stress_nodal_average(ModalOp *op, int32_t m, int32_t k, const double *elem, int64_t ld_elem, double *node,
                                int64_t ld_node) {
  SAA_HIP_TRY(stress_prepare(op));
  const dim3 grid(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads), static_cast<unsigned>(m));
#define STRESS_NODAL(K)                                                                                                       \
  case K:                                                                                                                     \
    hipLaunchKernelGGL(nodal_average_kernel<K>, grid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs, \
                       op->abs_vol, op->node_wsum, elem, ld_elem, node, ld_node);                                             \
    break;
  switch (k) {
    STRESS_NODAL(1)
    STRESS_NODAL(2)
    STRESS_NODAL(3)
    STRESS_NODAL(4)
    STRESS_NODAL(5)
    STRESS_NODAL(6)
    STRESS_NODAL(7)
    STRESS_NODAL(8)
    default:
      return hipErrorInvalidValue;
  }
#undef STRESS_NODAL
  return hipGetLastError();
}

}  // namespace saa
