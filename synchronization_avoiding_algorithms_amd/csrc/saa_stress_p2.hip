// gfx950 kernels of the stress recovery and the stress error estimate of the quadratic (10-node) tetrahedron, on an
// order-2 saa_operator handle (same mesh, same isoparametric geometry as the K apply of saa_p2.hip).
//
// Voigt rows xx, yy, zz, yz, xz, xy with engineering shear, D of commons.py:25-31, as in saa_stress.hip.  The Gauss points
// q = 0..3 are those of the K rule (make_rule4): point q has barycentric weight a on vertex v(q) = (q + 1) mod 4 and b on
// the others, a - b = 1 / sqrt(5), a + 3 b = 1.
//
//  * p2_stress_elem_kernel - one element per lane: J^-1 and w |detJ| at the four points once (as p2_apply_k_kernel), then
//    for each of up to 16 columns the ten nodal displacements STREAM into the four parametric gradients (36 fp64);
//    eps_q = sum_a B_a(xi_q) u_a, sigma_q = D eps_q, von Mises, W_e = 1/2 sum_q w_q |detJ_q| sigma_q . eps_q.  No
//    thirty-entry displacement or physical-gradient array exists per lane.  Per column the lanes reduce sum_e W_e and the
//    largest von Mises with its point index 4 e + q (lowest on ties) to one partial per workgroup.
//  * p2_stress_nodal_kernel - one (node, column) per lane walks the node -> (element, corner) CSR in ascending element
//    order.  The element-linear field through the four Gauss values has the vertex values c_v = sqrt(5) (sigma_q(v) - b S),
//    S = sum_q sigma_q, q(v) = (v + 3) mod 4, and an edge node takes the mean of its two vertices; both are the weights
//    sqrt(5) ((delta(q, q1) + delta(q, q2)) / 2 - b) on the four Gauss rows, formed from the corner number in registers, so
//    the extrapolation is fused into the gather and no [10][6] per-element intermediate is written.
//  * p2_stress_error_kernel<nodal> - one element per lane.  Nodal form (the Zienkiewicz-Zhu estimate): w_p |detJ_p| at the
//    fourteen points of make_rule14 from the ten coordinates, which are then dropped; per column the components are the
//    outer loop: ten nodal and four Gauss values give the ten nodal differences d_a = sigma*_a - sigma_h(node a), and
//    d(xi_p) = sum_a N_a(xi_p) d_a (the quadratic interpolant reproduces the linear sigma_h) updates two accumulators per
//    point, the deviatoric part of d:d and tr d, so the six components never live together at fourteen points.  Element form: the
//    four w_q |detJ_q| and the difference of the two fields at the Gauss points.
//    eta_e^2 = sum_p w_p |detJ_p| (|dev d|^2 / (2 mu) + tr(d)^2 / (3 (3 lambda + 2 mu))), the compliance form d^T C d split
//    into two squares.
//  * p2_stress_vol_kernel, p2_stress_node_weight_kernel - |V_e| = sum_q w_q |detJ_q| and its nodal sums, once per handle.
//
// Register note.  The element pass holds J^-1 (36 fp64), w |detJ| (4), the gradients (36) and ten node ids: 162 of the 256
// registers a lane has at two waves per SIMD.  Left alone the compiler turns the ten ids into ten 64-bit row offsets kept
// across the column loop and works on the four Gauss points (and, in the error pass, on the six components) at once for
// instruction-level parallelism, which needs about 285 registers: one wave per SIMD, or scratch.  Three empty asm
// statements state the intended order as data dependences (sched_barrier and memory clobbers were tried and do not hold
// here, because the reordering happens before instruction scheduling): a node id is opaque where it is used, so its
// offset is formed next to the load; Gauss point q + 1 starts from the energy sum of point q; component c + 1 of the
// error pass starts from the accumulators of component c.  They emit no instruction.  The nodal pass has its two
// alignments as template arguments, since the branch inside the CSR loop cost 27 registers and three waves.
//
// The (sum, max, lowest argmax) partials, load6 / store6 and compliance_form are those of the linear element
// (saa_stress_dev.h); the buffers of the handle are made by stress_prepare of saa_stress.hip, which launches the two setup
// kernels here through p2_stress_setup, and totals and maxima go through its final kernel (one workgroup per column,
// fixed order).  No float atomics: every output is bitwise repeatable, and a column's results do not depend on the other
// columns of the call.  The Dirichlet mask of the handle is not applied: the displacement is read as given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_p2_elem.h"
#include "saa_stress.h"
#include "saa_stress_dev.h"
#include "saa_stress_p2.h"

namespace saa {

namespace {

constexpr double kGaussB = 0.1381966011250105;  // make_rule4's b
constexpr double kSqrt5 = 2.23606797749978969;

// w_q |detJ_q| at the points of rule R from the element's ten coordinates
template <int NQ>
__device__ __forceinline__ void abs_weights(const Rule<NQ> &R, const double p[10][3], double wd[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double J[3][3];
    jacobian10(R, q, p, J);
    wd[q] = R.w[q] * fabs(det3(J));
  }
}

}  // namespace

__global__ void __launch_bounds__(kThreads) p2_stress_vol_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                 const int32_t *__restrict__ cells,
                                                                 double *__restrict__ abs_vol) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double p[10][3], wd[4];
  load_element10(xyz, cells, nullptr, e, v, p);
  abs_weights(R, p, wd);
  abs_vol[e] = (wd[0] + wd[1]) + (wd[2] + wd[3]);
}

__global__ void __launch_bounds__(kThreads) p2_stress_node_weight_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                         const int32_t *__restrict__ pairs,
                                                                         const double *__restrict__ abs_vol,
                                                                         double *__restrict__ node_wsum) {
  const int64_t n = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (n >= n_nodes) return;
  double s = 0.0;
  for (int64_t i = offsets[n]; i < offsets[n + 1]; ++i) s += abs_vol[pairs[i] / 10];
  node_wsum[n] = s;
}

// Element pass: sigma [column][24 e + 6 q + c], von_mises [column][4 e + q], energy [column][e] (each may be null); with
// part_w non-null the per-workgroup partials [column][workgroup] of sum W_e and the largest von Mises with its point.
__global__ void __launch_bounds__(kThreads, 2) p2_stress_elem_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                                  const int32_t *__restrict__ cells, double lam, double mu,
                                                                  const double *__restrict__ x, int64_t ldx,
                                                                  double *__restrict__ sigma, int64_t ld_sigma, bool wide_sigma,
                                                                  double *__restrict__ von_mises, int64_t ld_vm,
                                                                  double *__restrict__ energy, int64_t ld_elem,
                                                                  double *__restrict__ part_w, double *__restrict__ part_vm,
                                                                  int32_t *__restrict__ part_idx) {
  constexpr Rule<4> R = make_rule4();
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  const int64_t ec = valid ? e : 0;  // (idle lanes of the last workgroup compute element 0 and write nothing)
  int32_t v[10];
  double G[4][3][3], hwd[4];
  {
    double p[10][3];
    load_element10(xyz, cells, nullptr, ec, v, p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double J[3][3];
      jacobian10(R, q, p, J);
      hwd[q] = 0.5 * R.w[q] * fabs(inverse3(J, G[q]));
    }
  }
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
      int32_t va = v[a];
      asm volatile("" : "+v"(va));  // (see the register note above)
#pragma unroll
      for (int i = 0; i < 3; ++i) u[i] = xj[3 * (int64_t)va + i];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (R.dN[q][a][k] != 0.0) T[q][i][k] += u[i] * R.dN[q][a][k];
    }
    double w = 0.0, best = -1.0;
    int32_t arg = INT32_MAX;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q > 0) asm volatile("" : "+v"(T[q][0][0]), "+v"(T[q][1][0]), "+v"(T[q][2][0]) : "v"(w));  // (register note)
      // H = grad u = T G; eps = (Hxx, Hyy, Hzz, Hyz + Hzy, Hxz + Hzx, Hxy + Hyx) = sum_a B_a u_a
      double h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = T[q][i][0] * G[q][0][k] + T[q][i][1] * G[q][1][k] + T[q][i][2] * G[q][2][k];
      const double eps[6] = {h[0][0], h[1][1], h[2][2], h[1][2] + h[2][1], h[0][2] + h[2][0], h[0][1] + h[1][0]};
      const double ltr = lam * (eps[0] + eps[1] + eps[2]);
      const double s[6] = {ltr + 2.0 * mu * eps[0], ltr + 2.0 * mu * eps[1], ltr + 2.0 * mu * eps[2],
                           mu * eps[3],             mu * eps[4],             mu * eps[5]};
      // the differences of the normal stresses from the strains: lambda tr(eps) drops out before it can round them
      const double d01 = 2.0 * mu * (eps[0] - eps[1]), d12 = 2.0 * mu * (eps[1] - eps[2]), d20 = 2.0 * mu * (eps[2] - eps[0]);
      const double vm = sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
      w += hwd[q] * (s[0] * eps[0] + s[1] * eps[1] + s[2] * eps[2] + s[3] * eps[3] + s[4] * eps[4] + s[5] * eps[5]);
      if (valid) {
        max_merge(best, arg, vm, (int32_t)(4 * e + q));
        if (sigma) store6(sigma + j * ld_sigma + 24 * e + 6 * q, wide_sigma, s);
        if (von_mises) von_mises[j * ld_vm + 4 * e + q] = vm;
      }
    }
    if (!valid) w = 0.0;
    if (valid && energy) energy[j * ld_elem + e] = w;
    if (part_w) wave_partial(lds, j, w, best, arg);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

// Node pass with the extrapolation fused in: one (node, column) per lane.  kWide: the rows of sigma are 16-byte aligned.
template <bool kWide>
__global__ void __launch_bounds__(kThreads, 8) p2_stress_nodal_kernel(int32_t n_nodes, int32_t m, const int64_t *__restrict__ offsets,
                                                                   const int32_t *__restrict__ pairs,
                                                                   const double *__restrict__ abs_vol,
                                                                   const double *__restrict__ node_wsum,
                                                                   const double *__restrict__ sigma, int64_t ld_sigma,
                                                                   double *__restrict__ sigma_node, int64_t ld_node) {
  const int64_t n = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int32_t j = blockIdx.y;  // one column per grid row
  if (n >= n_nodes || j >= m) return;
  const int64_t b = offsets[n], end = offsets[n + 1];
  const double ws = node_wsum[n];
  const double *sj = sigma + j * ld_sigma;
  // the two vertices of corner 0..9, two bits each: (c, c) for a vertex, the edges (0,1), (1,2), (0,2), (0,3), (1,3), (2,3)
  constexpr uint32_t kVa = 0u | 1u << 2 | 2u << 4 | 3u << 6 | 0u << 8 | 1u << 10 | 0u << 12 | 0u << 14 | 1u << 16 | 2u << 18;
  constexpr uint32_t kVb = 0u | 1u << 2 | 2u << 4 | 3u << 6 | 1u << 8 | 2u << 10 | 2u << 12 | 3u << 14 | 3u << 16 | 3u << 18;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = b; i < end; ++i) {
    const int32_t pair = pairs[i];
    const int64_t e = pair / 10;
    const int corner = pair - 10 * (int32_t)e;
    const int q1 = ((kVa >> (2 * corner)) + 3) & 3, q2 = ((kVb >> (2 * corner)) + 3) & 3;  // q(v) = (v + 3) mod 4
    const double w = abs_vol[e] * kSqrt5;
    const int64_t row = 24 * e;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double t[6];
      load6(sj + row + 6 * q, kWide, t);
      const double cq = w * (0.5 * ((q == q1 ? 1.0 : 0.0) + (q == q2 ? 1.0 : 0.0)) - kGaussB);
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += cq * t[c];
    }
  }
  double *o = sigma_node + j * ld_node + 6 * n;
#pragma unroll
  for (int c = 0; c < 6; ++c) o[c] = ws > 0.0 ? acc[c] / ws : 0.0;
}

// Error pass, one element per lane, the columns looped inside; partials as in p2_stress_elem_kernel (sum, max, lowest
// element).  kNodal: against the quadratic field of other [column][6 n + c] with the 14-point rule; otherwise against the
// Gauss-point field other [column][24 e + 6 q + c] with the 4-point rule.
template <bool kNodal>
__global__ void __launch_bounds__(kThreads, 2) p2_stress_error_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                                   const int32_t *__restrict__ cells, double half_imu,
                                                                   double cvol, const double *__restrict__ sigma,
                                                                   int64_t ld_sigma, const double *__restrict__ other,
                                                                   int64_t ld_other, bool wide, double *__restrict__ eta2,
                                                                   int64_t ld_eta, double *__restrict__ part_w,
                                                                   double *__restrict__ part_vm, int32_t *__restrict__ part_idx) {
  constexpr int NQ = kNodal ? 14 : 4;
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  const int64_t ec = valid ? e : 0;  // (idle lanes of the last workgroup compute element 0 and write nothing)
  int32_t v[10];
  double wd[NQ];
  {
    double p[10][3];
    load_element10(xyz, cells, nullptr, ec, v, p);
    if constexpr (kNodal) {
      constexpr Rule<14> R = make_rule14();
      abs_weights(R, p, wd);
    } else {
      constexpr Rule<4> R = make_rule4();
      abs_weights(R, p, wd);
    }
  }
  for (int32_t j = 0; j < m; ++j) {
    const double *sj = sigma + j * ld_sigma + 24 * ec, *oj = other + j * ld_other;
    double w = 0.0;
    if constexpr (kNodal) {
      constexpr Rule<14> R = make_rule14();
      double dd[14], tr[14];
#pragma unroll
      for (int p = 0; p < 14; ++p) dd[p] = tr[p] = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        int co = c;  // (register note: one component's fourteen loads in flight, not six components')
        if (c > 3)
          asm volatile("" : "+v"(co) : "v"(dd[13]));
        else if (c > 0)
          asm volatile("" : "+v"(co) : "v"(tr[13]));  // (components 0 to 2 end in tr, see below)
        else
          asm volatile("" : "+v"(co));
        const double g0 = sj[co], g1 = sj[6 + co], g2 = sj[12 + co], g3 = sj[18 + co];
        const double bs = kGaussB * ((g0 + g1) + (g2 + g3));
        // vertex values of the element-linear field, c_v = sqrt(5) (sigma_q(v) - b S) with q(v) = (v + 3) mod 4
        const double cv[4] = {kSqrt5 * (g3 - bs), kSqrt5 * (g0 - bs), kSqrt5 * (g1 - bs), kSqrt5 * (g2 - bs)};
        constexpr int ea[6] = {0, 1, 0, 0, 1, 2}, eb[6] = {1, 2, 2, 3, 3, 3};
        double d[10];
#pragma unroll
        for (int a = 0; a < 4; ++a) d[a] = oj[6 * (int64_t)v[a] + co] - cv[a];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[4 + k] = oj[6 * (int64_t)v[4 + k] + co] - 0.5 * (cv[ea[k]] + cv[eb[k]]);
#pragma unroll
        for (int p = 0; p < 14; ++p) {
          double dp = 0.0;
#pragma unroll
          for (int a = 0; a < 10; ++a)
            if (R.N[p][a] != 0.0) dp += R.N[p][a] * d[a];
          // dd: 2 mu times the deviatoric density, tr: the sum of the normal components so far.  The three normal values
          // x0, x1, x2 arrive one component at a time: sum_i (x_i - tr / 3)^2 = (x0 - x1)^2 / 2 + 2 / 3 (x2 - (x0 + x1) / 2)^2,
          // each bracket a difference of neighbours, so that a common pressure drops out of dd before it is squared
          if (c == 0) {
            tr[p] = dp;
          } else if (c == 1) {
            const double d = tr[p] - dp;
            dd[p] = 0.5 * (d * d);
            tr[p] += dp;
          } else if (c == 2) {
            const double d = dp - 0.5 * tr[p];
            dd[p] += (2.0 / 3.0) * (d * d);
            tr[p] += dp;
          } else {
            dd[p] += 2.0 * (dp * dp);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < 14; ++p) w += wd[p] * (half_imu * dd[p] + cvol * (tr[p] * tr[p]));
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double s[6], d[6];
        load6(sj + 6 * q, wide, s);
        load6(oj + 24 * ec + 6 * q, wide, d);
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] -= s[c];
        w += wd[q] * compliance_form(d, half_imu, cvol);
      }
    }
    double best = w;
    int32_t arg = (int32_t)e;
    if (valid) {
      if (eta2) eta2[j * ld_eta + e] = w;
    } else {
      w = 0.0, best = -1.0, arg = INT32_MAX;
    }
    if (part_w) wave_partial(lds, j, w, best, arg);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

namespace {

dim3 elem_grid(const ModalOp *op) { return dim3(static_cast<unsigned>((op->n_elems + kThreads - 1) / kThreads)); }

}  // namespace

hipError_t p2_stress_setup(ModalOp *op) {
  if (op->n_elems > 0)
    hipLaunchKernelGGL(p2_stress_vol_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                       op->abs_vol);
  SAA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(p2_stress_node_weight_kernel, dim3(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs, op->abs_vol, op->node_wsum);
  return hipGetLastError();
}

hipError_t p2_stress_element(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *sigma, int64_t ld_sigma,
                             double *von_mises, int64_t ld_vm, double *energy, int64_t ld_elem, double *energy_total,
                             double *von_mises_max, int32_t *von_mises_argmax) {
  const bool reduce = energy_total || von_mises_max || von_mises_argmax;
  if (!reduce && !sigma && !von_mises && !energy) return hipSuccess;
  SAA_HIP_TRY(stress_prepare(op));
  if (op->n_elems > 0) {
    hipLaunchKernelGGL(p2_stress_elem_kernel, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                       op->lam, op->mu, x, ldx, sigma, ld_sigma, wide_rows(sigma, ld_sigma, m), von_mises, ld_vm, energy, ld_elem,
                       reduce ? op->st_part_w : nullptr, op->st_part_vm, op->st_part_idx);
    SAA_HIP_TRY(hipGetLastError());
  }
  if (reduce) SAA_HIP_TRY(stress_reduce_partials(op, m, energy_total, von_mises_max, von_mises_argmax));
  return hipSuccess;
}

hipError_t p2_stress_nodal(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, double *sigma_node, int64_t ld_node) {
  SAA_HIP_TRY(stress_prepare(op));
  if (op->n_nodes <= 0) return hipSuccess;
  const dim3 grid(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads), static_cast<unsigned>(m));
  if (wide_rows(sigma, ld_sigma, m))
    hipLaunchKernelGGL(p2_stress_nodal_kernel<true>, grid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs,
                       op->abs_vol, op->node_wsum, sigma, ld_sigma, sigma_node, ld_node);
  else
    hipLaunchKernelGGL(p2_stress_nodal_kernel<false>, grid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs,
                       op->abs_vol, op->node_wsum, sigma, ld_sigma, sigma_node, ld_node);
  return hipGetLastError();
}

hipError_t p2_stress_error(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, const double *sigma_node,
                           int64_t ld_node, const double *sigma_other, int64_t ld_other, double *eta2, int64_t ld_eta,
                           double *eta2_total, double *eta2_max, int32_t *eta2_argmax) {
  const bool reduce = eta2_total || eta2_max || eta2_argmax;
  if (!reduce && !eta2) return hipSuccess;
  SAA_HIP_TRY(stress_prepare(op));
  if (op->n_elems > 0) {
    const double half_imu = 0.5 / op->mu, cvol = 1.0 / (3.0 * (3.0 * op->lam + 2.0 * op->mu));
    double *pw = reduce ? op->st_part_w : nullptr;
    if (sigma_node)
      hipLaunchKernelGGL(p2_stress_error_kernel<true>, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz,
                         op->tets, half_imu, cvol, sigma, ld_sigma, sigma_node, ld_node, false, eta2, ld_eta, pw, op->st_part_vm,
                         op->st_part_idx);
    else
      hipLaunchKernelGGL(p2_stress_error_kernel<false>, elem_grid(op), dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz,
                         op->tets, half_imu, cvol, sigma, ld_sigma, sigma_other, ld_other,
                         wide_rows(sigma, ld_sigma, m) && wide_rows(sigma_other, ld_other, m), eta2, ld_eta, pw, op->st_part_vm,
                         op->st_part_idx);
    SAA_HIP_TRY(hipGetLastError());
  }
  if (reduce) SAA_HIP_TRY(stress_reduce_partials(op, m, eta2_total, eta2_max, eta2_argmax));
  return hipSuccess;
}

}  // namespace saa
