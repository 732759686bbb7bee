// gfx950 kernels of the explicit time loop on the saa_operator handle, either element order (saa_opstep.h).
//
//  * Lumped mass.  Order 2 is HRZ (Hinton-Rock-Zienkiewicz): the diagonal of the consistent element mass of the 14-point
//    rule, scaled so that an element's ten masses add up to rho times its volume.  The reference's row sum
//    (Tools/commons.py:103-107) gives every vertex of a quadratic tetrahedron the NEGATIVE mass rho integral N_vertex =
//    -rho V/20, which is why its p = 2 stops at the steady case (Data_prepare.py:43, Mat_construction.py:31).  On a straight
//    element the HRZ masses are rho V/36 at a vertex and 4 rho V/27 on an edge.  Order 1 is the row sum rho V/4.
//  * One step, Dynamic_solver.py:12-20 on one rank, in two launches.  (a) The K element pass for the single column d0 writes
//    every (element, corner) contribution: the pass of the block apply itself (p2_apply_k_kernel / elem_apply_kernel with
//    m = 1), or, for order 2, opstep_elem_p2_kernel, which reads the element's reduced geometry - J^-1 and w detJ at the four
//    points of the K rule, 40 fp64, and its 30 free-dof bits - from a table built once, component-major ([40][n_elems]) so
//    that a wave reads every component coalesced, instead of rebuilding four Jacobians from thirty gathered coordinates.
//    (b) opstep_node_kernel<MODE, ENERGY>, one lane per node, sums the node's contributions through the node -> (element,
//    corner) CSR in ascending element order, forms d1 and writes it over dn (a lane touches its own node only, so two buffers
//    and a pointer swap are the whole state), and writes the recorder column.  f_int never exists in memory.  No
//    floating-point atomics; every result is bitwise repeatable.  The loop is not captured in a HIP graph.
//  * The same step on one rank of a partition (saa_operator_stepper_set_shared).  Synchronised: MODE 1 is the node pass that
//    sends a shared node's sum to the interface buffer instead of updating it, and after the caller's reduction over the
//    ranks opstep_finish_kernel<ENERGY>, one lane per shared or foreign dof, updates the shared dofs.  Predicted: MODE 2
//    writes the table row over the shared dofs and into the history in the node pass itself, so a predicted step stays at
//    two launches.  Every dof of every pass is updated by opstep_update_dof, so a shared node is rounded by the finish kernel
//    exactly as the node pass would have rounded it.
//  * The energy balance (saa_operator_stepper_set_energy), ENERGY = true.  The central-difference update
//    m (d1 - 2 d0 + dn)/dt^2 + alpha m (d1 - dn)/(2 dt) + s = lambda f with s = K d0, multiplied by (d1 - dn)/2 and summed
//    over the dofs, is with the symmetry of K
//        (T + U)_{n+1/2} - (T + U)_{n-1/2} = dW_n - dD_n,
//        T_{n+1/2} = 1/2 sum m ((d1 - d0)/dt)^2,  U_{n+1/2} = 1/2 sum d1 s,  dW_n = lambda sum f (d1 - dn)/2,
//        dD_n = alpha/(4 dt) sum m (d1 - dn)^2,
//    exactly, in the discrete sense.  The node pass holds every one of these factors per lane - s in registers, where it
//    never reaches memory - so the balance costs a block reduction and one small launch per step, not another sweep over the
//    mesh.  Each lane adds its share to five sums, the block reduces them - __shfl_down over the 64 lanes of a wave, then the
//    four waves through LDS in wave order - and writes one [block][5] partial; the finish pass likewise, its partials after
//    the node pass's.  opstep_energy_final_kernel, one block: lane t sums partials t, t + 256, ... in ascending order, the
//    block reduces as above, and lane 0 adds dW, dD to the running W, D and writes the row (T, U_{n+1/2}, U_n, W, D) on a
//    recording step.  No floating-point atomics here either: the rows do not depend on how a run is split into calls.  All of
//    it sits under `if (ENERGY)` in the two kernels, so the state is the same with the balance on and off by construction and
//    the ENERGY = false instantiations carry none of it.
//  * Shares of a partition (the rows of all ranks add up to the row of the whole mesh).  A dof counts when it is free and its
//    node has elements on this rank.  Terms with m or f - T, dW, dD - carry the global mass and load, which every holder of a
//    shared node has in full: a shared node counts only on the rank whose flag owned[k] is set.  U_n = 1/2 sum d0 s is formed
//    from the rank's partial s on every holder, and the partial s add up to s.  U_{n+1/2} of a shared node: in a
//    synchronised step from the summed s of the interface buffer in the finish kernel, on the owner; in a predicted step
//    from the partial s on every holder (each with the d1 of its own table) - which is why MODE 2 sums a shared node's
//    contributions when ENERGY is set, and leaves before them when it is not.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>
#include <vector>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_p2.h"
#include "saa_p2_elem.h"

namespace saa {

namespace {

// The K action of one column on one element, given its reduced geometry (G_q = J_q^-1 and wd_q = w_q detJ_q at the four
// points of the K rule): streams the ten nodal displacements of xj (masked by `bits`) through the parametric gradients and
// writes the thirty contributions o[3 a + i] as they are formed.  Statement for statement the column body of
// p2_apply_k_kernel (saa_p2.hip, whose header explains the register shape); that kernel keeps its own text so that its
// code object stays what it was.
__device__ __forceinline__ void p2_k_column(const Rule<4> &R, const int32_t v[10], uint32_t bits, const double G[4][3][3],
                                            const double wd[4], double lam, double mu, const double *xj,
                                            double *o) {
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

}  // namespace

// Reduced geometry of every order-2 element, once: geom[(9 q + 3 i + k) n_elems + e] = (J_q^-1)[i][k],
// geom[(36 + q) n_elems + e] = w_q detJ_q, bits[e] = the element's 30 free-dof bits.
__global__ void __launch_bounds__(kThreads) opstep_geometry_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                   const int32_t *__restrict__ cells,
                                                                   const double *__restrict__ free_mask,
                                                                   double *__restrict__ geom, uint32_t *__restrict__ bits) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double p[10][3];
  bits[e] = load_element10(xyz, cells, free_mask, e, v, p);
  // coordinates relative to node 0 (sum_a dN_a = 0: J is the same): the products are of the element's size, not of the
  // mesh's, so a thin element far from the origin keeps the digits of its thin direction
#pragma unroll
  for (int a = 9; a >= 0; --a)
#pragma unroll
    for (int c = 0; c < 3; ++c) p[a][c] -= p[0][c];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double J[3][3], G[3][3];
    jacobian10(R, q, p, J);
    const double wd = R.w[q] * inverse3(J, G);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) geom[(9 * q + 3 * i + k) * (int64_t)n_elems + e] = G[i][k];
    geom[(36 + q) * (int64_t)n_elems + e] = wd;
  }
}

// K element pass, order 2, one column, geometry from the table: out[30 e + 3 corner + component].
__global__ void __launch_bounds__(kThreads) opstep_elem_p2_kernel(int32_t n_elems, const int32_t *__restrict__ cells,
                                                                  const double *__restrict__ geom,
                                                                  const uint32_t *__restrict__ bits_tab, double lam, double mu,
                                                                  const double *__restrict__ x, double *__restrict__ out) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
#pragma unroll
  for (int a = 0; a < 10; ++a) v[a] = cells[10 * e + a];
  const uint32_t bits = bits_tab[e];
  double G[4][3][3], wd[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) G[q][i][k] = geom[(9 * q + 3 * i + k) * (int64_t)n_elems + e];
    wd[q] = geom[(36 + q) * (int64_t)n_elems + e];
  }
  p2_k_column(R, v, bits, G, wd, lam, mu, x, out + 30 * e);
}

// HRZ masses of the ten nodes of element e: out[10 e + corner].
__global__ void __launch_bounds__(kThreads) opstep_hrz_mass_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                   const int32_t *__restrict__ cells, double rho,
                                                                   double *__restrict__ out) {
  constexpr Rule<14> R = make_rule14();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[10];
  double p[10][3], wd[14], vol = 0.0;
  load_element10(xyz, cells, nullptr, e, v, p);
#pragma unroll
  for (int q = 0; q < 14; ++q) {
    double J[3][3];
    jacobian10(R, q, p, J);
    wd[q] = R.w[q] * det3(J);
    vol += wd[q];
  }
  double I[10], total = 0.0;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 14; ++q)
      if (R.N[q][a] != 0.0) s += wd[q] * (R.N[q][a] * R.N[q][a]);
    I[a] = s;
    total += s;
  }
  const double scale = rho * vol / total;
#pragma unroll
  for (int a = 0; a < 10; ++a) out[10 * e + a] = scale * I[a];
}

// Row-sum masses of the linear element: out[4 e + corner] = rho V_e / 4, V_e = detJ / 6 signed like saa_setup_fields'.
__global__ void __launch_bounds__(kThreads) opstep_p1_mass_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                  const int32_t *__restrict__ tets, double rho,
                                                                  double *__restrict__ out) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[4];
  double g[4][3];
  const double m = rho * (element_gradients(xyz, tets, e, v, g) / 6.0) / 4.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) out[4 * e + a] = m;
}

// mass[3 v + c] = sum of node v's entries of contrib[pair] in ascending element order; no Dirichlet mask.
__global__ void __launch_bounds__(kThreads) opstep_mass_node_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                    const int32_t *__restrict__ pairs,
                                                                    const double *__restrict__ contrib, double *__restrict__ mass) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes) return;
  double s = 0.0;
  for (int64_t i = offsets[v]; i < offsets[v + 1]; ++i) s += contrib[pairs[i]];
  mass[3 * v] = mass[3 * v + 1] = mass[3 * v + 2] = s;
}

// *count += number of nodes with an element whose mass is not > 0 on some dof (NaN counts)
__global__ void __launch_bounds__(kThreads) opstep_mass_check_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                     const double *__restrict__ mass, int32_t *__restrict__ count) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes || offsets[v + 1] == offsets[v]) return;
  if (!(mass[3 * v] > 0.0 && mass[3 * v + 1] > 0.0 && mass[3 * v + 2] > 0.0)) atomicAdd(count, 1);
}

// ---- the node pass and the finish pass ---------------------------------------------------------------------------------

// The update of one dof, Dynamic_solver.py:13-20, shared by the node pass and the finish pass, so that a shared node is
// rounded by the finish kernel exactly as the node pass would have rounded it.
__device__ __forceinline__ double opstep_update_dof(bool live, double s, double fi, double m, double x0, double xn, double dt,
                                                    double alpha, double scale) {
  const double num = dt * dt * (scale * fi - s) + 2.0 * m * x0 - m * xn + 0.5 * dt * m * alpha * xn;
  const double den = m + alpha * m * 0.5 * dt;
  return live ? num / den : 0.0;
}

constexpr int kCols = 5;  // of the energy balance: T_{n+1/2}, U_{n+1/2}, U_n, dW (row: W), dD (row: D)

namespace {

// One dof's share of the balance.  `mass_terms`: this rank counts T, dW and dD of the dof.
__device__ __forceinline__ void energy_add(double (&e)[kCols], bool mass_terms, double s, double fi, double m, double x0, double xn,
                                           double d1, double dt, double alpha, double scale) {
  const double v = (d1 - x0) / dt, w = d1 - xn;
  if (mass_terms) {
    e[0] += 0.5 * m * (v * v);
    e[3] += scale * fi * (0.5 * w);
    e[4] += alpha / (4.0 * dt) * m * (w * w);
  }
  e[1] += 0.5 * d1 * s;
}

// The sums of e[] over the block, valid in lanes 0 .. kCols - 1 of the return value: a wave by __shfl_down (lanes past the
// data hold 0), the waves through LDS in wave order.  Every lane of the block must call it.
__device__ __forceinline__ double block_sum(double (&e)[kCols]) {
  __shared__ double lds[kWaves][kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e[c] += __shfl_down(e[c], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) lds[wave][c] = e[c];
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < kCols) {
    t = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += lds[w][threadIdx.x];
  }
  return t;
}

}  // namespace

// Node pass fused with the update, either order, one lane per node: f_int = the node's contributions in ascending element
// order,
//   d1 = (dt^2 (scale f - f_int) + 2 m d0 - m dn + dt/2 m alpha dn) / (m + alpha m dt / 2)     (opstep_update_dof),
// 0 on Dirichlet dofs and at a node without elements; d1 replaces dn, and goes to column `col` of the row-major
// (3 n_nodes, n_cols) recorder when col >= 0.  MODE 0 is the whole mesh.  MODE 1 and 2 are one rank of a partition, where a
// node with k = shared_of[v] >= 0 is the k-th of the rank's shared list:
//   MODE 1 (step_begin): its summed contributions go to iface[3 slot[k] + c]; dn and the recorder are left alone, because d1
//     overwrites dn in place and the true d1 needs the other ranks' sums (opstep_finish_kernel);
//   MODE 2 (predicted): d1 = table_row[3 k + c] unconditionally, a Dirichlet dof included (halo_overwrite_kernel,
//     Online_predictor.py:298), recorded in hist_row (:301) and in the recorder column.
// ENERGY: the block's five sums go to partial[kCols blockIdx.x + ...]; no lane returns before block_sum.
template <int MODE, bool ENERGY>
__global__ void __launch_bounds__(kThreads) opstep_node_kernel(
    int32_t n_nodes, const int64_t *__restrict__ offsets, const int32_t *__restrict__ pairs, const double *__restrict__ free_mask,
    const double *__restrict__ contrib, const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ d0,
    double *__restrict__ dn, double dt, double alpha, double scale, double *__restrict__ traj, int64_t n_cols, int64_t col,
    const int32_t *__restrict__ shared_of, const int32_t *__restrict__ slot, double *__restrict__ iface,
    const double *__restrict__ table_row, double *__restrict__ hist_row, const uint8_t *__restrict__ owned,
    double *__restrict__ partial) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (v < n_nodes) {
    const int32_t k = MODE == 0 ? -1 : shared_of[v];
    const bool predicted = MODE == 2 && k >= 0;
    if (predicted && !ENERGY) {  // nothing of the node is needed but its table row
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t i = 3 * v + c;
        const double d1 = table_row[3 * (int64_t)k + c];
        dn[i] = d1;
        if (hist_row) hist_row[3 * (int64_t)k + c] = d1;
        if (col >= 0) traj[i * n_cols + col] = d1;
      }
      return;
    }
    const int64_t b = offsets[v], end = offsets[v + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = b; i < end; ++i) {
      const double *q = contrib + 3 * (int64_t)pairs[i];
      s[0] += q[0];
      s[1] += q[1];
      s[2] += q[2];
    }
    if (MODE == 1 && k >= 0) {
      double *o = iface + 3 * (int64_t)slot[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t i = 3 * v + c;
        o[c] = s[c];
        if (ENERGY && end > b && free_mask[i] != 0.0) e[2] += 0.5 * d0[i] * s[c];
      }
    } else {
      const bool mine = ENERGY && predicted ? owned[k] != 0 : true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t i = 3 * v + c;
        const bool live = end > b && free_mask[i] != 0.0;
        const double fi = f[i], m = mass[i], x0 = d0[i], xn = dn[i];
        double d1;
        if (ENERGY && predicted) {
          d1 = table_row[3 * (int64_t)k + c];
          if (hist_row) hist_row[3 * (int64_t)k + c] = d1;
        } else {
          d1 = opstep_update_dof(live, s[c], fi, m, x0, xn, dt, alpha, scale);  // (a node without elements: never its 0/0)
        }
        dn[i] = d1;
        if (col >= 0) traj[i * n_cols + col] = d1;
        if (ENERGY && live) {
          energy_add(e, mine, s[c], fi, m, x0, xn, d1, dt, alpha, scale);
          e[2] += 0.5 * x0 * s[c];
        }
      }
    }
  }
  if (ENERGY) {
    const double t = block_sum(e);
    if (threadIdx.x < kCols) partial[kCols * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

// After the reduction of iface over the ranks, one lane per shared dof and per foreign dof: d1 of shared dof 3 k + c from
// the summed force iface[3 slot[k] + c] (0 on a Dirichlet dof) over dn, into the recorder column and into hist_row; the
// slots of shared nodes this rank does not hold are zeroed, so that the next sum sees fresh partial forces only
// (iface_finish_kernel of saa_kernels.hip).  ENERGY: the shared dofs' share of T, U_{n+1/2} (from the summed s), dW and dD,
// on the owner.
template <bool ENERGY>
__global__ void __launch_bounds__(kThreads) opstep_finish_kernel(
    int32_t n_shared, int32_t n_foreign, const int32_t *__restrict__ node, const int32_t *__restrict__ slot,
    const int32_t *__restrict__ foreign, const int64_t *__restrict__ offsets, const double *__restrict__ free_mask,
    const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ d0, double *__restrict__ dn, double dt,
    double alpha, double scale, double *__restrict__ traj, int64_t n_cols, int64_t col, double *__restrict__ iface,
    double *__restrict__ hist_row, const uint8_t *__restrict__ owned, double *__restrict__ partial) {
  const int64_t j = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t n_local = 3 * (int64_t)n_shared;
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (j < n_local) {
    const int64_t k = j / 3;
    const int c = (int)(j - 3 * k);
    const int64_t v = node[k], i = 3 * v + c;
    const double s = iface[3 * (int64_t)slot[k] + c];
    const bool live = offsets[v + 1] > offsets[v] && free_mask[i] != 0.0;
    const double fi = f[i], m = mass[i], x0 = d0[i], xn = dn[i];
    const double d1 = opstep_update_dof(live, s, fi, m, x0, xn, dt, alpha, scale);
    dn[i] = d1;
    if (col >= 0) traj[i * n_cols + col] = d1;
    if (hist_row) hist_row[j] = d1;
    if (ENERGY && live && owned[k] != 0) energy_add(e, true, s, fi, m, x0, xn, d1, dt, alpha, scale);
  } else if (j < n_local + 3 * (int64_t)n_foreign) {
    const int64_t r = j - n_local;
    iface[3 * (int64_t)foreign[r / 3] + (r % 3)] = 0.0;
  }
  if (ENERGY) {
    const double t = block_sum(e);
    if (threadIdx.x < kCols) partial[kCols * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

// One block.  The step's sums from its n_part partials; run[0] += dW, run[1] += dD; row >= 0: energy[kCols row + ...] =
// T_{n+1/2}, U_{n+1/2}, U_n, W_{n+1}, D_{n+1}.
__global__ void __launch_bounds__(kThreads) opstep_energy_final_kernel(int32_t n_part, const double *__restrict__ partial,
                                                                       double *__restrict__ run, double *__restrict__ energy,
                                                                       int64_t row) {
  __shared__ double total[kCols];
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t b = threadIdx.x; b < n_part; b += kThreads) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) e[c] += partial[kCols * (int64_t)b + c];
  }
  const double t = block_sum(e);
  if (threadIdx.x < kCols) total[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double W = run[0] + total[3], D = run[1] + total[4];
    run[0] = W;
    run[1] = D;
    if (row >= 0) {
      double *o = energy + kCols * row;
      o[0] = total[0];
      o[1] = total[1];
      o[2] = total[2];
      o[3] = W;
      o[4] = D;
    }
  }
}

// row[3 k + c] = d[3 node[k] + c] (GATHER) or the reverse, one lane per shared dof.
template <bool GATHER>
__global__ void __launch_bounds__(kThreads) opstep_halo_kernel(int32_t n_shared, const int32_t *__restrict__ node, double *d,
                                                               double *row) {
  const int64_t j = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (j >= 3 * (int64_t)n_shared) return;
  const int64_t i = 3 * (int64_t)node[j / 3] + (j % 3);
  if (GATHER)
    row[j] = d[i];
  else
    d[i] = row[j];
}

namespace {

// frees the energy buffers and switches the balance off; the caller has made sure that nothing in flight reads them
void energy_clear(OpStepper *st) {
  void *bufs[] = {st->energy_part, st->energy_run, st->owned};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  st->energy = st->energy_part = st->energy_run = nullptr;
  st->owned = nullptr;
  st->energy_rows = st->energy_index = 0;
  st->energy_every = 1;
}

// the K element pass of one column x into contrib, by the variant the stepper is set to
hipError_t element_pass(OpStepper *st, const double *x, double *contrib) {
  ModalOp *op = st->op;
  if (st->material != 0) return opfs_element_pass(st, x, contrib);
  if (op->order != 2) return modal_elem_pass_k(op, x, contrib);
  if (!st->stored) return p2_elem_pass_k(op, x, contrib);
  if (op->n_elems == 0) return hipSuccess;
  hipLaunchKernelGGL(opstep_elem_p2_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->tets, op->geom,
                     op->bits, op->lam, op->mu, x, contrib);
  return hipGetLastError();
}

}  // namespace

hipError_t operator_geometry(ModalOp *op) {
  if (op->geom || op->order != 2) return hipSuccess;
  if (!op->bits) SAA_HIP_TRY(dev_alloc(&op->bits, static_cast<size_t>(op->n_elems)));
  SAA_HIP_TRY(dev_alloc(&op->geom, 40 * static_cast<size_t>(op->n_elems)));  // (geom set = both exist)
  if (op->n_elems > 0) {
    hipLaunchKernelGGL(opstep_geometry_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                       op->free_mask, op->geom, op->bits);
    SAA_HIP_TRY(hipGetLastError());
  }
  return hipSuccess;
}

hipError_t operator_lumped_mass(ModalOp *op, double *mass) {
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));  // (npe n_elems scalars fit one column of 3 npe n_elems)
  if (op->n_elems > 0) {
    if (op->order == 2)
      hipLaunchKernelGGL(opstep_hrz_mass_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                         op->rho, contrib);
    else
      hipLaunchKernelGGL(opstep_p1_mass_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                         op->rho, contrib);
    SAA_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(opstep_mass_node_kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs,
                     contrib, mass);
  return hipGetLastError();
}

void opstep_destroy(OpStepper *st) {
  if (!st) return;
  (void)hipSetDevice(st->op->device);
  energy_clear(st);
  void *bufs[] = {st->mass, st->f, st->buf[0], st->buf[1], st->shared_of, st->node, st->slot, st->foreign};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete st;
}

int opstep_device(const OpStepper *st) { return st->op->device; }

hipError_t opstep_create(ModalOp *op, const double *mass, const double *f_ext, double dt, double alpha, int ramp, OpStepper **out,
                         std::string &err) {
  *out = nullptr;
  OpStepper *st = new (std::nothrow) OpStepper;
  if (!st) return hipErrorOutOfMemory;
  st->op = op;
  st->dt = dt;
  st->alpha = alpha;
  st->ramp = ramp;
  const size_t n_dof = 3 * static_cast<size_t>(op->n_nodes), bytes = n_dof * sizeof(double);
  int32_t *count = nullptr;
  int32_t bad = 0;
  hipError_t e = dev_alloc(&st->mass, n_dof);
  if (e == hipSuccess) e = dev_alloc(&st->f, n_dof);
  if (e == hipSuccess) e = dev_alloc(&st->buf[0], n_dof);
  if (e == hipSuccess) e = dev_alloc(&st->buf[1], n_dof);
  if (e == hipSuccess) e = dev_alloc(&count, 1);
  if (e == hipSuccess) e = hipMemcpyAsync(st->mass, mass, bytes, hipMemcpyDeviceToDevice, op->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(st->f, f_ext, bytes, hipMemcpyDeviceToDevice, op->stream);
  if (e == hipSuccess) e = hipMemsetAsync(st->buf[0], 0, bytes, op->stream);
  if (e == hipSuccess) e = hipMemsetAsync(st->buf[1], 0, bytes, op->stream);
  if (e == hipSuccess) e = hipMemsetAsync(count, 0, sizeof(int32_t), op->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(opstep_mass_check_kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                       st->mass, count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, count, sizeof(int32_t), hipMemcpyDeviceToHost, op->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(op->stream);
  if (count) (void)hipFree(count);
  if (e == hipSuccess && bad > 0) {
    err = "saa_operator_stepper_create: the mass is not > 0 at " + std::to_string(bad) + " node(s) that have elements";
    e = hipErrorInvalidValue;
  }
  if (e == hipSuccess && st->stored) e = operator_geometry(st->op);
  if (e != hipSuccess) {
    opstep_destroy(st);
    return e;
  }
  *out = st;
  return hipSuccess;
}

hipError_t opstep_set_state(OpStepper *st, const double *d0, const double *dn, double tn) {
  const size_t bytes = 3 * static_cast<size_t>(st->op->n_nodes) * sizeof(double);
  const double *src[2] = {d0, dn};
  double *dst[2] = {st->buf[st->cur], st->buf[1 - st->cur]};
  for (int k = 0; k < 2; ++k) {
    if (src[k])
      SAA_HIP_TRY(hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyDeviceToDevice, st->op->stream));
    else
      SAA_HIP_TRY(hipMemsetAsync(dst[k], 0, bytes, st->op->stream));
  }
  st->tn = tn;
  return hipSuccess;
}

hipError_t opstep_get_state(OpStepper *st, double *d0, double *dn, double *tn) {
  const size_t bytes = 3 * static_cast<size_t>(st->op->n_nodes) * sizeof(double);
  if (d0) SAA_HIP_TRY(hipMemcpyAsync(d0, st->buf[st->cur], bytes, hipMemcpyDeviceToDevice, st->op->stream));
  if (dn) SAA_HIP_TRY(hipMemcpyAsync(dn, st->buf[1 - st->cur], bytes, hipMemcpyDeviceToDevice, st->op->stream));
  SAA_HIP_TRY(hipStreamSynchronize(st->op->stream));
  if (tn) *tn = st->tn;
  return hipSuccess;
}

void opstep_set_recorder(OpStepper *st, double *traj, int64_t n_cols, int32_t save_every, int64_t next_step_index) {
  st->traj = traj;
  st->n_cols = n_cols;
  st->save_every = save_every;
  st->step_index = next_step_index;
}

bool opstep_set_option(OpStepper *st, const char *name, double value, hipError_t *e) {
  *e = hipSuccess;
  if (std::strcmp(name, "passes") == 0 && (value == 1.0 || value == 2.0 || value == 3.0)) {
    st->passes = static_cast<int>(value);
    return true;
  }
  if (std::strcmp(name, "stored_geometry") != 0 || (value != 0.0 && value != 1.0)) return false;
  st->stored = value == 1.0 && st->op->order == 2;
  if (st->stored) *e = operator_geometry(st->op);
  return true;
}

namespace {

double ramp_scale(const OpStepper *st) { return st->ramp ? (st->tn < 1.0 ? st->tn : 1.0) : 1.0; }  // min(tn, 1), Dynamic_solver.py:13

int64_t recorder_column(const OpStepper *st) {
  if (st->traj && st->step_index % st->save_every == 0 && st->step_index / st->save_every < st->n_cols)
    return st->step_index / st->save_every;
  return -1;
}

void advance(OpStepper *st) {
  st->cur = 1 - st->cur;
  st->tn += st->dt;
  ++st->step_index;
  ++st->energy_index;
}

// shared_of of a stepper without a shared set: all -1, built on first need
hipError_t ensure_shared_map(OpStepper *st) {
  if (st->shared_of) return hipSuccess;
  const size_t n = static_cast<size_t>(st->op->n_nodes);
  SAA_HIP_TRY(dev_alloc(&st->shared_of, n));
  return hipMemsetAsync(st->shared_of, 0xff, (n ? n : 1) * sizeof(int32_t), st->op->stream);
}

int32_t node_blocks(const OpStepper *st) { return static_cast<int32_t>(opstep_grid(st->op->n_nodes).x); }
int64_t finish_lanes(const OpStepper *st) { return 3 * (static_cast<int64_t>(st->n_shared) + st->n_foreign); }

// the energy row of this step, by the recorder's rule (-1: none)
int64_t energy_row(const OpStepper *st) {
  if (st->energy_index % st->energy_every == 0 && st->energy_index / st->energy_every < st->energy_rows)
    return st->energy_index / st->energy_every;
  return -1;
}

// balance on: the step's row from its first n_part partials (node-pass blocks first, then finish blocks)
hipError_t finalise(OpStepper *st, int32_t n_part) {
  if (!st->energy) return hipSuccess;
  hipLaunchKernelGGL(opstep_energy_final_kernel, dim3(1), dim3(kThreads), 0, st->op->stream, n_part, st->energy_part, st->energy_run,
                     st->energy, energy_row(st));
  return hipGetLastError();
}

// the node pass of this step from contrib, with the energy sums when the balance is on
template <int MODE>
hipError_t node_pass(OpStepper *st, const double *contrib, const double *table_row, double *hist_row) {
  ModalOp *op = st->op;
  if (op->n_nodes == 0) return hipSuccess;
  const auto kernel = st->energy ? opstep_node_kernel<MODE, true> : opstep_node_kernel<MODE, false>;
  hipLaunchKernelGGL(kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs,
                     op->free_mask, contrib, st->mass, st->f, st->buf[st->cur], st->buf[1 - st->cur], st->dt, st->alpha, ramp_scale(st),
                     st->traj, st->n_cols, recorder_column(st), st->shared_of, st->slot, st->iface, table_row, hist_row, st->owned,
                     st->energy_part);
  return hipGetLastError();
}

}  // namespace

hipError_t opstep_step(OpStepper *st, int32_t nsteps) {
  if (nsteps <= 0) return hipSuccess;
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(st->op, 1, &contrib));
  for (int32_t k = 0; k < nsteps; ++k) {
    if (st->passes & 1) SAA_HIP_TRY(element_pass(st, st->buf[st->cur], contrib));
    if (st->passes == 1) continue;
    SAA_HIP_TRY(node_pass<0>(st, contrib, nullptr, nullptr));
    if (st->passes != 3) continue;
    SAA_HIP_TRY(finalise(st, node_blocks(st)));
    advance(st);
  }
  return hipSuccess;
}

hipError_t opstep_element_pass_at_d0(OpStepper *st, double *contrib) {
  if (st->material != 0) return opfs_element_pass_scratch(st, st->buf[st->cur], contrib);
  return element_pass(st, st->buf[st->cur], contrib);
}

double opstep_ramp_scale(const OpStepper *st) { return ramp_scale(st); }

hipError_t operator_element_masses(ModalOp *op, double *out) {
  if (op->n_elems == 0) return hipSuccess;
  if (op->order == 2)
    hipLaunchKernelGGL(opstep_hrz_mass_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                       op->rho, out);
  else
    hipLaunchKernelGGL(opstep_p1_mass_kernel, opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                       op->rho, out);
  return hipGetLastError();
}

bool opstep_pending(const OpStepper *st) { return st->pending; }
int32_t opstep_n_shared(const OpStepper *st) { return st->n_shared; }
bool opstep_lacks_interface_buffer(const OpStepper *st) { return st->n_global_shared > 0 && !st->iface; }
void opstep_set_interface_buffer(OpStepper *st, double *iface) { st->iface = iface; }
bool opstep_energy_on(const OpStepper *st) { return st->energy != nullptr; }
int opstep_passes(const OpStepper *st) { return st->passes; }

hipError_t opstep_set_energy(OpStepper *st, double *energy, int64_t n_rows, int32_t every, int64_t next_step_index,
                             const uint8_t *shared_owned) {
  ModalOp *op = st->op;
  SAA_HIP_TRY(hipStreamSynchronize(op->stream));  // the old buffers may still be read by work in flight
  energy_clear(st);
  if (!energy) return hipSuccess;
  const size_t n_part = static_cast<size_t>(node_blocks(st)) + opstep_grid(finish_lanes(st)).x;
  const size_t n_owned = st->n_shared > 0 ? static_cast<size_t>(st->n_shared) : 1;
  std::vector<uint8_t> flags(n_owned, 1);
  if (shared_owned)
    for (int32_t k = 0; k < st->n_shared; ++k) flags[k] = shared_owned[k] ? 1 : 0;
  hipError_t e = dev_alloc(&st->energy_part, n_part * kCols);
  if (e == hipSuccess) e = dev_alloc(&st->energy_run, 2);
  if (e == hipSuccess) e = dev_alloc(&st->owned, n_owned);
  if (e == hipSuccess) e = hipMemsetAsync(st->energy_run, 0, 2 * sizeof(double), op->stream);
  if (e == hipSuccess) e = hipMemcpy(st->owned, flags.data(), n_owned, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    energy_clear(st);
    return e;
  }
  st->energy = energy;
  st->energy_rows = n_rows;
  st->energy_every = every;
  st->energy_index = next_step_index;
  return hipSuccess;
}

hipError_t opstep_set_shared(OpStepper *st, int32_t n_shared, const int32_t *shared_local, const int32_t *shared_slots,
                             int32_t n_global_shared, std::string &err) {
  ModalOp *op = st->op;
  const int32_t n_nodes = op->n_nodes;
  std::vector<int32_t> of(static_cast<size_t>(n_nodes), -1), foreign;
  std::vector<char> held(static_cast<size_t>(n_global_shared), 0);
  for (int32_t k = 0; k < n_shared; ++k) {
    const int32_t v = shared_local[k], s = shared_slots[k];
    if (v < 0 || v >= n_nodes || s < 0 || s >= n_global_shared) {
      err = "saa_operator_stepper_set_shared: shared node " + std::to_string(k) + " has node id " + std::to_string(v) +
            " or slot " + std::to_string(s) + " out of range";
      return hipErrorInvalidValue;
    }
    if (of[v] >= 0 || held[s]) {
      err = "saa_operator_stepper_set_shared: node id " + std::to_string(v) + " or slot " + std::to_string(s) + " is repeated";
      return hipErrorInvalidValue;
    }
    of[v] = k;
    held[s] = 1;
  }
  for (int32_t s = 0; s < n_global_shared; ++s)
    if (!held[s]) foreign.push_back(s);
  // the old lists may still be read by work in flight
  SAA_HIP_TRY(hipStreamSynchronize(op->stream));
  energy_clear(st);  // its ownership flags and partial sums are sized by the old lists
  void *old[] = {st->shared_of, st->node, st->slot, st->foreign};
  for (void *b : old)
    if (b) (void)hipFree(b);
  st->shared_of = st->node = st->slot = st->foreign = nullptr;
  st->n_shared = st->n_foreign = st->n_global_shared = 0;
  if (n_shared == 0 && n_global_shared == 0) return hipSuccess;
  const int32_t n_foreign = static_cast<int32_t>(foreign.size());
  SAA_HIP_TRY(dev_alloc(&st->shared_of, of.size()));
  SAA_HIP_TRY(dev_alloc(&st->node, static_cast<size_t>(n_shared)));
  SAA_HIP_TRY(dev_alloc(&st->slot, static_cast<size_t>(n_shared)));
  SAA_HIP_TRY(dev_alloc(&st->foreign, foreign.size()));
  if (n_nodes > 0) SAA_HIP_TRY(hipMemcpy(st->shared_of, of.data(), of.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (n_shared > 0) {
    SAA_HIP_TRY(hipMemcpy(st->node, shared_local, static_cast<size_t>(n_shared) * sizeof(int32_t), hipMemcpyHostToDevice));
    SAA_HIP_TRY(hipMemcpy(st->slot, shared_slots, static_cast<size_t>(n_shared) * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (n_foreign > 0) SAA_HIP_TRY(hipMemcpy(st->foreign, foreign.data(), foreign.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  st->n_shared = n_shared;
  st->n_foreign = n_foreign;
  st->n_global_shared = n_global_shared;
  return hipSuccess;
}

hipError_t opstep_step_begin(OpStepper *st) {
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(st->op, 1, &contrib));
  SAA_HIP_TRY(ensure_shared_map(st));
  SAA_HIP_TRY(element_pass(st, st->buf[st->cur], contrib));
  SAA_HIP_TRY(node_pass<1>(st, contrib, nullptr, nullptr));
  st->pending = true;
  return hipSuccess;
}

hipError_t opstep_step_finish(OpStepper *st, double *hist, int64_t hist_row) {
  ModalOp *op = st->op;
  const int64_t lanes = finish_lanes(st);
  if (lanes > 0) {
    double *row = hist ? hist + hist_row * 3 * static_cast<int64_t>(st->n_shared) : nullptr;
    const auto kernel = st->energy ? opstep_finish_kernel<true> : opstep_finish_kernel<false>;
    hipLaunchKernelGGL(kernel, opstep_grid(lanes), dim3(kThreads), 0, op->stream, st->n_shared, st->n_foreign, st->node, st->slot,
                       st->foreign, op->offsets, op->free_mask, st->mass, st->f, st->buf[st->cur], st->buf[1 - st->cur], st->dt,
                       st->alpha, ramp_scale(st), st->traj, st->n_cols, recorder_column(st), st->iface, row, st->owned,
                       st->energy ? st->energy_part + kCols * static_cast<int64_t>(node_blocks(st)) : nullptr);
    SAA_HIP_TRY(hipGetLastError());
  }
  SAA_HIP_TRY(finalise(st, node_blocks(st) + static_cast<int32_t>(opstep_grid(lanes).x)));
  st->pending = false;
  advance(st);
  return hipSuccess;
}

hipError_t opstep_step_predicted(OpStepper *st, int32_t nsteps, const double *table, int64_t table_row0, double *hist,
                                 int64_t hist_row0) {
  if (nsteps <= 0) return hipSuccess;
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(st->op, 1, &contrib));
  SAA_HIP_TRY(ensure_shared_map(st));
  const int64_t width = 3 * static_cast<int64_t>(st->n_shared);
  for (int32_t k = 0; k < nsteps; ++k) {
    SAA_HIP_TRY(element_pass(st, st->buf[st->cur], contrib));
    SAA_HIP_TRY(node_pass<2>(st, contrib, width > 0 ? table + (table_row0 + k) * width : nullptr,
                            hist ? hist + (hist_row0 + k) * width : nullptr));
    SAA_HIP_TRY(finalise(st, node_blocks(st)));
    advance(st);
  }
  return hipSuccess;
}

hipError_t opstep_halo(OpStepper *st, double *row, bool gather) {
  const int64_t lanes = 3 * static_cast<int64_t>(st->n_shared);
  if (lanes == 0) return hipSuccess;
  if (gather)
    hipLaunchKernelGGL(opstep_halo_kernel<true>, opstep_grid(lanes), dim3(kThreads), 0, st->op->stream, st->n_shared, st->node,
                       st->buf[st->cur], row);
  else
    hipLaunchKernelGGL(opstep_halo_kernel<false>, opstep_grid(lanes), dim3(kThreads), 0, st->op->stream, st->n_shared, st->node,
                       st->buf[st->cur], row);
  return hipGetLastError();
}

}  // namespace saa
