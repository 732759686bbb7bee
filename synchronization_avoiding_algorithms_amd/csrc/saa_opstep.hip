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
//    (b) opstep_node_update_kernel, one lane per node, sums the node's contributions through the node -> (element, corner)
//    CSR in ascending element order, forms d1 and writes it over dn (a lane touches its own node only, so two buffers and a
//    pointer swap are the whole state), and writes the recorder column.  f_int never exists in memory.  No floating-point
//    atomics; every result is bitwise repeatable.  The loop is not captured in a HIP graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>

#include "saa_modal_op.h"
#include "saa_opstep.h"
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

// Node pass fused with the update, either order: f_int = the node's contributions in ascending element order,
//   d1 = (dt^2 (scale f - f_int) + 2 m d0 - m dn + dt/2 m alpha dn) / (m + alpha m dt / 2)     (Dynamic_solver.py:13-20),
// 0 on Dirichlet dofs and at a node without elements; d1 replaces dn, and goes to column `col` of the row-major
// (3 n_nodes, n_cols) recorder when col >= 0.
__global__ void __launch_bounds__(kThreads) opstep_node_update_kernel(
    int32_t n_nodes, const int64_t *__restrict__ offsets, const int32_t *__restrict__ pairs, const double *__restrict__ free_mask,
    const double *__restrict__ contrib, const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ d0,
    double *__restrict__ dn, double dt, double alpha, double scale, double *__restrict__ traj, int64_t n_cols, int64_t col) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes) return;
  const int64_t b = offsets[v], end = offsets[v + 1];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = b; i < end; ++i) {
    const double *q = contrib + 3 * (int64_t)pairs[i];
    s[0] += q[0];
    s[1] += q[1];
    s[2] += q[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t i = 3 * v + c;
    const bool live = end > b && free_mask[i] != 0.0;
    const double m = mass[i], x0 = d0[i], xn = dn[i];
    const double num = dt * dt * (scale * f[i] - s[c]) + 2.0 * m * x0 - m * xn + 0.5 * dt * m * alpha * xn;
    const double den = m + alpha * m * 0.5 * dt;
    const double d1 = live ? num / den : 0.0;  // (a node without elements may carry mass 0: never its 0/0)
    dn[i] = d1;
    if (col >= 0) traj[i * n_cols + col] = d1;
  }
}

#define OPSTEP_TRY(expr)             \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

struct OpStepper {
  ModalOp *op = nullptr;  // borrowed: must outlive the stepper
  double *mass = nullptr, *f = nullptr;
  double *buf[2] = {nullptr, nullptr};  // buf[cur] = d0, buf[1 - cur] = dn
  int cur = 0;
  double *geom = nullptr;               // order 2, stored geometry: [40][n_elems]
  uint32_t *bits = nullptr;             // n_elems
  bool stored = false;
  int passes = 3;                       // measurement aid: 1 = element pass only, 2 = node pass only (state not advanced)
  double dt = 0.0, alpha = 0.0, tn = 0.0;
  int ramp = 1;
  double *traj = nullptr;
  int64_t n_cols = 0, step_index = 0;
  int32_t save_every = 1;
};

namespace {

dim3 grid_for(int64_t n) { return dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)); }

template <typename T>
hipError_t dev_alloc(T **p, size_t count) {
  return hipMalloc(reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T));
}

// builds the geometry table of an order-2 stepper on first need
hipError_t ensure_geometry(OpStepper *st) {
  ModalOp *op = st->op;
  if (st->geom || op->order != 2) return hipSuccess;
  OPSTEP_TRY(dev_alloc(&st->geom, 40 * static_cast<size_t>(op->n_elems)));
  OPSTEP_TRY(dev_alloc(&st->bits, static_cast<size_t>(op->n_elems)));
  if (op->n_elems > 0) {
    hipLaunchKernelGGL(opstep_geometry_kernel, grid_for(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                       op->free_mask, st->geom, st->bits);
    OPSTEP_TRY(hipGetLastError());
  }
  return hipSuccess;
}

// the K element pass of one column x into contrib, by the variant the stepper is set to
hipError_t element_pass(OpStepper *st, const double *x, double *contrib) {
  ModalOp *op = st->op;
  if (op->order != 2) return modal_elem_pass_k(op, x, contrib);
  if (!st->stored) return p2_elem_pass_k(op, x, contrib);
  if (op->n_elems == 0) return hipSuccess;
  hipLaunchKernelGGL(opstep_elem_p2_kernel, grid_for(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->tets, st->geom,
                     st->bits, op->lam, op->mu, x, contrib);
  return hipGetLastError();
}

}  // namespace

hipError_t operator_lumped_mass(ModalOp *op, double *mass) {
  double *contrib = nullptr;
  OPSTEP_TRY(operator_scratch(op, 1, &contrib));  // (npe n_elems scalars fit one column of 3 npe n_elems)
  if (op->n_elems > 0) {
    if (op->order == 2)
      hipLaunchKernelGGL(opstep_hrz_mass_kernel, grid_for(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                         op->rho, contrib);
    else
      hipLaunchKernelGGL(opstep_p1_mass_kernel, grid_for(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz, op->tets,
                         op->rho, contrib);
    OPSTEP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(opstep_mass_node_kernel, grid_for(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs,
                     contrib, mass);
  return hipGetLastError();
}

void opstep_destroy(OpStepper *st) {
  if (!st) return;
  (void)hipSetDevice(st->op->device);
  void *bufs[] = {st->mass, st->f, st->buf[0], st->buf[1], st->geom, st->bits};
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
    hipLaunchKernelGGL(opstep_mass_check_kernel, grid_for(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
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
  if (e == hipSuccess && st->stored) e = ensure_geometry(st);
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
      OPSTEP_TRY(hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyDeviceToDevice, st->op->stream));
    else
      OPSTEP_TRY(hipMemsetAsync(dst[k], 0, bytes, st->op->stream));
  }
  st->tn = tn;
  return hipSuccess;
}

hipError_t opstep_get_state(OpStepper *st, double *d0, double *dn, double *tn) {
  const size_t bytes = 3 * static_cast<size_t>(st->op->n_nodes) * sizeof(double);
  if (d0) OPSTEP_TRY(hipMemcpyAsync(d0, st->buf[st->cur], bytes, hipMemcpyDeviceToDevice, st->op->stream));
  if (dn) OPSTEP_TRY(hipMemcpyAsync(dn, st->buf[1 - st->cur], bytes, hipMemcpyDeviceToDevice, st->op->stream));
  OPSTEP_TRY(hipStreamSynchronize(st->op->stream));
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
  if (st->stored) *e = ensure_geometry(st);
  return true;
}

hipError_t opstep_step(OpStepper *st, int32_t nsteps) {
  ModalOp *op = st->op;
  if (nsteps <= 0) return hipSuccess;
  double *contrib = nullptr;
  OPSTEP_TRY(operator_scratch(op, 1, &contrib));
  for (int32_t k = 0; k < nsteps; ++k) {
    const double *d0 = st->buf[st->cur];
    if (st->passes & 1) OPSTEP_TRY(element_pass(st, d0, contrib));
    if (st->passes == 1) continue;
    const double scale = st->ramp ? (st->tn < 1.0 ? st->tn : 1.0) : 1.0;  // min(tn, 1), Dynamic_solver.py:13
    int64_t col = -1;
    if (st->traj && st->step_index % st->save_every == 0 && st->step_index / st->save_every < st->n_cols)
      col = st->step_index / st->save_every;
    hipLaunchKernelGGL(opstep_node_update_kernel, grid_for(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                       op->pairs, op->free_mask, contrib, st->mass, st->f, d0, st->buf[1 - st->cur], st->dt, st->alpha, scale, st->traj,
                       st->n_cols, col);
    OPSTEP_TRY(hipGetLastError());
    if (st->passes != 3) continue;
    st->cur = 1 - st->cur;
    st->tn += st->dt;
    ++st->step_index;
  }
  return hipSuccess;
}

}  // namespace saa
