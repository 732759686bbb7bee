// gfx950 kernels that let the operator stepper follow its stable time step at finite strain, either element order:
// saa_operator_tangent_bound, a one-pass upper bound of omega_max of M_L^-1 K_T(u), and saa_operator_stepper_set_dt, the exact
// change of dt between two steps of the central-difference scheme.
//
//  * The bound, one element per lane.  At each point q of the K rule (order 1: one point; order 2: the four Gauss points) H =
//    grad_X u is formed as the force pass of that order forms it (u masked to 0 on Dirichlet dofs; order 2 reads the handle's
//    geometry table).  With g_a = grad_X N_a(q) and m_a the element's share of the lumped mass (order 1: rho |V_e| / 4; order
//    2: the HRZ share of opstep_hrz_mass_kernel, written into the contributions scratch by the call)
//        C_q = sum_a g_a g_a^T / m_a = R R^T  (3x3, Cholesky),  A_q = dP/dF at H (9x9, never stored),
//        T_q = (I_3 (x) R)^T A_q (I_3 (x) R):  column (j, l) is dP of the direction dh[j][k] = R[k][l] (optan_dstress on
//        the state of optan_state, nine calls), row (i, k') = sum_k dP[i][k] R[k][k'],
//        mu_q = w_q |detJ_q| max(lambda_max(T_q), 0)  (cyclic Jacobi on the upper triangle in registers),
//        omega_e = sqrt(sum_q mu_q).
//    The nonzero spectrum of M_e^-1 G_q^T A_q G_q is that of T_q, lambda_max of a sum is at most the sum of the lambda_max, and
//    the Dirichlet mask only removes rows and columns: max_e omega_e >= omega_max (Irons-Treharne, per quadrature point).
//    SAA_MATERIAL_LINEAR is the St. Venant-Kirchhoff law at H = 0 (u is not read).  Order 2 walks its four points in a rolled
//    loop, so that the unrolled Jacobi exists once in the code, and within a point its ten nodes in a loop unrolled by two:
//    a node's id, mass share and u are read again at every point (they sit in L1/L2) and its gradient comes from a constant
//    table by the two loop indices.  Unrolled over the nodes, the thirty Dirichlet-bit compares of a point are hoisted into
//    thirty scalar masks (58 spilled scalar registers), or, as integer ANDs, the thirty gathered values and their masks into
//    vector registers (17 spilled).
//  * The maximum and its element (ties: the lowest index) and three counts - elements with detJ <= 0 at a point; neo-Hooke
//    elements with !(J > 0) at a point, whose omega_e is 0 and which leave the maximum, as the force pass drops them; elements
//    whose omega_e is not finite, stored as computed and left out of the maximum - by the two-stage reduction of
//    elem_bound_kernel (saa_modal.hip): per workgroup, then one workgroup over the partials in a fixed order.  No
//    floating-point atomics; bitwise repeatable.
//  * set_dt.  With v- = (d0 - dn)/dt_old, h = (dt_old + dt_new)/2, a = (scale f - s)/m, s = f_int(d0) of the stepper's material:
//        m (v+ - v-)/h + alpha m (v+ + v-)/2 + s = scale f,   d1 = d0 + dt_new v+
//    is the variable-step scheme, and opstep_update_dof with dt_new gives that d1 when dn is replaced by dn' = d0 - dt_new v',
//        v+ = ((1/h - alpha/2) v- + a) / (1/h + alpha/2),   v' = ((1/dt_new + alpha/2) v+ - a) / (1/dt_new - alpha/2).
//    The stepper's own element pass at d0 goes into the contributions scratch and opdt_set_dt_kernel, one lane per node, sums
//    a node's contributions in ascending element order as opstep_node_kernel does and overwrites dn with dn'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opfs_dev.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_optan_dev.h"
#include "saa_p2.h"
#include "saa_p2_elem.h"
#include "saa_stress_dev.h"

namespace saa {

namespace {

// the four points of the K rule, indexed by the rolled point and node loops of the order-2 pass
__constant__ Rule<4> kRule4 = make_rule4();

// place of (p, q), p <= q, in the row-wise upper triangle of a symmetric 9x9
__host__ __device__ constexpr int tri9(int p, int q) {
  return p <= q ? 9 * p - p * (p - 1) / 2 + (q - p) : 9 * q - q * (q - 1) / 2 + (p - q);
}

// lambda_max of the symmetric 9x9 whose upper triangle is `t`, by cyclic Jacobi - jacobi_max_eig6 of saa_modal.hip at size 9.
// All indices are compile-time after unrolling, so `t` lives in registers.
__device__ __forceinline__ double jacobi_max_eig9(double (&t)[45]) {
  for (int sweep = 0; sweep < 24; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < 9; ++p) {
      diag += t[tri9(p, p)] * t[tri9(p, p)];
#pragma unroll
      for (int q = p + 1; q < 9; ++q) off += t[tri9(p, q)] * t[tri9(p, q)];
    }
    if (!(off > 1e-34 * diag)) break;  // (also ends on NaN)
#pragma unroll
    for (int p = 0; p < 8; ++p) {
#pragma unroll
      for (int q = p + 1; q < 9; ++q) {
        const double apq = t[tri9(p, q)];
        if (apq != 0.0) {
          const double theta = (t[tri9(q, q)] - t[tri9(p, p)]) / (2.0 * apq);
          const double at = fabs(theta);
          double r = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
          if (theta < 0.0) r = -r;
          const double c = 1.0 / sqrt(r * r + 1.0), s = r * c;
          t[tri9(p, p)] -= r * apq;
          t[tri9(q, q)] += r * apq;
          t[tri9(p, q)] = 0.0;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            if (k == p || k == q) continue;
            const double akp = t[tri9(k, p)], akq = t[tri9(k, q)];
            t[tri9(k, p)] = c * akp - s * akq;
            t[tri9(k, q)] = s * akp + c * akq;
          }
        }
      }
    }
  }
  double m = t[tri9(0, 0)];
#pragma unroll
  for (int p = 1; p < 9; ++p) m = t[tri9(p, p)] > m ? t[tri9(p, p)] : m;
  return m;
}

// max(lambda_max(T_q), 0) at the displacement gradient h with C_q = {xx, xy, xz, yy, yz, zz}; NaN when T_q is not finite.
// false: neo-Hooke and !(det F > 0); the value is then 0.
template <int MAT>
__device__ __forceinline__ bool opdt_point(const double h[3][3], const double C[6], double lam, double mu, double &lmax) {
  lmax = 0.0;
  double sa[3][3], sb[3][3], sc = 0.0;
  if (!optan_state<MAT>(h, lam, mu, sa, sb, sc)) return false;
  // C = R R^T, R lower triangular
  double R[3][3];
  R[0][1] = R[0][2] = R[1][2] = 0.0;
  R[0][0] = sqrt(C[0]);
  R[1][0] = C[1] / R[0][0];
  R[2][0] = C[2] / R[0][0];
  R[1][1] = sqrt(C[3] - R[1][0] * R[1][0]);
  R[2][1] = (C[4] - R[2][0] * R[1][0]) / R[1][1];
  R[2][2] = sqrt(C[5] - R[2][0] * R[2][0] - R[2][1] * R[2][1]);
  double t[45], sum = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      double dh[3][3], dP[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) dh[i][k] = i == j && k >= l ? R[k][l] : 0.0;
      optan_dstress<MAT>(sa, sb, sc, dh, lam, mu, dP);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) {
          if (3 * i + k2 > 3 * j + l) continue;  // the upper triangle: T_q is symmetric
          double s = 0.0;
#pragma unroll
          for (int k = k2; k < 3; ++k) s += dP[i][k] * R[k][k2];
          t[tri9(3 * i + k2, 3 * j + l)] = s;
          sum += fabs(s);
        }
    }
  if (!(sum < __builtin_huge_val())) {  // NaN or infinite somewhere: the Jacobi sweeps would hide it
    lmax = __builtin_nan("");
    return true;
  }
  const double m = jacobi_max_eig9(t);
  lmax = m < 0.0 ? 0.0 : m;
  return true;
}

// wave, then workgroup reduction of (max, argmax, three counts); the result is valid in thread 0
__device__ __forceinline__ void opdt_block_reduce(double &v, int32_t &i, int32_t (&cnt)[3]) {
  __shared__ double sv[kWaves];
  __shared__ int32_t si[kWaves], sc[kWaves][3];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int32_t oi = __shfl_xor(i, off, 64);
#pragma unroll
    for (int c = 0; c < 3; ++c) cnt[c] += __shfl_xor(cnt[c], off, 64);
    max_merge(v, i, ov, oi);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = v;
    si[w] = i;
#pragma unroll
    for (int c = 0; c < 3; ++c) sc[w][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) {
      max_merge(v, i, sv[k], si[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) cnt[c] += sc[k][c];
    }
  }
}

// what an element hands to the reduction: omega_e enters the maximum when it was evaluated (ok) and is finite
__device__ __forceinline__ void opdt_classify(bool ok, double w, int64_t e, double &best, int32_t &arg, int32_t (&cnt)[3]) {
  if (!ok) {
    cnt[1] = 1;
  } else if (fabs(w) < __builtin_huge_val()) {
    best = w;
    arg = static_cast<int32_t>(e);
  } else {
    cnt[2] = 1;
  }
}

__device__ __forceinline__ void opdt_write_partial(double best, int32_t arg, const int32_t (&cnt)[3], double *part_val,
                                                   int32_t *part_idx, int32_t *part_cnt) {
  if (threadIdx.x == 0) {
    part_val[blockIdx.x] = best;
    part_idx[blockIdx.x] = arg;
#pragma unroll
    for (int c = 0; c < 3; ++c) part_cnt[3 * (int64_t)blockIdx.x + c] = cnt[c];
  }
}

}  // namespace

// The bound, order 1: one point, g and detJ of element_gradients, m = rho |V_e| / 4.  u = NULL: H = 0.
template <int MAT>
__global__ void __launch_bounds__(kThreads) opdt_bound_p1_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                 const int32_t *__restrict__ tets, const double *__restrict__ free_mask,
                                                                 double lam, double mu, double rho, const double *__restrict__ u,
                                                                 double *__restrict__ omega_e, double *__restrict__ part_val,
                                                                 int32_t *__restrict__ part_idx, int32_t *__restrict__ part_cnt) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double best = -1.0;
  int32_t arg = INT32_MAX, cnt[3] = {0, 0, 0};
  if (e < n_elems) {
    int32_t id[4];
    double g[4][3];
    const double det = element_gradients(xyz, tets, e, id, g);
    cnt[0] = det > 0.0 ? 0 : 1;
    const double vol = fabs(det) / 6.0, rm = 4.0 / (rho * vol);
    double h[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) h[i][k] = 0.0;
    if (u) {
      double w[4][3];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[a][c] = free_mask[3 * (int64_t)id[a] + c] * u[3 * (int64_t)id[a] + c];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = w[0][i] * g[0][k] + w[1][i] * g[1][k] + w[2][i] * g[2][k] + w[3][i] * g[3][k];
    }
    double C[6];
    {
      int n = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = i; k < 3; ++k)
          C[n++] = rm * (g[0][i] * g[0][k] + g[1][i] * g[1][k] + g[2][i] * g[2][k] + g[3][i] * g[3][k]);
    }
    double lmax;
    const bool ok = opdt_point<MAT>(h, C, lam, mu, lmax);
    const double w = ok ? sqrt(vol * lmax) : 0.0;
    if (omega_e) omega_e[e] = w;
    opdt_classify(ok, w, e, best, arg, cnt);
  }
  opdt_block_reduce(best, arg, cnt);
  opdt_write_partial(best, arg, cnt, part_val, part_idx, part_cnt);
}

// The bound, order 2: the four points of the K rule in a rolled loop, geometry from the handle's table, elem_mass[10 e + a]
// the HRZ shares.  u = NULL: H = 0.
template <int MAT>
__global__ void __launch_bounds__(kThreads, 2) opdt_bound_p2_kernel(int32_t n_elems, const int32_t *__restrict__ cells,
                                                                    const double *__restrict__ geom,
                                                                    const uint32_t *__restrict__ bits_tab,
                                                                    const double *__restrict__ elem_mass, double lam, double mu,
                                                                    const double *__restrict__ u, double *__restrict__ omega_e,
                                                                    double *__restrict__ part_val, int32_t *__restrict__ part_idx,
                                                                    int32_t *__restrict__ part_cnt) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double best = -1.0;
  int32_t arg = INT32_MAX, cnt[3] = {0, 0, 0};
  if (e < n_elems) {
    const uint32_t bits = bits_tab[e];
    bool ok = true;
    double sum = 0.0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      // parametric gradient of u and sum_a gamma_a gamma_a^T / m_a at this point, node by node in a rolled loop: the node's
      // id, mass share and u are read again at every point (L1/L2) and its gradient comes from the constant table
      double Tu[3][3], Cp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Tu[i][k] = 0.0;
#pragma unroll 2
      for (int a = 0; a < 10; ++a) {
        const double d0 = kRule4.dN[q][a][0], d1 = kRule4.dN[q][a][1], d2 = kRule4.dN[q][a][2];
        const double rm = 1.0 / elem_mass[10 * e + a];
        Cp[0] += rm * (d0 * d0);
        Cp[1] += rm * (d0 * d1);
        Cp[2] += rm * (d0 * d2);
        Cp[3] += rm * (d1 * d1);
        Cp[4] += rm * (d1 * d2);
        Cp[5] += rm * (d2 * d2);
        if (u) {
          const int64_t va = cells[10 * e + a];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double xv = u[3 * va + i];
            const double ui = (bits >> (3 * a + i)) & 1u ? xv : 0.0;
            Tu[i][0] += ui * d0;
            Tu[i][1] += ui * d1;
            Tu[i][2] += ui * d2;
          }
        }
      }
      double G[3][3], h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) G[i][k] = geom[(9 * q + 3 * i + k) * (int64_t)n_elems + e];
      const double wd = geom[(36 + q) * (int64_t)n_elems + e];
      if (!(wd > 0.0)) cnt[0] = 1;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = Tu[i][0] * G[0][k] + Tu[i][1] * G[1][k] + Tu[i][2] * G[2][k];
      // C = G^T Cp G (g_a = G^T gamma_a)
      const double P[3][3] = {{Cp[0], Cp[1], Cp[2]}, {Cp[1], Cp[3], Cp[4]}, {Cp[2], Cp[4], Cp[5]}};
      double PG[3][3], C[6];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) PG[i][k] = P[i][0] * G[0][k] + P[i][1] * G[1][k] + P[i][2] * G[2][k];
      {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = i; k < 3; ++k) C[n++] = G[0][i] * PG[0][k] + G[1][i] * PG[1][k] + G[2][i] * PG[2][k];
      }
      double lmax;
      ok = opdt_point<MAT>(h, C, lam, mu, lmax) && ok;
      sum += fabs(wd) * lmax;
    }
    const double w = ok ? sqrt(sum) : 0.0;
    if (omega_e) omega_e[e] = w;
    opdt_classify(ok, w, e, best, arg, cnt);
  }
  opdt_block_reduce(best, arg, cnt);
  opdt_write_partial(best, arg, cnt, part_val, part_idx, part_cnt);
}

// One block: the maximum, its element and the three counts from the n_parts partials, each lane its fixed share of them.
__global__ void __launch_bounds__(kThreads) opdt_bound_final_kernel(int32_t n_parts, const double *__restrict__ part_val,
                                                                    const int32_t *__restrict__ part_idx,
                                                                    const int32_t *__restrict__ part_cnt, double *__restrict__ res_val,
                                                                    int32_t *__restrict__ res_idx, int32_t *__restrict__ res_cnt) {
  double best = -1.0;
  int32_t arg = INT32_MAX, cnt[3] = {0, 0, 0};
  for (int32_t k = threadIdx.x; k < n_parts; k += kThreads) {
    max_merge(best, arg, part_val[k], part_idx[k]);
#pragma unroll
    for (int c = 0; c < 3; ++c) cnt[c] += part_cnt[3 * (int64_t)k + c];
  }
  opdt_block_reduce(best, arg, cnt);
  if (threadIdx.x == 0) {
    res_val[0] = best;
    res_idx[0] = arg;
#pragma unroll
    for (int c = 0; c < 3; ++c) res_cnt[c] = cnt[c];
  }
}

// set_dt, one lane per node: s = the node's contributions in ascending element order (the order of opstep_node_kernel), then
// dn <- dn' = d0 - dt_new v' per dof; 0 on Dirichlet dofs and at a node without elements.
__global__ void __launch_bounds__(kThreads) opdt_set_dt_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ pairs, const double *__restrict__ free_mask,
                                                               const double *__restrict__ contrib, const double *__restrict__ mass,
                                                               const double *__restrict__ f, const double *__restrict__ d0,
                                                               double *__restrict__ dn, double dt_old, double dt_new, double alpha,
                                                               double scale) {
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
  const double rh = 2.0 / (dt_old + dt_new), rn = 1.0 / dt_new, ha = 0.5 * alpha;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t i = 3 * v + c;
    const bool live = end > b && free_mask[i] != 0.0;
    const double x0 = d0[i];
    const double vm = (x0 - dn[i]) / dt_old;
    const double a = (scale * f[i] - s[c]) / mass[i];
    const double vp = ((rh - ha) * vm + a) / (rh + ha);
    const double vq = ((rn + ha) * vp - a) / (rn - ha);
    dn[i] = live ? x0 - dt_new * vq : 0.0;  // (a node without elements: never its 0/0)
  }
}

namespace {

template <int MAT>
hipError_t launch_bound(ModalOp *op, const double *elem_mass, const double *u, double *omega_e, int32_t n_parts) {
  if (op->order == 2)
    hipLaunchKernelGGL((opdt_bound_p2_kernel<MAT>), dim3(static_cast<unsigned>(n_parts)), dim3(kThreads), 0, op->stream, op->n_elems,
                       op->tets, op->geom, op->bits, elem_mass, op->lam, op->mu, u, omega_e, op->part_val, op->part_idx, op->dt_cnt);
  else
    hipLaunchKernelGGL((opdt_bound_p1_kernel<MAT>), dim3(static_cast<unsigned>(n_parts)), dim3(kThreads), 0, op->stream, op->n_elems,
                       op->xyz, op->tets, op->free_mask, op->lam, op->mu, op->rho, u, omega_e, op->part_val, op->part_idx, op->dt_cnt);
  return hipGetLastError();
}

}  // namespace

hipError_t operator_tangent_bound(ModalOp *op, int material, const double *u, double *omega_e, double *omega_max, int32_t *argmax,
                                  int64_t *counts) {
  const int32_t n_parts = (op->n_elems + kThreads - 1) / kThreads;
  if (!op->dt_cnt) SAA_HIP_TRY(dev_alloc(&op->dt_cnt, 3 * static_cast<size_t>(n_parts) + 3));  // partials, then the totals
  int32_t *res_cnt = op->dt_cnt + 3 * static_cast<int64_t>(n_parts);
  if (n_parts > 0) {
    double *elem_mass = nullptr;
    if (op->order == 2) {
      SAA_HIP_TRY(operator_geometry(op));
      SAA_HIP_TRY(operator_scratch(op, 1, &elem_mass));  // (10 n_elems scalars fit one column of 30 n_elems)
      SAA_HIP_TRY(operator_element_masses(op, elem_mass));
    }
    // the linear operator is the St. Venant-Kirchhoff law at H = 0
    if (material == kNeo)
      SAA_HIP_TRY(launch_bound<kNeo>(op, elem_mass, u, omega_e, n_parts));
    else
      SAA_HIP_TRY(launch_bound<kSvk>(op, elem_mass, material == 0 ? nullptr : u, omega_e, n_parts));
  }
  hipLaunchKernelGGL(opdt_bound_final_kernel, dim3(1), dim3(kThreads), 0, op->stream, n_parts, op->part_val, op->part_idx, op->dt_cnt,
                     op->res_val, op->res_int, res_cnt);
  SAA_HIP_TRY(hipGetLastError());
  double val = 0.0;
  int32_t idx = 0, cnt[3] = {0, 0, 0};
  SAA_HIP_TRY(hipMemcpyAsync(&val, op->res_val, sizeof(double), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipMemcpyAsync(&idx, op->res_int, sizeof(int32_t), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipMemcpyAsync(cnt, res_cnt, sizeof(cnt), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipStreamSynchronize(op->stream));
  const bool none = idx == INT32_MAX;  // no element entered the maximum
  *omega_max = none ? 0.0 : val;
  *argmax = none ? -1 : idx;
  if (counts)
    for (int c = 0; c < 3; ++c) counts[c] = cnt[c];
  return hipSuccess;
}

bool opstep_has_shared_set(const OpStepper *st) { return st->n_shared > 0 || st->n_global_shared > 0; }
double opstep_alpha(const OpStepper *st) { return st->alpha; }

hipError_t opstep_set_dt(OpStepper *st, double dt_new) {
  ModalOp *op = st->op;
  if (dt_new == st->dt) return hipSuccess;
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  SAA_HIP_TRY(opstep_element_pass_at_d0(st, contrib));
  if (op->n_nodes > 0) {
    hipLaunchKernelGGL(opdt_set_dt_kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs,
                       op->free_mask, contrib, st->mass, st->f, st->buf[st->cur], st->buf[1 - st->cur], st->dt, dt_new, st->alpha,
                       opstep_ramp_scale(st));
    SAA_HIP_TRY(hipGetLastError());
  }
  st->dt = dt_new;
  return hipSuccess;
}

}  // namespace saa
