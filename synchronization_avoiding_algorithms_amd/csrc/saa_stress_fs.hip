// gfx950 kernels of the finite-strain stress recovery on the saa_operator handle, either element order, and the host side
// of saa_operator_stress_finite.
//
//  * H = grad_X x at the points of the K rule, formed as the force pass of that order forms it (saa_opfs.hip): order 1 the
//    one constant gradient of element_gradients, order 2 H = T G at the four Gauss points with G and w detJ from the
//    handle's geometry table (operator_geometry), so that the energy and the stress are those of the internal force to the
//    last bit of H.  x is read as given: the Dirichlet mask is not applied, as in the linear stress passes.
//  * Per point (fs_point), everything from H and never from an inverse of I + H, A = cof(H):
//      J - 1 = tr H + tr A + det H,  det_f = 1 + that,  ln J = log1p(J - 1),  G = F^-T - I = (A - H^T - (tr A + det H) I) / J
//      St. Venant-Kirchhoff:  E = (H + H^T + H^T H)/2, S = lam tr(E) I + 2 mu E, sigma = F S F^T / J
//      neo-Hooke:             S = -mu M + lam ln J (I + M) with M = G + G^T + G^T G (= C^-1 - I),
//                             sigma = (mu (H + H^T + H H^T) + lam ln J I) / J
//    and W as opfs_stress has it.  Under a rigid rotation E, M and H + H^T + H H^T vanish to the rounding of H, so both
//    measures do.  The von Mises value is that of the chosen measure, and in all four instantiations the differences of
//    the normal stresses are taken before the common pressure is added: 2 mu (E_ii - E_jj), (lam ln J - mu)(M_ii - M_jj) and
//    mu (B_ii - B_jj) / J with B = H + H^T + H H^T where the normal stresses are a multiple of a strain plus a pressure, and
//    for the Cauchy stress of St. Venant-Kirchhoff those of (2 mu F E F^T + lam tr(E) B) / J, to which lam tr(E) / J is added
//    on the diagonal afterwards (F F^T = I + B).  Differences of the finished stresses lose lam / mu times the rounding.
//  * Layouts are those of the linear passes (saa_stress.hip, saa_stress_p2.hip), so that their nodal and error kernels read
//    the fields unchanged: stress [column][6 (nq e + q) + c], von_mises and det_f [column][nq e + q], energy [column][e];
//    the (sum W_e, max von Mises, lowest point index) partials per workgroup and stress_final_kernel are theirs too.
//  * Inversion: an element with !(J > 0) at any point, NaN included, under neo-Hooke (either measure) or with the Cauchy
//    measure (either material) writes 0 to its stress, von Mises and energy of that column, stays out of the column's total
//    and maximum, and adds 1 to the column's counter word (integer atomic).  det_f always holds the computed value.  SVK with
//    PK2 does not look at J.
// One element per lane, the columns looped inside.  No floating-point atomics: bitwise repeatable, and a column's result
// does not depend on the other columns of the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opfs_dev.h"
#include "saa_opstep_impl.h"
#include "saa_p2_elem.h"
#include "saa_stress.h"
#include "saa_stress_dev.h"
#include "saa_stress_fs.h"

namespace saa {

namespace {

// Voigt row c = (vi(c), vk(c)): xx, yy, zz, yz, xz, xy
__host__ __device__ constexpr int vi(int c) { return c < 3 ? c : c == 3 ? 1 : 0; }
__host__ __device__ constexpr int vk(int c) { return c < 3 ? c : c == 5 ? 1 : 2; }

// Stress s (Voigt) of measure MEAS, its von Mises value, W and det F of material MAT at displacement gradient h.  false:
// J is looked at (neo-Hooke or Cauchy) and !(det F > 0); s, vm and W are then not to be used.
template <int MAT, int MEAS>
__device__ __forceinline__ bool fs_point(const double h[3][3], double lam, double mu, double s[6], double &vm, double &W,
                                         double &det_f) {
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
  det_f = J;
  const bool ok = (MAT == kSvk && MEAS == kStressPk2) || J > 0.0;
  const double rJ = 1.0 / J;
  double d01, d12, d20;  // differences of the normal stresses
  if (MAT == kSvk) {
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
    double ee = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) ee += E[i][k] * E[i][k];
    W = 0.5 * lam * tr * tr + mu * ee;
    const double ltr = lam * tr, mu2 = 2.0 * mu;
    if (MEAS == kStressPk2) {
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] = mu2 * E[vi(c)][vk(c)] + (c < 3 ? ltr : 0.0);
      d01 = mu2 * (E[0][0] - E[1][1]), d12 = mu2 * (E[1][1] - E[2][2]), d20 = mu2 * (E[2][2] - E[0][0]);
    } else {
      // F S F^T = 2 mu F E F^T + lam tr(E) (I + B) with B = F F^T - I = h + h^T + h h^T: the common pressure lam tr(E) / J goes
      // on the diagonal last, after the differences are taken (it is lam / mu times the rest at small strain)
      // (one row of F E at a time, E scaled by 2 mu / J first: three values live where the whole product was nine)
      const double p = ltr * rJ, f = mu2 * rJ;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = i; k < 3; ++k) {
          E[i][k] *= f;
          E[k][i] = E[i][k];
        }
      double t[6];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double r[3];  // row i of (I + h) E
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = E[i][k] + (h[i][0] * E[0][k] + h[i][1] * E[1][k] + h[i][2] * E[2][k]);
#pragma unroll
        for (int k = i; k < 3; ++k) {
          const double B = (h[i][k] + h[k][i]) + (h[i][0] * h[k][0] + h[i][1] * h[k][1] + h[i][2] * h[k][2]);
          t[i == k ? i : 6 - i - k] = (r[k] + (r[0] * h[k][0] + r[1] * h[k][1] + r[2] * h[k][2])) + p * B;
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] = t[c] + (c < 3 ? p : 0.0);
      d01 = t[0] - t[1], d12 = t[1] - t[2], d20 = t[2] - t[0];
    }
  } else {
    const double lnJ = log1p(x);
    const double llj = lam * lnJ;
    if (MEAS == kStressPk2) {
      double G[3][3];  // F^-T - I
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) G[i][k] = ((A[i][k] - h[k][i]) - (i == k ? rest : 0.0)) * rJ;
      double M[6];  // C^-1 - I = G + G^T + G^T G
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int i = vi(c), k = vk(c);
        M[c] = (G[i][k] + G[k][i]) + (G[0][i] * G[0][k] + G[1][i] * G[1][k] + G[2][i] * G[2][k]);
      }
      const double f = llj - mu;
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] = f * M[c] + (c < 3 ? llj : 0.0);
      d01 = f * (M[0] - M[1]), d12 = f * (M[1] - M[2]), d20 = f * (M[2] - M[0]);
    } else {
      double B[6];  // F F^T - I = h + h^T + h h^T
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int i = vi(c), k = vk(c);
        B[c] = (h[i][k] + h[k][i]) + (h[i][0] * h[k][0] + h[i][1] * h[k][1] + h[i][2] * h[k][2]);
      }
      const double f = mu * rJ, p = llj * rJ;
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] = f * B[c] + (c < 3 ? p : 0.0);
      d01 = f * (B[0] - B[1]), d12 = f * (B[1] - B[2]), d20 = f * (B[2] - B[0]);
    }
    // W as opfs_stress (saa_opfs.hip): through e = 2 E, which a rigid rotation leaves alone
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
  vm = sqrt(0.5 * (d01 * d01 + d12 * d12 + d20 * d20) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
  return ok;
}

}  // namespace

// Order 1: stress [column][6 e + c], von_mises / det_f / energy [column][e] (each may be null); with part_w non-null the
// per-workgroup partials [column][workgroup]; cnt non-null: cnt[column] += 1 per inverted element.
template <int MAT, int MEAS>
__global__ void __launch_bounds__(kThreads) stress_fs_p1_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                                const int32_t *__restrict__ tets, double lam, double mu,
                                                                const double *__restrict__ x, int64_t ldx,
                                                                double *__restrict__ stress, int64_t ld_stress,
                                                                double *__restrict__ von_mises, int64_t ld_vm,
                                                                double *__restrict__ det_f, int64_t ld_det,
                                                                double *__restrict__ energy, int64_t ld_elem,
                                                                double *__restrict__ part_w, double *__restrict__ part_vm,
                                                                int32_t *__restrict__ part_idx,
                                                                unsigned long long *__restrict__ cnt) {
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  int32_t v[4] = {0, 0, 0, 0};
  double g[4][3] = {};
  double abs_vol = 0.0;
  if (valid) abs_vol = fabs(element_gradients(xyz, tets, e, v, g)) / 6.0;
  for (int32_t j = 0; j < m; ++j) {
    double w = 0.0, best = -1.0;
    int32_t arg = INT32_MAX;
    if (valid) {
      const double *xj = x + j * ldx;
      double u[4][3];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) u[a][c] = xj[3 * (int64_t)v[a] + c];
      double h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = u[0][i] * g[0][k] + u[1][i] * g[1][k] + u[2][i] * g[2][k] + u[3][i] * g[3][k];
      double s[6], vm, W, J;
      const bool ok = fs_point<MAT, MEAS>(h, lam, mu, s, vm, W, J);
      if (ok) {
        w = abs_vol * W;
        best = vm;
        arg = (int32_t)e;
      } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = 0.0;
        vm = 0.0;
        if (cnt) atomicAdd(cnt + j, 1ull);
      }
      if (stress) {
        double *o = stress + j * ld_stress + 6 * e;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = s[c];
      }
      if (von_mises) von_mises[j * ld_vm + e] = vm;
      if (det_f) det_f[j * ld_det + e] = J;
      if (energy) energy[j * ld_elem + e] = w;
    }
    if (part_w) wave_partial(lds, j, w, best, arg);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

// Order 2, geometry from the handle's table geom [40][n_elems] (nine G and w detJ per point): stress [column][24 e + 6 q + c],
// von_mises / det_f [column][4 e + q], energy [column][e].  As in opfs_elem_p2_kernel the four points are worked through one
// at a time, each reading its own nine G and its w detJ (per column: kept over the columns they cost 80 registers next to
// T and the kernel spills), and are written as they come; an inverted element then overwrites its rows with 0 (the same
// lane, in program order).
template <int MAT, int MEAS>
__global__ void __launch_bounds__(kThreads, 2) stress_fs_p2_kernel(int32_t n_elems, int32_t m, const int32_t *__restrict__ cells,
                                                                   const double *__restrict__ geom, double lam, double mu,
                                                                   const double *__restrict__ x, int64_t ldx,
                                                                   double *__restrict__ stress, int64_t ld_stress,
                                                                   bool wide_stress, double *__restrict__ von_mises, int64_t ld_vm,
                                                                   double *__restrict__ det_f, int64_t ld_det,
                                                                   double *__restrict__ energy, int64_t ld_elem,
                                                                   double *__restrict__ part_w, double *__restrict__ part_vm,
                                                                   int32_t *__restrict__ part_idx,
                                                                   unsigned long long *__restrict__ cnt) {
  constexpr Rule<4> R = make_rule4();
  __shared__ PartialLds lds;
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const bool valid = e < n_elems;
  const int64_t ec = valid ? e : 0;  // (idle lanes of the last workgroup compute element 0 and write nothing)
  int32_t v[10];
#pragma unroll
  for (int a = 0; a < 10; ++a) v[a] = cells[10 * ec + a];
  // (the element's rows of the four outputs as per-lane pointers that move on by a column per turn, null for an idle lane:
  // the bases and their column offsets would be scalar registers, which this kernel runs out of)
  double *o_stress = valid && stress ? stress + 24 * e : nullptr, *o_vm = valid && von_mises ? von_mises + 4 * e : nullptr;
  double *o_det = valid && det_f ? det_f + 4 * e : nullptr, *o_energy = valid && energy ? energy + e : nullptr;
  asm volatile("" : "+v"(ld_stress), "+v"(ld_vm), "+v"(ld_det), "+v"(ld_elem), "+v"(lam), "+v"(mu), "+v"(cnt));  // (vector registers too)
  for (int32_t j = 0; j < m; ++j, x += ldx) {
    const double *xj = x;
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
      asm volatile("" : "+v"(va));  // (register note of saa_stress_p2.hip: the row offset is formed next to the load)
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
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // (register note of saa_stress_p2.hip: point q + 1 starts from the energy sum of point q, and its table row is opaque
      // there, so that its ten loads are neither hoisted out of the column loop nor issued four points at once; the row
      // stride is opaque too and the rows are walked with a per-lane pointer: forty uniform 64-bit offsets kept over the
      // column loop are eighty scalar registers, which spill)
      int64_t eq = ec, ne = n_elems;
      asm volatile("" : "+v"(eq), "+v"(ne) : "v"(w));
      const double *gp = geom + eq + 9 * q * ne;
      double G[3][3], h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          G[i][k] = *gp;
          gp += ne;
        }
      const double awd = fabs(geom[eq + (36 + q) * ne]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = T[q][i][0] * G[0][k] + T[q][i][1] * G[1][k] + T[q][i][2] * G[2][k];
      double s[6], vm, W, J;
      ok = fs_point<MAT, MEAS>(h, lam, mu, s, vm, W, J) && ok;
      w += awd * W;
      if (valid) {
        max_merge(best, arg, vm, (int32_t)(4 * e + q));
        if (o_stress) store6(o_stress + 6 * q, wide_stress, s);
        if (o_vm) o_vm[q] = vm;
        if (o_det) o_det[q] = J;
      }
    }
    if (!(MAT == kSvk && MEAS == kStressPk2) && valid && !ok) {
      const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int q = 0; q < 4; ++q) {
        if (o_stress) store6(o_stress + 6 * q, wide_stress, zero);
        if (o_vm) o_vm[q] = 0.0;
      }
      if (cnt) atomicAdd(cnt + j, 1ull);
    }
    if (!valid || !ok) w = 0.0, best = -1.0, arg = INT32_MAX;
    if (o_energy) *o_energy = w;
    if (o_stress) o_stress += ld_stress;
    if (o_vm) o_vm += ld_vm;
    if (o_det) o_det += ld_det;
    if (o_energy) o_energy += ld_elem;
    if (part_w) wave_partial(lds, j, w, best, arg);  // (uniform branch)
  }
  if (part_w) fold_partials(lds, m, part_w, part_vm, part_idx);
}

namespace {

template <int MAT, int MEAS>
hipError_t launch(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *stress, int64_t ld_stress, double *von_mises,
                  int64_t ld_vm, double *det_f, int64_t ld_det, double *energy, int64_t ld_elem, double *part_w,
                  unsigned long long *cnt) {
  const dim3 grid(static_cast<unsigned>((op->n_elems + kThreads - 1) / kThreads));
  if (op->order == 2)
    hipLaunchKernelGGL((stress_fs_p2_kernel<MAT, MEAS>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->tets, op->geom,
                       op->lam, op->mu, x, ldx, stress, ld_stress, wide_rows(stress, ld_stress, m), von_mises, ld_vm, det_f, ld_det,
                       energy, ld_elem, part_w, op->st_part_vm, op->st_part_idx, cnt);
  else
    hipLaunchKernelGGL((stress_fs_p1_kernel<MAT, MEAS>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                       op->lam, op->mu, x, ldx, stress, ld_stress, von_mises, ld_vm, det_f, ld_det, energy, ld_elem, part_w,
                       op->st_part_vm, op->st_part_idx, cnt);
  return hipGetLastError();
}

}  // namespace

hipError_t stress_finite(ModalOp *op, int material, int measure, int32_t m, const double *x, int64_t ldx, double *stress,
                         int64_t ld_stress, double *von_mises, int64_t ld_vm, double *det_f, int64_t ld_det, double *energy,
                         int64_t ld_elem, double *energy_total, double *von_mises_max, int32_t *von_mises_argmax,
                         int64_t *n_inverted) {
  const bool reduce = energy_total || von_mises_max || von_mises_argmax;
  if (!reduce && !stress && !von_mises && !det_f && !energy && !n_inverted) return hipSuccess;
  SAA_HIP_TRY(stress_prepare(op));
  SAA_HIP_TRY(operator_geometry(op));
  unsigned long long *cnt = nullptr;
  if (n_inverted) {
    if (!op->st_inverted) SAA_HIP_TRY(dev_alloc(&op->st_inverted, static_cast<size_t>(kModalMaxColumns)));
    cnt = op->st_inverted;
    SAA_HIP_TRY(hipMemsetAsync(cnt, 0, kModalMaxColumns * sizeof(unsigned long long), op->stream));
  }
  if (op->n_elems > 0) {
    double *pw = reduce ? op->st_part_w : nullptr;
#define STRESS_FS(MAT, MEAS) \
  launch<MAT, MEAS>(op, m, x, ldx, stress, ld_stress, von_mises, ld_vm, det_f, ld_det, energy, ld_elem, pw, cnt)
    if (material == kSvk)
      SAA_HIP_TRY(measure == kStressPk2 ? STRESS_FS(kSvk, kStressPk2) : STRESS_FS(kSvk, kStressCauchy));
    else
      SAA_HIP_TRY(measure == kStressPk2 ? STRESS_FS(kNeo, kStressPk2) : STRESS_FS(kNeo, kStressCauchy));
#undef STRESS_FS
  }
  if (reduce) SAA_HIP_TRY(stress_reduce_partials(op, m, energy_total, von_mises_max, von_mises_argmax));
  if (n_inverted) {
    unsigned long long host[kModalMaxColumns] = {};
    SAA_HIP_TRY(hipMemcpyAsync(host, cnt, sizeof(host), hipMemcpyDeviceToHost, op->stream));
    SAA_HIP_TRY(hipStreamSynchronize(op->stream));
    for (int32_t j = 0; j < m; ++j) n_inverted[j] = static_cast<int64_t>(host[j]);
  }
  return hipSuccess;
}

}  // namespace saa
