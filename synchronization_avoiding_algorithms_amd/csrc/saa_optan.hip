// gfx950 kernels of the matrix-free tangent of the finite-strain element pass (saa_opfs.hip) on the saa_operator handle, either
// element order: kv = K_T(u) v = d/ds f_int(u + s v) at s = 0, one column.  The host side is operator_tangent_apply of
// saa_opfs.hip, which owns the counters; everything downstream of the element pass is modal_node_sum.
//
//  * H = grad_X u and dH = grad_X v at the points of the K rule, both formed as the force pass forms H (order 1: the one
//    constant gradient of element_gradients; order 2: T G at the four Gauss points), u and v masked to 0 on Dirichlet dofs on
//    input.  dP, the directional derivative of the first Piola-Kirchhoff stress, takes the place of P:
//      kv_a[i] = sum_q w_q detJ_q sum_k dP_q[i][k] dN_a/dX_k(q),  weights and sign those of the force pass.
//      St. Venant-Kirchhoff:    dE = (dH + dH^T + H^T dH + dH^T H)/2, dS = lam tr(dE) I + 2 mu dE, dP = dH S + F dS
//      compressible neo-Hooke:  dP = mu dH + (mu - lam ln J) F^-T dH^T F^-T + lam (F^-T : dH) F^-T
//    F^-T - I and ln J come from H as in opfs_stress (cofactors of H, log1p(J - 1)); F^-T = I + (F^-T - I) is never taken from
//    an inverse of I + H.  At u = 0 both are the handle's K.
//  * Inversion (neo-Hooke only): an element with !(J > 0) at any of its points, NaN included, writes all its contributions as
//    0 and is counted, by the rule and in the counter words of the force pass.  No floating-point atomics.
//  * H(u) is recomputed on every apply; nothing per point is stored between applies.
//
// Register note (order 2).  The force pass holds T[4][3][3] of its one column and sits at 237 registers under neo-Hooke.  Here
// the 36 parametric gradients of v are held (they are overwritten point by point with w detJ dP G^T, as the force pass
// overwrites T).  St. Venant-Kirchhoff has room for the 36 of u next to them (254 registers, two waves) and gathers u once.
// Neo-Hooke has not: the parametric gradient of u exists for one point at a time, each point reads the ten nodes' u again -
// they sit in L1/L2 - through node ids made opaque by an empty asm, so that the compiler cannot keep the thirty values, and
// every point's ids and geometry index depend on ALL nine results of the point before, so that two points are never
// interleaved (with three of the nine: 34 spilled registers; saa_stress_p2.hip has the same device).  dH of a point is formed
// after ln J, from values that are live anyway.  242 registers, two waves, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opfs_dev.h"
#include "saa_optan_dev.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_p2.h"
#include "saa_p2_elem.h"

namespace saa {

// Tangent element pass, order 1, one column: out[12 e + 3 corner + component].
template <int MAT>
__global__ void __launch_bounds__(kThreads) optan_elem_p1_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                                 const int32_t *__restrict__ tets, const double *__restrict__ free_mask,
                                                                 double lam, double mu, const double *__restrict__ u,
                                                                 const double *__restrict__ v, double *__restrict__ out,
                                                                 unsigned long long *__restrict__ cnt) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t id[4];
  double g[4][3];
  const double det = element_gradients(xyz, tets, e, id, g);
  const double vol = det / 6.0;  // signed, like the force pass
  double h[3][3], dh[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) h[i][k] = dh[i][k] = 0.0;
  {
    double w[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) w[a][c] = free_mask[3 * (int64_t)id[a] + c] * u[3 * (int64_t)id[a] + c];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) h[i][k] = w[0][i] * g[0][k] + w[1][i] * g[1][k] + w[2][i] * g[2][k] + w[3][i] * g[3][k];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) w[a][c] = free_mask[3 * (int64_t)id[a] + c] * v[3 * (int64_t)id[a] + c];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dh[i][k] = w[0][i] * g[0][k] + w[1][i] * g[1][k] + w[2][i] * g[2][k] + w[3][i] * g[3][k];
  }
  double sa[3][3], sb[3][3], sc = 0.0, dP[3][3];
  double *o = out + 12 * e;
  if (!optan_state<MAT>(h, lam, mu, sa, sb, sc)) {
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0.0;
    opfs_count(cnt, 0);
    return;
  }
  optan_dstress<MAT>(sa, sb, sc, dh, lam, mu, dP);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) dP[i][k] *= vol;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[3 * a + i] = dP[i][0] * g[a][0] + dP[i][1] * g[a][1] + dP[i][2] * g[a][2];
}

// Tangent element pass, order 2, one column, geometry from the handle's table: out[30 e + 3 corner + component].  The body of
// opfs_elem_p2_kernel with dP in the place of P; T holds the parametric gradients of v, those of u exist per point (register
// note above).
template <int MAT>
__global__ void __launch_bounds__(kThreads, 2) optan_elem_p2_kernel(int32_t n_elems, const int32_t *__restrict__ cells,
                                                                    const double *__restrict__ geom,
                                                                    const uint32_t *__restrict__ bits_tab, double lam, double mu,
                                                                    const double *__restrict__ u, const double *__restrict__ v,
                                                                    double *__restrict__ out, unsigned long long *__restrict__ cnt) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  const uint32_t bits = bits_tab[e];
  int32_t id[10];
#pragma unroll
  for (int a = 0; a < 10; ++a) id[a] = cells[10 * e + a];
  // parametric gradients of v at the four points: T[q][i][k] = sum_a v_a[i] dN_a/dxi_k(q)
  double T[4][3][3];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) T[q][i][k] = 0.0;
  // St. Venant-Kirchhoff has the registers to hold those of u as well (register note)
  constexpr bool kOnce = MAT == kSvk;
  double TU[kOnce ? 4 : 1][3][3];
#pragma unroll
  for (int q = 0; q < (kOnce ? 4 : 1); ++q)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) TU[q][i][k] = 0.0;
#pragma unroll
  for (int a = 0; a < 10; ++a) {
    double w[3], wu[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double xv = v[3 * (int64_t)id[a] + i];
      w[i] = (bits >> (3 * a + i)) & 1u ? xv : 0.0;
      if (kOnce) {
        const double xu = u[3 * (int64_t)id[a] + i];
        wu[i] = (bits >> (3 * a + i)) & 1u ? xu : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (R.dN[q][a][k] != 0.0) {
            T[q][i][k] += w[i] * R.dN[q][a][k];
            if (kOnce) TU[q][i][k] += wu[i] * R.dN[q][a][k];
          }
  }
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // the parametric gradient of u at this point alone, the ten nodes read again (register note)
    double Tu[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) Tu[i][k] = kOnce ? TU[kOnce ? q : 0][i][k] : 0.0;
#pragma unroll
    for (int a = 0; a < 10; ++a) {
      if (kOnce) break;
      if (!(R.dN[q][a][0] != 0.0 || R.dN[q][a][1] != 0.0 || R.dN[q][a][2] != 0.0)) continue;
      int32_t va = id[a];
      if (q > 0)
        asm volatile("" : "+v"(va) : "v"(T[q - 1][0][0]), "v"(T[q - 1][0][1]), "v"(T[q - 1][0][2]), "v"(T[q - 1][1][0]), "v"(T[q - 1][1][1]),
                       "v"(T[q - 1][1][2]), "v"(T[q - 1][2][0]), "v"(T[q - 1][2][1]), "v"(T[q - 1][2][2]));
      else
        asm volatile("" : "+v"(va));
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double xv = u[3 * (int64_t)va + i];
        const double ui = (bits >> (3 * a + i)) & 1u ? xv : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (R.dN[q][a][k] != 0.0) Tu[i][k] += ui * R.dN[q][a][k];
      }
    }
    double G[3][3], h[3][3];
    int32_t eo = static_cast<int32_t>(e);
    if (kOnce) {
    } else if (q > 0)
      asm volatile("" : "+v"(eo) : "v"(T[q - 1][0][0]), "v"(T[q - 1][0][1]), "v"(T[q - 1][0][2]), "v"(T[q - 1][1][0]), "v"(T[q - 1][1][1]),
                       "v"(T[q - 1][1][2]), "v"(T[q - 1][2][0]), "v"(T[q - 1][2][1]), "v"(T[q - 1][2][2]));
    else
      asm volatile("" : "+v"(eo));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) G[i][k] = geom[(9 * q + 3 * i + k) * (int64_t)n_elems + eo];
    const double wd = geom[(36 + q) * (int64_t)n_elems + eo];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) h[i][k] = Tu[i][0] * G[0][k] + Tu[i][1] * G[1][k] + Tu[i][2] * G[2][k];
    double sa[3][3], sb[3][3], sc = 0.0, dh[3][3], dP[3][3];
    ok = optan_state<MAT>(h, lam, mu, sa, sb, sc) && ok;
    if (MAT == kNeo)  // dH only once ln J exists (register note)
      asm volatile("" : "+v"(T[q][0][0]), "+v"(T[q][1][0]), "+v"(T[q][2][0]) : "v"(sc));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dh[i][k] = T[q][i][0] * G[0][k] + T[q][i][1] * G[1][k] + T[q][i][2] * G[2][k];
    optan_dstress<MAT>(sa, sb, sc, dh, lam, mu, dP);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dP[i][k] *= wd;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) T[q][i][k] = dP[i][0] * G[k][0] + dP[i][1] * G[k][1] + dP[i][2] * G[k][2];
  }
  double *o = out + 30 * e;
  if (MAT == kNeo && !ok) {
#pragma unroll
    for (int j = 0; j < 30; ++j) o[j] = 0.0;
    opfs_count(cnt, 0);
    return;
  }
  // kv_a[i] = sum_q sum_k T[q][i][k] dN_a/dxi_k(q)
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

namespace {

template <int MAT>
hipError_t launch(ModalOp *op, const double *u, const double *v, double *contrib, unsigned long long *cnt) {
  if (op->n_elems == 0) return hipSuccess;
  if (op->order == 2)
    hipLaunchKernelGGL((optan_elem_p2_kernel<MAT>), opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->tets,
                       op->geom, op->bits, op->lam, op->mu, u, v, contrib, cnt);
  else
    hipLaunchKernelGGL((optan_elem_p1_kernel<MAT>), opstep_grid(op->n_elems), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz,
                       op->tets, op->free_mask, op->lam, op->mu, u, v, contrib, cnt);
  return hipGetLastError();
}

}  // namespace

hipError_t optan_element_pass(ModalOp *op, int material, const double *u, const double *v, double *contrib,
                              unsigned long long *cnt) {
  return material == kSvk ? launch<kSvk>(op, u, v, contrib, cnt) : launch<kNeo>(op, u, v, contrib, cnt);
}

}  // namespace saa
