// gfx950 kernels of the BLOCK tangent apply on the saa_operator handle, either element order: column j of kv is K_T(u) v_j
// for up to 16 columns of one call, the operator of saa_optan.hip (its header has the definition) with what does not depend
// on the column taken out of the column loop.  The host side is operator_tangent_apply_block of saa_opfs.hip, which owns
// the counters; everything downstream of the element pass is modal_node_sum on the m columns.
//
//  * The point law is optan_state / optan_dstress of saa_optan_dev.h, H and dH are formed as the one-column passes form
//    them, weights and sign are theirs, u and every v_j are masked to 0 on Dirichlet dofs on input.
//  * A column's result does not depend on m, on the other columns or on its place in the call: every column runs the same
//    instructions on its own data (order 1: one trip of a loop that is not unrolled; order 2: one grid row).
//  * Inversion (neo-Hooke only): an element with !(J > 0) at any of its points, NaN included, writes 0 into every column and
//    is counted ONCE per call in the counter words of the force pass (order 2: by grid row 0 alone).  Integer atomics on
//    the counters only; no floating-point atomics.
//
// Order 1.  One lane per element: the gradients, H(u), the Dirichlet mask of the twelve dofs and the state of the point law
// once, then per column twelve values of v_j, dH, dP and twelve outputs.
//
// Order 2.  The one-column pass is at 254 (St. Venant-Kirchhoff) and 242 (neo-Hooke) registers, and the state of the four
// points is 76 doubles: it cannot be held across a column loop, and a loop inside the point loop would have to keep thirty
// partial outputs per column.  The column is therefore the grid's y index and every row recomputes the state of its element:
// the body of optan_elem_p2_kernel on column blockIdx.y.  What the block saves at this order is launches and the node pass
// (one for all columns), not the state; DESIGN section 7 has the variants that were not built.
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

// Block tangent element pass, order 1: out[j * stride + 12 e + 3 corner + component] for the columns j < m.
template <int MAT>
__global__ void __launch_bounds__(kThreads) optan_block_p1_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                                  const int32_t *__restrict__ tets,
                                                                  const double *__restrict__ free_mask, double lam, double mu,
                                                                  const double *__restrict__ u, const double *__restrict__ v,
                                                                  int64_t ldv, double *__restrict__ out, int64_t stride,
                                                                  unsigned long long *__restrict__ cnt) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t id[4];
  double g[4][3];
  const double det = element_gradients(xyz, tets, e, id, g);
  const double vol = det / 6.0;  // signed, like the force pass
  double mask[4][3], h[3][3];
  {
    double w[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mask[a][c] = free_mask[3 * (int64_t)id[a] + c];
        w[a][c] = mask[a][c] * u[3 * (int64_t)id[a] + c];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) h[i][k] = w[0][i] * g[0][k] + w[1][i] * g[1][k] + w[2][i] * g[2][k] + w[3][i] * g[3][k];
  }
  double sa[3][3], sb[3][3], sc = 0.0;
  double *o = out + 12 * e;
  if (!optan_state<MAT>(h, lam, mu, sa, sb, sc)) {
#pragma unroll 1
    for (int32_t j = 0; j < m; ++j)
#pragma unroll
      for (int c = 0; c < 12; ++c) o[j * stride + c] = 0.0;
    opfs_count(cnt, 0);
    return;
  }
#pragma unroll 1
  for (int32_t j = 0; j < m; ++j) {
    const double *vj = v + j * ldv;
    double w[4][3], dh[3][3], dP[3][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) w[a][c] = mask[a][c] * vj[3 * (int64_t)id[a] + c];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dh[i][k] = w[0][i] * g[0][k] + w[1][i] * g[1][k] + w[2][i] * g[2][k] + w[3][i] * g[3][k];
    optan_dstress<MAT>(sa, sb, sc, dh, lam, mu, dP);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) dP[i][k] *= vol;
    double *oj = o + j * stride;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < 3; ++i) oj[3 * a + i] = dP[i][0] * g[a][0] + dP[i][1] * g[a][1] + dP[i][2] * g[a][2];
  }
}

// Block tangent element pass, order 2, column j = blockIdx.y: out[30 n_elems j + 30 e + 3 corner + component].  The body of
// optan_elem_p2_kernel (saa_optan.hip, whose register note explains the opaque node ids and the chained points).
template <int MAT>
__global__ void __launch_bounds__(kThreads, 2) optan_block_p2_kernel(int32_t n_elems, const int32_t *__restrict__ cells,
                                                                     const double *__restrict__ geom,
                                                                     const uint32_t *__restrict__ bits_tab, double lam, double mu,
                                                                     const double *__restrict__ u, const double *__restrict__ v,
                                                                     int64_t ldv, double *__restrict__ out,
                                                                     unsigned long long *__restrict__ cnt) {
  constexpr Rule<4> R = make_rule4();
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  // neo-Hooke has no scalar register left (106, as the one-column pass): there the column index lives in a vector register,
  // so that neither it nor a shifted pointer is held in scalar ones
  int32_t col = static_cast<int32_t>(blockIdx.y);
  if (MAT == kNeo) asm volatile("" : "+v"(col));
  const int64_t voff = col * ldv;
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
  // St. Venant-Kirchhoff has the registers to hold those of u as well
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
      const double xv = v[voff + 3 * (int64_t)id[a] + i];
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
    // neo-Hooke: the parametric gradient of u at this point alone, the ten nodes read again
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
    if (MAT == kNeo)  // dH only once ln J exists
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
  // the column's place in the scratch, formed here and per lane (the scratch's column stride is 30 n_elems)
  double *o = out + 30 * (e + col * (int64_t)n_elems);
  if (MAT == kNeo && !ok) {
#pragma unroll
    for (int j = 0; j < 30; ++j) o[j] = 0.0;
    if (col == 0) opfs_count(cnt, 0);  // once per call: every row finds the same elements
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
hipError_t launch(ModalOp *op, const double *u, int32_t m, const double *v, int64_t ldv, double *contrib, int64_t stride,
                  unsigned long long *cnt) {
  if (op->n_elems == 0) return hipSuccess;
  const dim3 grid = opstep_grid(op->n_elems);
  if (op->order == 2)
    hipLaunchKernelGGL((optan_block_p2_kernel<MAT>), dim3(grid.x, static_cast<unsigned>(m)), dim3(kThreads), 0, op->stream,
                       op->n_elems, op->tets, op->geom, op->bits, op->lam, op->mu, u, v, ldv, contrib, cnt);
  else
    hipLaunchKernelGGL((optan_block_p1_kernel<MAT>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                       op->free_mask, op->lam, op->mu, u, v, ldv, contrib, stride, cnt);
  return hipGetLastError();
}

}  // namespace

hipError_t optan_block_element_pass(ModalOp *op, int material, const double *u, int32_t m, const double *v, int64_t ldv,
                                    double *contrib, int64_t stride, unsigned long long *cnt) {
  return material == kSvk ? launch<kSvk>(op, u, m, v, ldv, contrib, stride, cnt)
                          : launch<kNeo>(op, u, m, v, ldv, contrib, stride, cnt);
}

}  // namespace saa
