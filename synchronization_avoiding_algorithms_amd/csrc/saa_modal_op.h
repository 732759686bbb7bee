// Device-side definition of the saa_operator handle and the element geometry shared by its kernels: the modal
// analysis (saa_modal.hip) and the stress recovery (saa_stress.hip) evaluate every element through the same
// element_gradients, so the stress is that of the K apply.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace saa {

// workgroup size of every kernel on the handle, and its waves (the block reductions work on whole waves)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kThreads % 64 == 0, "the block reductions work on whole waves");

struct ModalOp {
  int device = 0;
  int order = 1;  // 1: 4-node elements, 2: 10-node elements (saa_p2.hip)
  int32_t n_nodes = 0, n_elems = 0;
  double lam = 0.0, mu = 0.0, rho = 0.0;
  double L[6][6] = {};  // D = L L^T (lower triangular)
  double *xyz = nullptr;        // 3 * n_nodes
  int32_t *tets = nullptr;      // 4 * n_elems (order 2: 10 * n_elems)
  double *free_mask = nullptr;  // 3 * n_nodes: 1 on free dofs, 0 on Dirichlet dofs
  int64_t *offsets = nullptr;   // n_nodes + 1
  int32_t *pairs = nullptr;     // 4 * n_elems: 4 * element + corner, grouped by node, ascending (order 2: 10 *)
  double *scratch_k = nullptr, *scratch_m = nullptr;  // 12 * n_elems * cap_columns each (order 2: 30 *)
  int32_t cap_k = 0, cap_m = 0;
  double *part_val = nullptr;   // per-workgroup maxima of the element bound
  int32_t *part_idx = nullptr, *part_cnt = nullptr;
  double *res_val = nullptr;    // final reduction: omega_max
  int32_t *res_int = nullptr;   // argmax, n_nonpositive
  hipStream_t stream = nullptr;
  // stress recovery (saa_stress.hip), made on its first call
  double *abs_vol = nullptr;     // n_elems: |detJ| / 6
  double *node_wsum = nullptr;   // n_nodes: sum of abs_vol over a node's elements, ascending element order
  double *st_part_w = nullptr;   // [column][workgroup] partial energy sums
  double *st_part_vm = nullptr;  // [column][workgroup] partial von Mises maxima
  int32_t *st_part_idx = nullptr;
  // order 2: the reduced geometry of opstep_geometry_kernel, made on first need (operator_geometry, saa_opstep.hip) - one
  // table per handle, read by the stored-geometry pass of every stepper on it and by the finite-strain passes (saa_opfs.hip)
  double *geom = nullptr;    // [40][n_elems]
  uint32_t *bits = nullptr;  // n_elems
  unsigned long long *fs_count = nullptr;  // saa_operator_internal_force: the two counter words of the call (saa_opfs.hip)
  unsigned long long *st_inverted = nullptr;  // saa_operator_stress_finite: inverted elements per column (saa_stress_fs.hip)
  int32_t *dt_cnt = nullptr;  // saa_operator_tangent_bound: [workgroup][3] partial counts, then the three totals (saa_opdt.hip)
  double *imp_part = nullptr;  // saa_operator_shifted_apply: per-workgroup partials of the dot product (saa_opimp.hip)
};

// The node pass of saa_modal.hip on any [column][pair][3] contributions of this handle's CSR: y[j][3v + c] = sum of node
// v's entries of contrib + j * stride in ascending element order, 0 on Dirichlet dofs.  Enqueued on the op's stream.
hipError_t modal_node_sum(ModalOp *op, int32_t m, const double *contrib, int64_t stride, double *y, int64_t ldy);

// The K element pass of modal_apply alone (order 1), for one column: contrib[12 e + 3 corner + component], to be summed by
// the caller (the stepper's fused node pass, saa_opstep.hip).  Enqueued on the op's stream.
hipError_t modal_elem_pass_k(ModalOp *op, const double *x, double *contrib);

// Gradients of the four shape functions (rows) and detJ; J columns are the edges x_a - x_0 (Shape_function_Deriv.py:60-67).
__device__ __forceinline__ double element_gradients(const double *__restrict__ xyz, const int32_t *__restrict__ tets,
                                                    int64_t e, int32_t v[4], double g[4][3]) {
  double p[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    v[a] = tets[4 * e + a];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[a][c] = xyz[3 * (int64_t)v[a] + c];
  }
  double e1[3], e2[3], e3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e1[c] = p[1][c] - p[0][c];
    e2[c] = p[2][c] - p[0][c];
    e3[c] = p[3][c] - p[0][c];
  }
  // rows of adj J: c1 = e2 x e3, c2 = e3 x e1, c3 = e1 x e2; grad N_a = c_a / detJ, grad N_0 = -(sum of the others)
  const double c1[3] = {e2[1] * e3[2] - e2[2] * e3[1], e2[2] * e3[0] - e2[0] * e3[2], e2[0] * e3[1] - e2[1] * e3[0]};
  const double c2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
  const double c3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double det = e1[0] * c1[0] + e1[1] * c1[1] + e1[2] * c1[2];
  const double r = 1.0 / det;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g[1][c] = c1[c] * r;
    g[2][c] = c2[c] * r;
    g[3][c] = c3[c] * r;
    g[0][c] = -(g[1][c] + g[2][c] + g[3][c]);
  }
  return det;
}

}  // namespace saa
