// Stress recovery and error estimate of the quadratic (10-node) tetrahedron on an order-2 saa_operator handle
// (saa_stress_p2.hip): the stress at the four Gauss points of the K rule, its von Mises value and strain energy with
// their per-column totals, the recovered nodal stress and the energy norm of a stress difference per element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"

namespace saa {

// The setup kernels of stress_prepare (saa_stress.h) on an order-2 handle: |V_e| = sum_q w_q |detJ_q| into abs_vol, its
// nodal sums into node_wsum.  Enqueued on the op's stream.
hipError_t p2_stress_setup(ModalOp *op);

// 1 <= m <= kModalMaxColumns displacement columns; any output may be null.  sigma: [column][24 e + 6 q + c]; von_mises:
// [column][4 e + q]; energy: [column][e]; energy_total, von_mises_max, von_mises_argmax (a point index 4 e + q): m entries.
// Enqueued on the op's stream; arguments are validated by the caller.
hipError_t p2_stress_element(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *sigma, int64_t ld_sigma,
                             double *von_mises, int64_t ld_vm, double *energy, int64_t ld_elem, double *energy_total,
                             double *von_mises_max, int32_t *von_mises_argmax);

// sigma_node[column][6 n + c] = sum_{e at n} |V_e| c_{e,corner(n)} / sum_{e at n} |V_e| (ascending e; 0 at a node with no
// element), c the element-linear field through the four Gauss values of sigma [column][24 e + 6 q + c].
hipError_t p2_stress_nodal(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, double *sigma_node, int64_t ld_node);

// Energy norm per element of the difference between the element-linear field of sigma and either the quadratic field of
// the nodal values sigma_node [column][6 n + c] (14-point rule) or a second Gauss-point field sigma_other (4-point rule);
// exactly one of the two is non-null.  eta2: [column][e]; eta2_total, eta2_max, eta2_argmax: m entries.
hipError_t p2_stress_error(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, const double *sigma_node,
                           int64_t ld_node, const double *sigma_other, int64_t ld_other, double *eta2, int64_t ld_eta,
                           double *eta2_total, double *eta2_max, int32_t *eta2_argmax);

}  // namespace saa
