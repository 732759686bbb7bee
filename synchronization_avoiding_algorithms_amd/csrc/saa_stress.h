// Stress recovery on the saa_operator handle (saa_stress.hip): element stress, von Mises, strain energy and their
// per-column totals, the volume-weighted nodal average of element fields, and the energy norm of a stress difference per
// element (the Zienkiewicz-Zhu error estimate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"

namespace saa {

constexpr int kStressMaxComponents = 8;

int32_t modal_n_elems(const ModalOp *op);

// Shared by both element orders (saa_stress.hip, saa_stress_p2.hip).  stress_prepare: on the handle's first stress call,
// abs_vol, node_wsum and the partial buffers [column][workgroup], one workgroup per 256 elements (freed by modal_destroy),
// and the two setup kernels of the handle's order that fill abs_vol and node_wsum; nothing stays allocated when it fails.
// stress_reduce_partials: the handle's partials folded in a fixed order, one workgroup per column, into m totals, maxima
// and lowest argmaxima (each may be null; -1 and 0.0 when no partial holds a value).  Enqueued on the op's stream.
hipError_t stress_prepare(ModalOp *op);
hipError_t stress_reduce_partials(ModalOp *op, int32_t m, double *total, double *best, int32_t *argbest);

// 16-byte loads and stores of the six-double rows of m columns: base and column stride both multiples of 16 bytes
inline bool wide_rows(const double *p, int64_t ld, int32_t m) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (m == 1 || ld % 2 == 0);
}

// 1 <= m <= kModalMaxColumns displacement columns; any output may be null.  sigma: [column][6 e + c]; von_mises, energy:
// [column][e]; energy_total, von_mises_max, von_mises_argmax: m entries.  Enqueued on the op's stream; arguments are
// validated by the caller.
hipError_t stress_element(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *sigma, int64_t ld_sigma,
                          double *von_mises, double *energy, int64_t ld_elem, double *energy_total, double *von_mises_max,
                          int32_t *von_mises_argmax);

// node[column][k v + c] = sum_{e at v} |V_e| elem[column][k e + c] / sum_{e at v} |V_e| (ascending e; 0 at a node with
// no element) for 1 <= k <= kStressMaxComponents.  Enqueued on the op's stream.
hipError_t stress_nodal_average(ModalOp *op, int32_t m, int32_t k, const double *elem, int64_t ld_elem, double *node,
                                int64_t ld_node);

// The compliance C = D^-1 of the error norm exists: mu > 0 and 3 lambda + 2 mu > 0.
bool stress_has_compliance(const ModalOp *op);

// Energy norm of the difference between the element stress sigma [column][6 e + c] and either the piecewise-linear field
// of the nodal values sigma_node [column][6 v + c] (the Zienkiewicz-Zhu estimate) or a second element field sigma_other
// [column][6 e + c]; exactly one of the two is non-null.  eta2: [column][e]; eta2_total, eta2_max, eta2_argmax: m entries;
// any output may be null.  Enqueued on the op's stream; arguments are validated by the caller.
hipError_t stress_error(ModalOp *op, int32_t m, const double *sigma, int64_t ld_sigma, const double *sigma_node, int64_t ld_node,
                        const double *sigma_other, int64_t ld_other, double *eta2, int64_t ld_eta, double *eta2_total,
                        double *eta2_max, int32_t *eta2_argmax);

}  // namespace saa
