// Stress recovery on the saa_operator handle (saa_stress.hip): element stress, von Mises, strain energy and their
// per-column totals, and the volume-weighted nodal average of element fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"

namespace saa {

constexpr int kStressMaxComponents = 8;

int32_t modal_n_elems(const ModalOp *op);

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

}  // namespace saa
