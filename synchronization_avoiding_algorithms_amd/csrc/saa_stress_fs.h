// Finite-strain stress recovery on the saa_operator handle, either element order (saa_stress_fs.hip): the second
// Piola-Kirchhoff or the Cauchy stress of St. Venant-Kirchhoff or neo-Hooke at the points of the K rule, its von Mises
// value, det F, the stored energy per element and the per-column totals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"

namespace saa {

constexpr int kStressPk2 = 0, kStressCauchy = 1;

// 1 <= m <= kModalMaxColumns displacement columns, material kSvk or kNeo (saa_opfs_dev.h), measure kStressPk2 or
// kStressCauchy; any output may be null, and with all of them null nothing is launched.  With nq = 1 (order 1) or 4
// (order 2): stress [column][6 (nq e + q) + c]; von_mises, det_f [column][nq e + q]; energy [column][e]; energy_total,
// von_mises_max, von_mises_argmax (a point index nq e + q): m entries.  n_inverted (host, m entries or null): the
// inverted elements of each column; asking for it synchronises the op's stream, otherwise everything is enqueued on it.
// Arguments are validated by the caller.
hipError_t stress_finite(ModalOp *op, int material, int measure, int32_t m, const double *x, int64_t ldx, double *stress,
                         int64_t ld_stress, double *von_mises, int64_t ld_vm, double *det_f, int64_t ld_det, double *energy,
                         int64_t ld_elem, double *energy_total, double *von_mises_max, int32_t *von_mises_argmax,
                         int64_t *n_inverted);

}  // namespace saa
