// Quadratic tetrahedra on the saa_operator handle (saa_p2.hip): the block apply of an order-2 handle, and the consistent
// load vector and the diagonals of K and M of a handle of either order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal.h"

namespace saa {

// 10 * n_elems pair indices must fit 32 bits
constexpr int32_t kP2MaxElems = INT32_MAX / 10;

int modal_order(const ModalOp *op);

// modal_apply of an order-2 handle (created by modal_create(..., order = 2)): K with the 4-point rule, M with the 14-point
// rule.  Same contract: 1 <= m <= kModalMaxColumns, either output may be null, enqueued on the op's stream.
hipError_t p2_apply(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *kx, double *mx, int64_t ldy);

// The handle's K scratch grown to `m` columns of 3 * (nodes per element) * n_elems doubles, either order.  Growing it
// synchronises the device and moves the buffer, so a caller fetches it before every use.
hipError_t operator_scratch(ModalOp *op, int32_t m, double **buf);

// The K element pass of p2_apply alone, for one column: contrib[30 e + 3 corner + component], to be summed by the caller
// (the stepper's fused node pass, saa_opstep.hip).  Enqueued on the op's stream.
hipError_t p2_elem_pass_k(ModalOp *op, const double *x, double *contrib);

// f[3v + c] = sum over elements of (fx, fy, fz)_c integral N_v dV (the K rule), 0 on Dirichlet dofs; 3 * n_nodes doubles.
hipError_t operator_load(ModalOp *op, double fx, double fy, double fz, double *f);

// diag(K) and / or diag(M) of the masked operator (0 on Dirichlet dofs); 3 * n_nodes doubles each, either may be null.
hipError_t operator_diagonal(ModalOp *op, double *diag_k, double *diag_m);

}  // namespace saa
