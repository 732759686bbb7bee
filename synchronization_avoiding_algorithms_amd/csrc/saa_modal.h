// Modal-analysis operator (saa_modal.hip): the mesh of one whole problem on the device, in the caller's node numbering,
// with the block apply of the stiffness and the consistent mass and the element stable-frequency kernel.  Independent of
// the step plan (saa_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace saa {

struct ModalOp;

constexpr int kModalMaxColumns = 16;

// Copies the mesh to `device`, builds the node -> (element, corner) CSR on the host (counting sort: every node's entries in
// ascending element order) and factors D = L L^T.  Arguments must be validated by the caller except the factorisation
// (err is set when D is not positive definite).  order 1: `tets` holds 4 node ids per element; order 2: 10 (saa_p2.h).
hipError_t modal_create(int device, int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets,
                        const int32_t *dirichlet_dofs, int32_t n_dirichlet, double lambda_, double mu, double rho,
                        ModalOp **out, std::string &err, int order = 1);
void modal_destroy(ModalOp *op);
int modal_device(const ModalOp *op);
int32_t modal_n_nodes(const ModalOp *op);
void modal_set_stream(ModalOp *op, hipStream_t stream);

// KX and/or MX (either output may be null) for 1 <= m <= kModalMaxColumns column-major columns; enqueued on the op's stream.
hipError_t modal_apply(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *kx, double *mx, int64_t ldy);

// Element stable frequencies: optional per-element omega_e (device), max over elements and its element, count of
// elements with signed volume <= 0.  Synchronises the op's stream.
hipError_t modal_element_bound(ModalOp *op, double *omega_e, double *omega_max, int32_t *argmax, int32_t *n_nonpositive);

}  // namespace saa
