// Implicit dynamics on the saa_operator handle (saa_opimp.hip): the shifted tangent apply K_T(u) v + s (.) v and a Newmark
// (trapezoidal) stepper whose Newton and Jacobi-PCG loops run on the device.  The element passes are the existing ones (the
// linear K passes, saa_opfs.hip, saa_optan.hip); everything downstream of them is here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "saa_modal.h"

namespace saa {

struct OpImplicit;

// what a step call reports (the fields of saa_implicit_info)
struct OpImplicitInfo {
  int32_t steps_done = 0, converged = 1, reason = 0;
  int64_t newton_iterations = 0, cg_iterations = 0;
  double residual = 0.0;
};

// out = K_T(u) v + shift (.) v (shift = NULL: K_T(u) v, bit-equal to operator_tangent_apply), 0 on Dirichlet dofs; dot (a
// device double, or NULL) = v . out by block partials and a fixed-order final sum.  material validated by the caller, 0
// ignores u.  n_inverted as operator_tangent_apply.
hipError_t operator_shifted_apply(ModalOp *op, int material, const double *u, const double *v, const double *shift, double *out,
                                  double *dot, int64_t *n_inverted);

// Copies mass and load, allocates the state and work vectors (d = v = 0, t = 0, a that of opimp_set_state there) and, for a
// nonlinear material on an order-2 handle, the geometry table.  Synchronises once to check the mass as opstep_create does.
hipError_t opimp_create(ModalOp *op, const double *mass, const double *f_ext, double dt, double alpha, int ramp, int material,
                        OpImplicit **out, std::string &err);
void opimp_destroy(OpImplicit *st);
int opimp_device(const OpImplicit *st);
// d, v (NULL = zeros) are masked on the way in; a = (scale(t) f - f_int(d) - alpha m v) / m.  Enqueued.
hipError_t opimp_set_state(OpImplicit *st, const double *d, const double *v, double t);
// Any pointer may be NULL.  Synchronises the op's stream.
hipError_t opimp_get_state(OpImplicit *st, double *d, double *v, double *a, double *t);
void opimp_set_recorder(OpImplicit *st, double *traj, int64_t n_cols, int32_t save_every, int64_t next_step_index);
// "tol", "max_newton", "max_cg", "check_every"; false: unknown name or a value out of range.
bool opimp_set_option(OpImplicit *st, const char *name, double value);
hipError_t opimp_set_dt(OpImplicit *st, double dt);  // the shift and the preconditioner only; enqueued
double opimp_alpha(const OpImplicit *st);
hipError_t opimp_step(OpImplicit *st, int32_t nsteps, OpImplicitInfo *info);

}  // namespace saa
