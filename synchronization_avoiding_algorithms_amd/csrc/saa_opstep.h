// Explicit dynamics on the saa_operator handle (saa_opstep.hip): the lumped mass of either element order and a stepper
// that runs the damped central-difference update of Tools/Dynamic_solver.py:12-20 on one whole mesh in two launches per
// step.  It exists for the quadratic element, for which there is no other time loop; on an order-1 handle it is NOT a
// rival of the LDS-resident step kernel of saa_kernels.hip (one launch per several steps, the partition kept on chip) -
// it is there so that one stepper serves both orders and the production kernel is a second oracle for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "saa_modal.h"

namespace saa {

struct OpStepper;

// mass[3v + c] (c = 0..2 alike), Dirichlet mask not applied.  Order 2: HRZ lumping with the 14-point rule, per element
// m_a = rho (sum_q w_q detJ_q) I_a / sum_b I_b, I_a = sum_q w_q detJ_q N_a(xi_q)^2.  Order 1: rho V_e / 4 per vertex.  An
// element pass and a nodal sum in ascending element order; enqueued on the op's stream.
hipError_t operator_lumped_mass(ModalOp *op, double *mass);

// Copies mass and load (3 * n_nodes device doubles each), allocates the two state buffers (zero) and, for an order-2
// handle, the geometry table.  Synchronises once to check the mass: err is set (and hipErrorInvalidValue returned) when it
// is not > 0 at a node that has elements.
hipError_t opstep_create(ModalOp *op, const double *mass, const double *f_ext, double dt, double alpha, int ramp,
                         OpStepper **out, std::string &err);
void opstep_destroy(OpStepper *st);
int opstep_device(const OpStepper *st);

// NULL = zeros.  Enqueued on the op's stream.
hipError_t opstep_set_state(OpStepper *st, const double *d0, const double *dn, double tn);
// Either pointer may be NULL.  Synchronises the op's stream.
hipError_t opstep_get_state(OpStepper *st, double *d0, double *dn, double *tn);
// The meaning of saa_set_recorder: row-major (3 * n_nodes, n_cols), step index i goes to column i / save_every when
// i % save_every == 0 and the column exists; traj = NULL switches it off.
void opstep_set_recorder(OpStepper *st, double *traj, int64_t n_cols, int32_t save_every, int64_t next_step_index);
// "stored_geometry" 1 / 0: the order-2 element pass reads J^-1 and w detJ of its four points from the table built once
// ([40][n_elems] doubles) / recomputes them from the thirty coordinates every step.  "passes" 3 / 1 / 2: a measurement aid
// (tools/p2_step_point.py) - a step launches both passes / the element pass only / the node pass only, and only with 3
// does the state advance.  false: unknown name or value.
bool opstep_set_option(OpStepper *st, const char *name, double value, hipError_t *e);
hipError_t opstep_step(OpStepper *st, int32_t nsteps);

}  // namespace saa
