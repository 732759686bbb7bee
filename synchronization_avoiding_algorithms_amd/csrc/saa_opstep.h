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

// One rank of a partition.  shared_local[k] = local node id of the rank's k-th shared node, shared_slots[k] = its place in the
// sorted Global_shared (both host arrays, n_shared entries); a table or history row is 3 * n_shared doubles in that order.
// Builds on the device the map node -> k (-1: not shared), the two lists and the list of foreign slots (those of the
// n_global_shared that this rank does not hold).  Ids out of range or repeated: err is set, hipErrorInvalidValue.
// n_shared = n_global_shared = 0 clears the set.  Synchronises the stream.
hipError_t opstep_set_shared(OpStepper *st, int32_t n_shared, const int32_t *shared_local, const int32_t *shared_slots,
                             int32_t n_global_shared, std::string &err);
void opstep_set_interface_buffer(OpStepper *st, double *iface);  // 3 * n_global_shared device doubles, caller-owned
bool opstep_pending(const OpStepper *st);                        // between step_begin and step_finish
int32_t opstep_n_shared(const OpStepper *st);
bool opstep_lacks_interface_buffer(const OpStepper *st);         // there are global shared slots and no buffer
// The synchronised step around the caller's reduction of the interface buffer.  begin: element pass of d0 and the node pass
// in which a shared node's summed contributions go to iface[3 slot + c] and its dn entry is left alone (d1 overwrites dn in
// place, so there is no provisional update).  finish: one launch over the shared dofs and foreign slots - d1 from the
// summed iface over dn, into the recorder column and row hist_row of hist (3 * n_shared wide, NULL: none); foreign slots
// zeroed; then swap, tn += dt, step index + 1.  Both ignore the "passes" option.
hipError_t opstep_step_begin(OpStepper *st);
hipError_t opstep_step_finish(OpStepper *st, double *hist, int64_t hist_row);
// nsteps steps of two launches: shared dofs take table[(table_row0 + k) * 3 n_shared + ...] unconditionally (Dirichlet dofs
// too), which also goes to row hist_row0 + k of hist and to the recorder; other nodes as opstep_step.
hipError_t opstep_step_predicted(OpStepper *st, int32_t nsteps, const double *table, int64_t table_row0, double *hist,
                                 int64_t hist_row0);
// gather: row[3 k + c] = d0[3 node_k + c]; else the reverse.
hipError_t opstep_halo(OpStepper *st, double *row, bool gather);

// The energy balance (saa_opstep.hip states the identity and the shares of a partition).  energy: device, row-major
// (n_rows, 5) = T_{n+1/2}, U_{n+1/2}, U_n, W, D, the row of energy step index i at i / every when i % every == 0 and the row
// exists; NULL switches the balance off.  shared_owned: n_shared host bytes (NULL: all owned).  While it is on, step, step_begin
// / step_finish and step_predicted launch the ENERGY instantiations of the node and finish passes (same state, bit for bit)
// and one more one-block kernel per step.  Zeroes the running W, D.  Synchronises the stream.  opstep_set_shared switches it
// off.  With a shared set, opstep_step counts every node of the rank as owned.
hipError_t opstep_set_energy(OpStepper *st, double *energy, int64_t n_rows, int32_t every, int64_t next_step_index,
                             const uint8_t *shared_owned);
bool opstep_energy_on(const OpStepper *st);
int opstep_passes(const OpStepper *st);  // the "passes" option

// Finite strain (saa_opfs.hip, which states the materials).  material 0 / 1 / 2 = linear / St. Venant-Kirchhoff / compressible
// neo-Hooke, validated by the caller.
// f = the internal force of one column x (0 on Dirichlet dofs): the element pass and modal_node_sum.  material 0: the linear
// passes of saa_operator_apply, energy_elem must be NULL.  energy_elem (n_elems device doubles or NULL) = sum_q w_q |detJ_q|
// W(F_q).  n_inverted (host, or NULL): neo-Hooke elements with !(det F > 0) at a point, which contributed 0; reading it
// synchronises the stream.  An order-2 handle makes its geometry table on first need.
hipError_t operator_internal_force(ModalOp *op, int material, const double *x, double *f, double *energy_elem, int64_t *n_inverted);
// kv = K_T(u) v, the tangent of that force at u applied to one column v (both masked on input, kv 0 on Dirichlet dofs): the
// element pass of saa_optan.hip and modal_node_sum.  material 0: operator_internal_force of v (u is not looked at).
// n_inverted as above.
hipError_t operator_tangent_apply(ModalOp *op, int material, const double *u, const double *v, double *kv, int64_t *n_inverted);
// kv + j * ldkv = K_T(u) (v + j * ldv) for the m <= 16 columns of one call: the element pass of saa_optan_block.hip into m
// columns of the contributions scratch and one modal_node_sum.  material 0: the K passes of saa_operator_apply on the m
// columns (u is not looked at).  n_inverted as above, an element counted once whatever m.
hipError_t operator_tangent_apply_block(ModalOp *op, int material, const double *u, int32_t m, const double *v, int64_t ldv,
                                        double *kv, int64_t ldkv, int64_t *n_inverted);
// The stepper's element pass becomes that of `material` (0: the linear pass the "stored_geometry" option selects); makes
// the handle's geometry table and the stepper's two inversion counters on first need and clears the counters.
hipError_t opstep_set_material(OpStepper *st, int material);
int opstep_material(const OpStepper *st);
// count = (element, step) inversion events since the counters were cleared, first_step = the lowest step index of one
// (-1: none).  Synchronises the stream.
hipError_t opstep_inverted(OpStepper *st, int64_t *count, int64_t *first_step);
hipError_t opstep_clear_inverted(OpStepper *st);  // enqueued
void opfs_release(OpStepper *st);                 // frees the counters; before opstep_destroy


// Following the time step at finite strain (saa_opdt.hip, which states the bound and the change of step).
// omega_e (n_elems device doubles or NULL), *omega_max and *argmax (0 and -1 when no element enters the maximum), counts (3
// host words or NULL: detJ <= 0 at a point; neo-Hooke !(J > 0) at a point; omega_e not finite) of the per-element bound of
// omega_max(M_L^-1 K_T(u)); material validated by the caller, 0 ignores u.  An order-2 handle makes its geometry table on
// first need and uses the contributions scratch for the HRZ shares.  Synchronises the stream.
hipError_t operator_tangent_bound(ModalOp *op, int material, const double *u, double *omega_e, double *omega_max, int32_t *argmax,
                                  int64_t *counts);
// dn <- dn' such that the unchanged step kernels with dt_new continue the variable-step scheme; dt_new == dt: nothing.  The
// stepper's element pass at d0 (inversions into the handle's scratch counter) and one node pass; enqueued.
hipError_t opstep_set_dt(OpStepper *st, double dt_new);
bool opstep_has_shared_set(const OpStepper *st);
double opstep_alpha(const OpStepper *st);

}  // namespace saa
