// What the two translation units of the operator stepper share (saa_opstep.hip: the time loop; saa_opfs.hip: the element
// passes of the finite-strain materials): the stepper's state, the launch grid and the one function each calls of the other.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal_op.h"
#include "saa_opstep.h"
#include "saa_p2_elem.h"

namespace saa {

struct OpStepper {
  ModalOp *op = nullptr;  // borrowed: must outlive the stepper
  double *mass = nullptr, *f = nullptr;
  double *buf[2] = {nullptr, nullptr};  // buf[cur] = d0, buf[1 - cur] = dn
  int cur = 0;
  bool stored = false;                  // order 2: the element pass reads the handle's geometry table (op->geom, op->bits)
  int passes = 3;                       // measurement aid: 1 = element pass only, 2 = node pass only (state not advanced)
  double dt = 0.0, alpha = 0.0, tn = 0.0;
  int ramp = 1;
  double *traj = nullptr;
  int64_t n_cols = 0, step_index = 0;
  int32_t save_every = 1;
  // the partition: shared_of[v] = k for the rank's k-th shared node (else -1), node[k], slot[k] its place in Global_shared,
  // foreign[] the slots of Global_shared this rank does not hold
  int32_t n_shared = 0, n_foreign = 0, n_global_shared = 0;
  int32_t *shared_of = nullptr, *node = nullptr, *slot = nullptr, *foreign = nullptr;
  double *iface = nullptr;  // caller-owned, 3 * n_global_shared
  bool pending = false;     // between step_begin and step_finish
  // the energy balance: energy = NULL is off, and then none of the rest is looked at
  double *energy = nullptr;        // caller-owned, (energy_rows, 5) row-major
  int64_t energy_rows = 0, energy_index = 0;
  int32_t energy_every = 1;
  double *energy_part = nullptr;   // [node-pass blocks, then finish blocks][5] partial sums of one step
  double *energy_run = nullptr;    // the running W, D
  uint8_t *owned = nullptr;        // n_shared flags: this rank counts the mass and load terms of its k-th shared node
  // the material (saa_opfs.hip): 0 linear - the passes above -, 1 St. Venant-Kirchhoff, 2 compressible neo-Hooke
  int material = 0;
  unsigned long long *inverted = nullptr;  // two device words: (element, step) inversion events, lowest step index (all ones: none)
};

inline dim3 opstep_grid(int64_t n) { return dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)); }

// saa_opstep.hip: the handle's order-2 geometry table op->geom / op->bits, built on first need (order 1: nothing).
hipError_t operator_geometry(ModalOp *op);
// saa_opfs.hip: the finite-strain element pass of the stepper's material (!= 0) for one column x into contrib; an inverted
// element is counted at st->step_index.
hipError_t opfs_element_pass(OpStepper *st, const double *x, double *contrib);
// saa_opfs.hip: that pass for a caller that is not a step (saa_operator_stepper_set_dt): an inverted element is counted in the
// handle's scratch counter (op->fs_count, cleared first), not in the stepper's.
hipError_t opfs_element_pass_scratch(OpStepper *st, const double *x, double *contrib);
// saa_opstep.hip: the element pass the stepper is set to (material, "stored_geometry") at its d0 into contrib, inversions
// counted as above; the ramp factor of the next step; the element's shares of the lumped mass, out[npe e + corner] (the
// element pass of operator_lumped_mass).
hipError_t opstep_element_pass_at_d0(OpStepper *st, double *contrib);
double opstep_ramp_scale(const OpStepper *st);
hipError_t operator_element_masses(ModalOp *op, double *out);
// saa_optan.hip: the tangent element pass of `material` (!= 0) at u for one column v into contrib; an inverted element writes
// zeros and is counted in cnt (the two words of saa_opfs.hip) at step 0.  The handle's geometry table must exist.
hipError_t optan_element_pass(ModalOp *op, int material, const double *u, const double *v, double *contrib,
                              unsigned long long *cnt);
// saa_optan_block.hip: that pass for the m columns v + j * ldv into contrib + j * stride; an inverted element writes zeros
// into every column and is counted once.
hipError_t optan_block_element_pass(ModalOp *op, int material, const double *u, int32_t m, const double *v, int64_t ldv,
                                    double *contrib, int64_t stride, unsigned long long *cnt);

}  // namespace saa
