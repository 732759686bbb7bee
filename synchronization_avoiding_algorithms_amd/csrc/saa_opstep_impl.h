// What the two translation units of the operator stepper share (saa_opstep.hip: the time loop; saa_openergy.hip: the same
// loop with the energy balance recorded): the stepper's state, the update of one dof, and the host helpers of saa_opstep.hip
// that the energy loop reuses unchanged.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "saa_modal_op.h"
#include "saa_opstep.h"
#include "saa_p2_elem.h"

namespace saa {

// The update of one dof, Dynamic_solver.py:13-20: the text of opstep_node_update_kernel's loop body, shared by every kernel
// of a partition and by the energy kernels, so that a shared node is rounded by the finish kernel exactly as the node pass
// would have rounded it and a run with the energy balance on is bit-equal to one with it off.
__device__ __forceinline__ double opstep_update_dof(bool live, double s, double fi, double m, double x0, double xn, double dt,
                                                    double alpha, double scale) {
  const double num = dt * dt * (scale * fi - s) + 2.0 * m * x0 - m * xn + 0.5 * dt * m * alpha * xn;
  const double den = m + alpha * m * 0.5 * dt;
  return live ? num / den : 0.0;
}

struct OpStepper {
  ModalOp *op = nullptr;  // borrowed: must outlive the stepper
  double *mass = nullptr, *f = nullptr;
  double *buf[2] = {nullptr, nullptr};  // buf[cur] = d0, buf[1 - cur] = dn
  int cur = 0;
  double *geom = nullptr;               // order 2, stored geometry: [40][n_elems]; the handle's table (op->geom), borrowed
  uint32_t *bits = nullptr;             // n_elems; op->bits, borrowed
  bool stored = false;
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
  // the energy balance (saa_openergy.hip): energy = NULL is off, and then none of the rest is looked at
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
inline double opstep_ramp_scale(const OpStepper *st) { return st->ramp ? (st->tn < 1.0 ? st->tn : 1.0) : 1.0; }  // min(tn, 1)

// saa_opstep.hip: the K element pass of one column x into contrib by the variant the stepper is set to; the recorder column
// of this step (-1: none); shared_of of a stepper without a shared set (all -1), built on first need; swap, tn += dt, the
// step indices + 1.
hipError_t opstep_element_pass(OpStepper *st, const double *x, double *contrib);
int64_t opstep_recorder_column(const OpStepper *st);
hipError_t opstep_ensure_shared_map(OpStepper *st);
void opstep_advance(OpStepper *st);

// saa_opstep.hip: the handle's order-2 geometry table op->geom / op->bits, built on first need (order 1: nothing).
hipError_t operator_geometry(ModalOp *op);
// saa_opfs.hip: the finite-strain element pass of the stepper's material (!= 0) for one column x into contrib; an inverted
// element is counted at st->step_index.
hipError_t opfs_element_pass(OpStepper *st, const double *x, double *contrib);

// saa_openergy.hip: the four loops of saa_opstep.h with the energy kernels, entered from them when st->energy is set.
hipError_t openergy_step(OpStepper *st, int32_t nsteps);
hipError_t openergy_step_begin(OpStepper *st);
hipError_t openergy_step_finish(OpStepper *st, double *hist, int64_t hist_row);
hipError_t openergy_step_predicted(OpStepper *st, int32_t nsteps, const double *table, int64_t table_row0, double *hist,
                                   int64_t hist_row0);
// frees the energy buffers and switches the balance off; the caller has made sure that nothing in flight reads them
void openergy_clear(OpStepper *st);

}  // namespace saa
