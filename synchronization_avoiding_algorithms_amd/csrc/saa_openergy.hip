// gfx950 kernels of the energy balance of the operator stepper (saa_operator_stepper_set_energy, saa_opstep.h).
//
// The central-difference update of Dynamic_solver.py:13-20, m (d1 - 2 d0 + dn)/dt^2 + alpha m (d1 - dn)/(2 dt) + s = lambda f
// with s = K d0, multiplied by (d1 - dn)/2 and summed over the dofs, is with the symmetry of K
//     (T + U)_{n+1/2} - (T + U)_{n-1/2} = dW_n - dD_n,
//     T_{n+1/2} = 1/2 sum m ((d1 - d0)/dt)^2,  U_{n+1/2} = 1/2 sum d1 s,  dW_n = lambda sum f (d1 - dn)/2,
//     dD_n = alpha/(4 dt) sum m (d1 - dn)^2,
// exactly, in the discrete sense.  The node pass holds every one of these factors per lane - s in registers, where it never
// reaches memory - so the balance costs a block reduction and one small launch per step, not another sweep over the mesh.
//
//  * openergy_node_kernel<MODE> is the node pass of saa_opstep.hip with the same statements in the same order (the update
//    through opstep_update_dof, so the state is bit-equal to a run with the balance off): MODE 0 the whole-mesh pass
//    (opstep_node_update_kernel), 1 the synchronised pass of a partition and 2 the predicted one (opstep_shared_node_kernel
//    <false> / <true>).  Each lane adds its node's share to five sums, the block reduces them - __shfl_down over the 64
//    lanes of a wave, then the four waves through LDS in wave order - and writes one [block][5] partial.
//  * openergy_finish_kernel is opstep_shared_finish_kernel with the shared dofs' share; its partials follow the node pass's.
//  * openergy_final_kernel, one block: lane t sums partials t, t + 256, ... in ascending order, the block reduces as above,
//    and lane 0 adds dW, dD to the running W, D and writes the row (T, U_{n+1/2}, U_n, W, D) on a recording step.
//  No floating-point atomics: every figure is bitwise repeatable and independent of how a run is split into calls.
//
// Shares of a partition (the rows of all ranks add up to the row of the whole mesh).  A dof counts when it is free and its
// node has elements on this rank.  Terms with m or f - T, dW, dD - carry the global mass and load, which every holder of a
// shared node has in full: a shared node counts only on the rank whose flag owned[k] is set.  U_n = 1/2 sum d0 s is formed
// from the rank's partial s on every holder, and the partial s add up to s.  U_{n+1/2} of a shared node: in a synchronised
// step from the summed s of the interface buffer in the finish kernel, on the owner; in a predicted step from the partial s
// on every holder (each with the d1 of its own table) - which is why MODE 2 sums a shared node's contributions, where
// opstep_shared_node_kernel<true> returns before it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "saa_modal_op.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_p2.h"

namespace saa {

namespace {

constexpr int kCols = 5;  // T_{n+1/2}, U_{n+1/2}, U_n, dW (row: W), dD (row: D)
constexpr int kWaves = kThreads / 64;
static_assert(kThreads % 64 == 0, "the block reduction works on whole waves");

// One dof's share.  `mass_terms`: this rank counts T, dW and dD of the dof; `half`: U_{n+1/2} is formed here from s.
__device__ __forceinline__ void energy_add(double (&e)[kCols], bool mass_terms, bool half, double s, double fi, double m, double x0,
                                           double xn, double d1, double dt, double alpha, double scale) {
  const double v = (d1 - x0) / dt, w = d1 - xn;
  if (mass_terms) {
    e[0] += 0.5 * m * (v * v);
    e[3] += scale * fi * (0.5 * w);
    e[4] += alpha / (4.0 * dt) * m * (w * w);
  }
  if (half) e[1] += 0.5 * d1 * s;
}

// The sums of e[] over the block, valid in lanes 0 .. kCols - 1 of the return value: a wave by __shfl_down (lanes past the
// data hold 0), the waves through LDS in wave order.  Every lane of the block must call it.
__device__ __forceinline__ double block_sum(double (&e)[kCols]) {
  __shared__ double lds[kWaves][kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e[c] += __shfl_down(e[c], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) lds[wave][c] = e[c];
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < kCols) {
    t = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += lds[w][threadIdx.x];
  }
  return t;
}

}  // namespace

// The node pass with the energy sums: MODE 0 = opstep_node_update_kernel, 1 = opstep_shared_node_kernel<false>,
// 2 = opstep_shared_node_kernel<true> (whose arguments these are), plus owned[k] and partial[kCols blockIdx.x + ...].
template <int MODE>
__global__ void __launch_bounds__(kThreads) openergy_node_kernel(
    int32_t n_nodes, const int64_t *__restrict__ offsets, const int32_t *__restrict__ pairs, const double *__restrict__ free_mask,
    const double *__restrict__ contrib, const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ d0,
    double *__restrict__ dn, double dt, double alpha, double scale, double *__restrict__ traj, int64_t n_cols, int64_t col,
    const int32_t *__restrict__ shared_of, const int32_t *__restrict__ slot, double *__restrict__ iface,
    const double *__restrict__ table_row, double *__restrict__ hist_row, const uint8_t *__restrict__ owned,
    double *__restrict__ partial) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (v < n_nodes) {
    const int32_t k = MODE == 0 ? -1 : shared_of[v];
    const int64_t b = offsets[v], end = offsets[v + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = b; i < end; ++i) {
      const double *q = contrib + 3 * (int64_t)pairs[i];
      s[0] += q[0];
      s[1] += q[1];
      s[2] += q[2];
    }
    if (MODE == 1 && k >= 0) {
      double *o = iface + 3 * (int64_t)slot[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t i = 3 * v + c;
        o[c] = s[c];
        if (end > b && free_mask[i] != 0.0) e[2] += 0.5 * d0[i] * s[c];
      }
    } else {
      const bool shared = MODE == 2 && k >= 0;
      const bool mine = shared ? owned[k] != 0 : true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int64_t i = 3 * v + c;
        const bool live = end > b && free_mask[i] != 0.0;
        const double fi = f[i], m = mass[i], x0 = d0[i], xn = dn[i];
        double d1;
        if (shared) {
          d1 = table_row[3 * (int64_t)k + c];
          if (hist_row) hist_row[3 * (int64_t)k + c] = d1;
        } else {
          d1 = opstep_update_dof(live, s[c], fi, m, x0, xn, dt, alpha, scale);
        }
        dn[i] = d1;
        if (col >= 0) traj[i * n_cols + col] = d1;
        if (live) {
          energy_add(e, mine, true, s[c], fi, m, x0, xn, d1, dt, alpha, scale);
          e[2] += 0.5 * x0 * s[c];
        }
      }
    }
  }
  const double t = block_sum(e);
  if (threadIdx.x < kCols) partial[kCols * (int64_t)blockIdx.x + threadIdx.x] = t;
}

// opstep_shared_finish_kernel with the shared dofs' share of T, U_{n+1/2} (from the summed s), dW and dD on the owner.
__global__ void __launch_bounds__(kThreads) openergy_finish_kernel(
    int32_t n_shared, int32_t n_foreign, const int32_t *__restrict__ node, const int32_t *__restrict__ slot,
    const int32_t *__restrict__ foreign, const int64_t *__restrict__ offsets, const double *__restrict__ free_mask,
    const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ d0, double *__restrict__ dn, double dt,
    double alpha, double scale, double *__restrict__ traj, int64_t n_cols, int64_t col, double *__restrict__ iface,
    double *__restrict__ hist_row, const uint8_t *__restrict__ owned, double *__restrict__ partial) {
  const int64_t j = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t n_local = 3 * (int64_t)n_shared;
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (j < n_local) {
    const int64_t k = j / 3;
    const int c = (int)(j - 3 * k);
    const int64_t v = node[k], i = 3 * v + c;
    const double s = iface[3 * (int64_t)slot[k] + c];
    const bool live = offsets[v + 1] > offsets[v] && free_mask[i] != 0.0;
    const double fi = f[i], m = mass[i], x0 = d0[i], xn = dn[i];
    const double d1 = opstep_update_dof(live, s, fi, m, x0, xn, dt, alpha, scale);
    dn[i] = d1;
    if (col >= 0) traj[i * n_cols + col] = d1;
    if (hist_row) hist_row[j] = d1;
    if (live && owned[k] != 0) energy_add(e, true, true, s, fi, m, x0, xn, d1, dt, alpha, scale);
  } else if (j < n_local + 3 * (int64_t)n_foreign) {
    const int64_t r = j - n_local;
    iface[3 * (int64_t)foreign[r / 3] + (r % 3)] = 0.0;
  }
  const double t = block_sum(e);
  if (threadIdx.x < kCols) partial[kCols * (int64_t)blockIdx.x + threadIdx.x] = t;
}

// One block.  The step's sums from its n_part partials; run[0] += dW, run[1] += dD; row >= 0: energy[kCols row + ...] =
// T_{n+1/2}, U_{n+1/2}, U_n, W_{n+1}, D_{n+1}.
__global__ void __launch_bounds__(kThreads) openergy_final_kernel(int32_t n_part, const double *__restrict__ partial,
                                                                  double *__restrict__ run, double *__restrict__ energy, int64_t row) {
  __shared__ double total[kCols];
  double e[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int32_t b = threadIdx.x; b < n_part; b += kThreads) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) e[c] += partial[kCols * (int64_t)b + c];
  }
  const double t = block_sum(e);
  if (threadIdx.x < kCols) total[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double W = run[0] + total[3], D = run[1] + total[4];
    run[0] = W;
    run[1] = D;
    if (row >= 0) {
      double *o = energy + kCols * row;
      o[0] = total[0];
      o[1] = total[1];
      o[2] = total[2];
      o[3] = W;
      o[4] = D;
    }
  }
}

#define OPENERGY_TRY(expr)           \
  do {                               \
    const hipError_t e_ = (expr);    \
    if (e_ != hipSuccess) return e_; \
  } while (0)

namespace {

int32_t node_blocks(const OpStepper *st) { return static_cast<int32_t>(opstep_grid(st->op->n_nodes).x); }
int64_t finish_lanes(const OpStepper *st) { return 3 * (static_cast<int64_t>(st->n_shared) + st->n_foreign); }

// the row of this step, by the recorder's rule (-1: none)
int64_t energy_row(const OpStepper *st) {
  if (st->energy_index % st->energy_every == 0 && st->energy_index / st->energy_every < st->energy_rows)
    return st->energy_index / st->energy_every;
  return -1;
}

hipError_t finalise(OpStepper *st, int32_t n_part) {
  hipLaunchKernelGGL(openergy_final_kernel, dim3(1), dim3(kThreads), 0, st->op->stream, n_part, st->energy_part, st->energy_run,
                     st->energy, energy_row(st));
  return hipGetLastError();
}

template <int MODE>
hipError_t node_pass(OpStepper *st, const double *contrib, const double *table_row, double *hist_row) {
  ModalOp *op = st->op;
  if (op->n_nodes == 0) return hipSuccess;
  hipLaunchKernelGGL(openergy_node_kernel<MODE>, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                     op->pairs, op->free_mask, contrib, st->mass, st->f, st->buf[st->cur], st->buf[1 - st->cur], st->dt, st->alpha,
                     opstep_ramp_scale(st), st->traj, st->n_cols, opstep_recorder_column(st), st->shared_of, st->slot, st->iface,
                     table_row, hist_row, st->owned, st->energy_part);
  return hipGetLastError();
}

}  // namespace

bool opstep_energy_on(const OpStepper *st) { return st->energy != nullptr; }
int opstep_passes(const OpStepper *st) { return st->passes; }

void openergy_clear(OpStepper *st) {
  void *bufs[] = {st->energy_part, st->energy_run, st->owned};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  st->energy = st->energy_part = st->energy_run = nullptr;
  st->owned = nullptr;
  st->energy_rows = st->energy_index = 0;
  st->energy_every = 1;
}

hipError_t opstep_set_energy(OpStepper *st, double *energy, int64_t n_rows, int32_t every, int64_t next_step_index,
                             const uint8_t *shared_owned) {
  ModalOp *op = st->op;
  OPENERGY_TRY(hipStreamSynchronize(op->stream));  // the old buffers may still be read by work in flight
  openergy_clear(st);
  if (!energy) return hipSuccess;
  const size_t n_part = static_cast<size_t>(node_blocks(st)) + opstep_grid(finish_lanes(st)).x;
  const size_t n_owned = st->n_shared > 0 ? static_cast<size_t>(st->n_shared) : 1;
  std::vector<uint8_t> flags(n_owned, 1);
  if (shared_owned)
    for (int32_t k = 0; k < st->n_shared; ++k) flags[k] = shared_owned[k] ? 1 : 0;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&st->energy_part), (n_part ? n_part : 1) * kCols * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&st->energy_run), 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&st->owned), n_owned);
  if (e == hipSuccess) e = hipMemsetAsync(st->energy_run, 0, 2 * sizeof(double), op->stream);
  if (e == hipSuccess) e = hipMemcpy(st->owned, flags.data(), n_owned, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    openergy_clear(st);
    return e;
  }
  st->energy = energy;
  st->energy_rows = n_rows;
  st->energy_every = every;
  st->energy_index = next_step_index;
  return hipSuccess;
}

hipError_t openergy_step(OpStepper *st, int32_t nsteps) {
  double *contrib = nullptr;
  OPENERGY_TRY(operator_scratch(st->op, 1, &contrib));
  for (int32_t k = 0; k < nsteps; ++k) {
    OPENERGY_TRY(opstep_element_pass(st, st->buf[st->cur], contrib));
    OPENERGY_TRY(node_pass<0>(st, contrib, nullptr, nullptr));
    OPENERGY_TRY(finalise(st, node_blocks(st)));
    opstep_advance(st);
  }
  return hipSuccess;
}

hipError_t openergy_step_begin(OpStepper *st) {
  double *contrib = nullptr;
  OPENERGY_TRY(operator_scratch(st->op, 1, &contrib));
  OPENERGY_TRY(opstep_ensure_shared_map(st));
  OPENERGY_TRY(opstep_element_pass(st, st->buf[st->cur], contrib));
  OPENERGY_TRY(node_pass<1>(st, contrib, nullptr, nullptr));
  st->pending = true;
  return hipSuccess;
}

hipError_t openergy_step_finish(OpStepper *st, double *hist, int64_t hist_row) {
  ModalOp *op = st->op;
  const int64_t lanes = finish_lanes(st);
  if (lanes > 0) {
    double *row = hist ? hist + hist_row * 3 * static_cast<int64_t>(st->n_shared) : nullptr;
    hipLaunchKernelGGL(openergy_finish_kernel, opstep_grid(lanes), dim3(kThreads), 0, op->stream, st->n_shared, st->n_foreign,
                       st->node, st->slot, st->foreign, op->offsets, op->free_mask, st->mass, st->f, st->buf[st->cur],
                       st->buf[1 - st->cur], st->dt, st->alpha, opstep_ramp_scale(st), st->traj, st->n_cols,
                       opstep_recorder_column(st), st->iface, row, st->owned, st->energy_part + kCols * static_cast<int64_t>(node_blocks(st)));
    OPENERGY_TRY(hipGetLastError());
  }
  OPENERGY_TRY(finalise(st, node_blocks(st) + static_cast<int32_t>(opstep_grid(lanes).x)));
  st->pending = false;
  opstep_advance(st);
  return hipSuccess;
}

hipError_t openergy_step_predicted(OpStepper *st, int32_t nsteps, const double *table, int64_t table_row0, double *hist,
                                   int64_t hist_row0) {
  double *contrib = nullptr;
  OPENERGY_TRY(operator_scratch(st->op, 1, &contrib));
  OPENERGY_TRY(opstep_ensure_shared_map(st));
  const int64_t width = 3 * static_cast<int64_t>(st->n_shared);
  for (int32_t k = 0; k < nsteps; ++k) {
    OPENERGY_TRY(opstep_element_pass(st, st->buf[st->cur], contrib));
    OPENERGY_TRY(node_pass<2>(st, contrib, width > 0 ? table + (table_row0 + k) * width : nullptr,
                              hist ? hist + (hist_row0 + k) * width : nullptr));
    OPENERGY_TRY(finalise(st, node_blocks(st)));
    opstep_advance(st);
  }
  return hipSuccess;
}

}  // namespace saa
