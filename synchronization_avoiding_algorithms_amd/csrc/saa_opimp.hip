// gfx950 kernels of the implicit time loop on the saa_operator handle, either element order, three materials (saa_opimp.h).
//
//  * The scheme is Newmark with beta = 1/4, gamma = 1/2 (the trapezoidal rule) on the semi-discrete system of the explicit
//    operator stepper, m a + alpha m v + f_int(d) = scale(t) f with the caller's diagonal mass:
//      v1 = 2/dt (x - d) - v,  a1 = 4/dt^2 (x - d - dt v) - a,  r(x) = scale(t + dt) f - f_int(x) - m (a1 + alpha v1),
//      J(x) = K_T(x) + s,  s = (4/dt^2 + 2 alpha/dt) m.
//    Predictor x = d + dt v, full Newton steps x += dx, J dx = r by Jacobi-PCG from 0 with 1 / (diag K + s), diag K that of the
//    linear operator.  NOT provided: a line search, an automatic cut of dt, HHT-alpha, a consistent mass, partitions, an energy
//    table.  A step that is not accepted leaves d, v, a untouched: the iterate lives in its own vector x.
//  * The element passes are the existing ones, called as they are - the linear K passes, the force pass of saa_opfs.hip (through
//    an OpStepper shell that carries the material and this stepper's counter words), the tangent pass of saa_optan.hip.  They
//    write the contributions scratch; the node passes here read it through the handle's CSR in ascending element order.
//  * Launches.  A vector kernel runs at most kImpMaxBlocks workgroups of kThreads lanes with a grid-stride loop, so a reduction
//    has at most kImpMaxBlocks partials, and the kernel that needs the sum folds the partials itself: lane t adds partials t,
//    t + kThreads, ... in ascending order, the block reduces by __shfl_down and through LDS in wave order - every block gets the
//    same bits.  One PCG iteration is 4 launches: the tangent element pass of p; the shifted node pass (Ap, partials of p . Ap);
//    the update (folds p . Ap; alpha_cg and the curvature guard on the device; x_cg += alpha p, r -= alpha Ap, partials of r . z
//    and |r|^2 with z = minv r in registers); the direction pass (folds those; p = minv r + beta p; block 0 writes the iteration's
//    scalars).  The scalars of an iteration are double-buffered by parity, so no block reads a word another block of the same
//    launch writes.  Once the iteration is over (converged, or p . J p <= 0) the three kernels here return at once: the iterate
//    does not depend on when the host looks.  A Newton iteration adds the force element pass, the residual pass (r, the first
//    p, x_cg = 0, partials of |r|^2, the three scale terms and r . z - f_int is never written as a vector), a one-block final
//    kernel and the x += dx pass; a step adds the predictor and the finish pass.
//  * The host reads one status block (kStLen doubles) once per Newton iteration and every check_every PCG iterations (and once
//    at the end of the linear material's solve, whose result it takes when the recurrence residual is within tol of the scale
//    at the solved x, which the next residual pass gives: a residual evaluated afresh has the round-off floor of f_int, which
//    a tight tol lies below).
//  * No floating-point atomics: every result is bitwise repeatable and independent of how a run is split into calls.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <new>

#include "saa_hip_host.h"
#include "saa_modal_op.h"
#include "saa_opimp.h"
#include "saa_opstep.h"
#include "saa_opstep_impl.h"
#include "saa_p2.h"

namespace saa {

constexpr int kImpMaxBlocks = 2048;

// the status block, doubles.  Newton: |r|, |scale f|, |f_int|, |m (a1 + alpha v1)|, inverted elements, r . z, the PCG iterations
// of the solves finished since the step call began.  S0 / S1: the PCG scalars by parity - r . z, live (1: iterating), iterations
// made, guard (1: stopped at p . J p <= 0), |r_cg|.  A: what the update kernel tells the direction kernel of the same
// iteration - live, guard.
enum { kStR = 0, kStExt = 1, kStInt = 2, kStIne = 3, kStInv = 4, kStRz = 5, kStCg = 6, kStS0 = 8, kStS1 = 16, kStA = 24, kStLen = 28 };
enum { kSRz = 0, kSLive = 1, kSIter = 2, kSGuard = 3, kSNorm = 4 };

struct OpImplicit {
  ModalOp *op = nullptr;  // borrowed: must outlive the stepper
  OpStepper fs;           // the shell the force pass of saa_opfs.hip reads: op, material, counter words, step index
  int material = 0;
  double *mass = nullptr, *f = nullptr, *diag_k = nullptr, *shift = nullptr, *minv = nullptr;
  double *d = nullptr, *v = nullptr, *a = nullptr;             // the accepted state
  double *x = nullptr;                                         // the Newton iterate
  double *r = nullptr, *p = nullptr, *ap = nullptr, *xcg = nullptr;
  double *part = nullptr;    // [8][kImpMaxBlocks]: p . Ap at 0, (r . z, |r|^2) at 1, the five of the residual pass at 3
  double *status = nullptr;  // kStLen
  unsigned long long *cnt = nullptr;  // the two counter words of the force pass
  double dt = 0.0, alpha = 0.0, t = 0.0;
  int ramp = 1;
  double tol = 1e-10;
  int32_t max_newton = 25, check_every = 25;
  int64_t max_cg = 0;
  double *traj = nullptr;
  int64_t n_cols = 0, step_index = 0;
  int32_t save_every = 1;
};

namespace {

inline int32_t imp_blocks(int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return static_cast<int32_t>(b < 1 ? 1 : (b > kImpMaxBlocks ? kImpMaxBlocks : b));
}

// The sums of e[] over the block, in every lane: a wave by __shfl_down, the waves through LDS in wave order.  Every lane of
// the block must call it.
template <int N>
__device__ __forceinline__ void imp_block_sum(double (&e)[N]) {
  __shared__ double lds[kWaves][N];
#pragma unroll
  for (int c = 0; c < N; ++c)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e[c] += __shfl_down(e[c], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (a second call: the first one's reads are over)
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) lds[wave][c] = e[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double t = lds[0][c];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += lds[w][c];
    e[c] = t;
  }
}

// The fixed-order final sum of n_part partials part[N b + c], in every lane of the block.
template <int N>
__device__ __forceinline__ void imp_fold(const double *__restrict__ part, int32_t n_part, double (&e)[N]) {
#pragma unroll
  for (int c = 0; c < N; ++c) e[c] = 0.0;
  for (int32_t b = threadIdx.x; b < n_part; b += kThreads) {
#pragma unroll
    for (int c = 0; c < N; ++c) e[c] += part[N * (int64_t)b + c];
  }
  imp_block_sum<N>(e);
}

// v1, a1 of the trial x, the formulas of the residual pass and of the finish pass alike
__device__ __forceinline__ void newmark_rates(double x, double d, double v, double a, double dt, double c2, double c4, double &v1,
                                              double &a1) {
  const double inc = x - d;
  v1 = c2 * inc - v;
  a1 = c4 * (inc - dt * v) - a;
}

}  // namespace

// *count += nodes with an element whose mass is not > 0 on some dof (NaN counts)
__global__ void __launch_bounds__(kThreads) opimp_mass_check_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                    const double *__restrict__ mass, int32_t *__restrict__ count) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes || offsets[v + 1] == offsets[v]) return;
  if (!(mass[3 * v] > 0.0 && mass[3 * v + 1] > 0.0 && mass[3 * v + 2] > 0.0)) atomicAdd(count, 1);
}

// shift = c m and minv = 1 / (diag K + shift) on the live dofs (free, at a node with elements), 0 elsewhere: minv != 0 is
// the live mask of every dof-wise kernel below.  One lane per node.
__global__ void __launch_bounds__(kThreads) opimp_setup_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                               const double *__restrict__ free_mask, const double *__restrict__ mass,
                                                               const double *__restrict__ diag_k, double c, double *__restrict__ shift,
                                                               double *__restrict__ minv) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes) return;
  const bool has = offsets[v + 1] > offsets[v];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t i = 3 * v + k;
    const bool live = has && free_mask[i] != 0.0;
    const double s = c * mass[i], j = diag_k[i] + s;
    shift[i] = live ? s : 0.0;
    minv[i] = live ? (j > 0.0 ? 1.0 / j : 1.0) : 0.0;
  }
}

// Shifted node pass: out[3v + c] = (sum of node v's contributions, ascending element order) + shift v (SHIFT), 0 on Dirichlet
// dofs; DOT: partial[blockIdx.x] = the block's share of v . out.  gate (or NULL): the live word of the PCG scalars, 0 = return.
template <bool SHIFT, bool DOT>
__global__ void __launch_bounds__(kThreads) opimp_shifted_node_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                                      const int32_t *__restrict__ pairs,
                                                                      const double *__restrict__ free_mask,
                                                                      const double *__restrict__ contrib,
                                                                      const double *__restrict__ shift, const double *__restrict__ vec,
                                                                      double *__restrict__ out, double *__restrict__ partial,
                                                                      const double *__restrict__ gate) {
  if (gate && *gate == 0.0) return;
  double e[1] = {0.0};
  for (int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kThreads) {
    const int64_t b = offsets[v], end = offsets[v + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = b; i < end; ++i) {
      const double *q = contrib + 3 * (int64_t)pairs[i];
      s[0] += q[0];
      s[1] += q[1];
      s[2] += q[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = 3 * v + c;
      const bool fr = free_mask[i] != 0.0;
      double o = s[c];
      if (SHIFT || DOT) {
        const double vi = vec[i];
        if (SHIFT) o += shift[i] * vi;
        if (DOT && fr) e[0] += vi * o;
      }
      out[i] = fr ? o : 0.0;
    }
  }
  if (DOT) {
    imp_block_sum<1>(e);
    if (threadIdx.x == 0) partial[blockIdx.x] = e[0];
  }
}

// One block: *dot = the fixed-order sum of the n_part partials.
__global__ void __launch_bounds__(kThreads) opimp_dot_final_kernel(int32_t n_part, const double *__restrict__ partial,
                                                                   double *__restrict__ dot) {
  double e[1];
  imp_fold<1>(partial, n_part, e);
  if (threadIdx.x == 0) *dot = e[0];
}

// The caller's velocity, masked, and the initial acceleration, one lane per node: v <- v_in on live dofs (NULL: 0), a = (scale f
// - f_int(d) - alpha m v) / m with f_int the node's contributions.
__global__ void __launch_bounds__(kThreads) opimp_accel_kernel(int32_t n_nodes, const int64_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ pairs, const double *__restrict__ contrib,
                                                               const double *__restrict__ minv, const double *__restrict__ mass,
                                                               const double *__restrict__ f, const double *__restrict__ v_in,
                                                               double alpha, double scale, double *__restrict__ v,
                                                               double *__restrict__ a) {
  for (int64_t n = blockIdx.x * (int64_t)kThreads + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * kThreads) {
    const int64_t b = offsets[n], end = offsets[n + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = b; i < end; ++i) {
      const double *q = contrib + 3 * (int64_t)pairs[i];
      s[0] += q[0];
      s[1] += q[1];
      s[2] += q[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = 3 * n + c;
      const bool live = minv[i] != 0.0;
      const double m = mass[i], vi = live && v_in ? v_in[i] : 0.0;
      v[i] = vi;
      a[i] = live ? (scale * f[i] - s[c] - alpha * m * vi) / m : 0.0;
    }
  }
}

// d <- d_in on live dofs, 0 elsewhere (before the force pass of set_state, which reads d)
__global__ void __launch_bounds__(kThreads) opimp_mask_kernel(int64_t n, const double *__restrict__ minv,
                                                              const double *__restrict__ d_in, double *__restrict__ d) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    d[i] = minv[i] != 0.0 && d_in ? d_in[i] : 0.0;
}

// Predictor: x = d + dt v on live dofs, 0 elsewhere.
__global__ void __launch_bounds__(kThreads) opimp_predict_kernel(int64_t n, const double *__restrict__ minv,
                                                                 const double *__restrict__ d, const double *__restrict__ v, double dt,
                                                                 double *__restrict__ x) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    x[i] = minv[i] != 0.0 ? d[i] + dt * v[i] : 0.0;
}

// Residual node pass: r = scale f - f_int(x) - m (a1 + alpha v1) on live dofs (0 elsewhere) from the contributions of the
// force pass, and the start of the PCG: p = minv r, x_cg = 0.  partial[5 blockIdx.x + ...] = the block's shares of |r|^2,
// |scale f|^2, |f_int|^2, |m (a1 + alpha v1)|^2 and r . minv r over the live dofs.
__global__ void __launch_bounds__(kThreads) opimp_residual_kernel(
    int32_t n_nodes, const int64_t *__restrict__ offsets, const int32_t *__restrict__ pairs, const double *__restrict__ contrib,
    const double *__restrict__ minv, const double *__restrict__ mass, const double *__restrict__ f, const double *__restrict__ x,
    const double *__restrict__ d, const double *__restrict__ v, const double *__restrict__ a, double dt, double c2, double c4,
    double alpha, double scale, double *__restrict__ r, double *__restrict__ p, double *__restrict__ xcg,
    double *__restrict__ partial) {
  double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t n = blockIdx.x * (int64_t)kThreads + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * kThreads) {
    const int64_t b = offsets[n], end = offsets[n + 1];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = b; i < end; ++i) {
      const double *q = contrib + 3 * (int64_t)pairs[i];
      s[0] += q[0];
      s[1] += q[1];
      s[2] += q[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t i = 3 * n + c;
      const double mi = minv[i];
      double ri = 0.0;
      if (mi != 0.0) {
        double v1, a1;
        newmark_rates(x[i], d[i], v[i], a[i], dt, c2, c4, v1, a1);
        const double ext = scale * f[i], ine = mass[i] * (a1 + alpha * v1);
        ri = ext - s[c] - ine;
        e[0] += ri * ri;
        e[1] += ext * ext;
        e[2] += s[c] * s[c];
        e[3] += ine * ine;
        e[4] += ri * (mi * ri);
      }
      r[i] = ri;
      p[i] = mi * ri;
      xcg[i] = 0.0;
    }
  }
  imp_block_sum<5>(e);
  if (threadIdx.x < 5) partial[5 * (int64_t)blockIdx.x + threadIdx.x] = e[threadIdx.x];
}

// One block, once per Newton iteration: the four norms, the inversion count of the force pass and r . z into the status
// block, and the PCG scalars of parity 0 for a start from 0.
__global__ void __launch_bounds__(kThreads) opimp_newton_final_kernel(int32_t n_part, const double *__restrict__ partial,
                                                                      const unsigned long long *__restrict__ cnt,
                                                                      double *__restrict__ status) {
  double e[5];
  imp_fold<5>(partial, n_part, e);
  if (threadIdx.x == 0) {
    const double rn = sqrt(e[0]);
    status[kStR] = rn;
    status[kStExt] = sqrt(e[1]);
    status[kStInt] = sqrt(e[2]);
    status[kStIne] = sqrt(e[3]);
    status[kStInv] = static_cast<double>(cnt[0]);
    status[kStRz] = e[4];
    double *s0 = status + kStS0;
    s0[kSRz] = e[4];
    s0[kSLive] = 1.0;
    s0[kSIter] = 0.0;
    s0[kSGuard] = 0.0;
    s0[kSNorm] = rn;
  }
}

// PCG update.  alpha_cg = r . z / p . Ap from the scalars s_in and the folded partials of p . Ap; p . Ap <= 0 (NaN included)
// stops the iteration here, on the device, and nothing is updated.  x_cg += alpha p, r -= alpha Ap; partial[2 blockIdx.x +
// ...] = the block's shares of r . minv r and |r|^2.  Block 0 leaves (live, guard) in a_out for the direction pass.
__global__ void __launch_bounds__(kThreads) opimp_cg_update_kernel(int64_t n, int32_t n_pap, const double *__restrict__ pap_part,
                                                                   const double *__restrict__ s_in, double *__restrict__ a_out,
                                                                   const double *__restrict__ minv, const double *__restrict__ p,
                                                                   const double *__restrict__ ap, double *__restrict__ xcg,
                                                                   double *__restrict__ r, double *__restrict__ partial) {
  if (s_in[kSLive] == 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      a_out[0] = 0.0;
      a_out[1] = s_in[kSGuard];
    }
    return;
  }
  double pap[1];
  imp_fold<1>(pap_part, n_pap, pap);
  const bool ok = pap[0] > 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a_out[0] = ok ? 1.0 : 0.0;
    a_out[1] = ok ? 0.0 : 1.0;
  }
  if (!ok) return;
  const double alpha = s_in[kSRz] / pap[0];
  double e[2] = {0.0, 0.0};
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    xcg[i] += alpha * p[i];
    const double rn = r[i] - alpha * ap[i];
    r[i] = rn;
    e[0] += rn * (minv[i] * rn);
    e[1] += rn * rn;
  }
  imp_block_sum<2>(e);
  if (threadIdx.x < 2) partial[2 * (int64_t)blockIdx.x + threadIdx.x] = e[threadIdx.x];
}

// PCG direction.  beta = (r . z)_new / (r . z)_old from the folded partials; p = minv r + beta p.  Block 0 writes the scalars
// of the next iteration into s_out (the other parity): live ends when |r| <= target.  An iteration that the update pass
// stopped, or that was over before, only carries the scalars forward with live = 0.
__global__ void __launch_bounds__(kThreads) opimp_cg_direction_kernel(int64_t n, int32_t n_part, const double *__restrict__ partial,
                                                                      const double *__restrict__ s_in, const double *__restrict__ a_in,
                                                                      double *__restrict__ s_out, double target,
                                                                      const double *__restrict__ minv, const double *__restrict__ r,
                                                                      double *__restrict__ p) {
  if (a_in[0] == 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      s_out[kSRz] = s_in[kSRz];
      s_out[kSLive] = 0.0;
      s_out[kSIter] = s_in[kSIter];
      s_out[kSGuard] = a_in[1];
      s_out[kSNorm] = s_in[kSNorm];
    }
    return;
  }
  double e[2];
  imp_fold<2>(partial, n_part, e);
  const double rz_old = s_in[kSRz];
  const double beta = rz_old > 0.0 ? e[0] / rz_old : 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    p[i] = minv[i] * r[i] + beta * p[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double rn = sqrt(e[1]);
    s_out[kSRz] = e[0];
    s_out[kSLive] = rn <= target ? 0.0 : 1.0;
    s_out[kSIter] = s_in[kSIter] + 1.0;
    s_out[kSGuard] = 0.0;
    s_out[kSNorm] = rn;
  }
}

// Newton update: x += x_cg, or += p - still the preconditioned residual - when the PCG made no iteration.  Block 0 adds the
// solve's iterations to the running count (its only writer).
__global__ void __launch_bounds__(kThreads) opimp_newton_update_kernel(int64_t n, const double *__restrict__ s_in,
                                                                       const double *__restrict__ xcg, const double *__restrict__ p,
                                                                       double *__restrict__ x, double *__restrict__ cg_total) {
  const double *dx = s_in[kSIter] > 0.0 ? xcg : p;
  if (blockIdx.x == 0 && threadIdx.x == 0) *cg_total += s_in[kSIter];
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) x[i] += dx[i];
}

// Finish pass: d, v, a <- x, v1(x), a1(x) (0 off the live dofs); d goes to column col of the row-major (n, n_cols) recorder when
// col >= 0.
__global__ void __launch_bounds__(kThreads) opimp_finish_kernel(int64_t n, const double *__restrict__ minv,
                                                                const double *__restrict__ x, double *__restrict__ d,
                                                                double *__restrict__ v, double *__restrict__ a, double dt, double c2,
                                                                double c4, double *__restrict__ traj, int64_t n_cols, int64_t col) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    double d1 = 0.0, v1 = 0.0, a1 = 0.0;
    if (minv[i] != 0.0) {
      d1 = x[i];
      newmark_rates(d1, d[i], v[i], a[i], dt, c2, c4, v1, a1);
    }
    d[i] = d1;
    v[i] = v1;
    a[i] = a1;
    if (col >= 0) traj[i * n_cols + col] = d1;
  }
}

namespace {

int64_t n_dof(const ModalOp *op) { return 3 * static_cast<int64_t>(op->n_nodes); }

hipError_t reset_counters(unsigned long long *cnt, hipStream_t stream) {
  SAA_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), stream));
  return hipMemsetAsync(cnt + 1, 0xff, sizeof(unsigned long long), stream);
}

// the linear K pass of one column, either order
hipError_t linear_pass(ModalOp *op, const double *x, double *contrib) {
  return op->order == 2 ? p2_elem_pass_k(op, x, contrib) : modal_elem_pass_k(op, x, contrib);
}

hipError_t force_pass(OpImplicit *st, const double *x, double *contrib) {
  if (st->material == 0) return linear_pass(st->op, x, contrib);
  st->fs.step_index = st->step_index;
  return opfs_element_pass(&st->fs, x, contrib);
}

hipError_t tangent_pass(OpImplicit *st, const double *u, const double *v, double *contrib) {
  if (st->material == 0) return linear_pass(st->op, v, contrib);
  return optan_element_pass(st->op, st->material, u, v, contrib, st->cnt);
}

double shift_factor(const OpImplicit *st) { return 4.0 / (st->dt * st->dt) + 2.0 * st->alpha / st->dt; }
double ramp_scale(const OpImplicit *st, double t) { return st->ramp ? (t < 1.0 ? t : 1.0) : 1.0; }

hipError_t setup(OpImplicit *st) {
  ModalOp *op = st->op;
  if (op->n_nodes == 0) return hipSuccess;
  hipLaunchKernelGGL(opimp_setup_kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                     op->free_mask, st->mass, st->diag_k, shift_factor(st), st->shift, st->minv);
  return hipGetLastError();
}

int64_t recorder_column(const OpImplicit *st) {
  if (st->traj && st->step_index % st->save_every == 0 && st->step_index / st->save_every < st->n_cols)
    return st->step_index / st->save_every;
  return -1;
}

hipError_t read_status(OpImplicit *st, double *host) {
  SAA_HIP_TRY(hipMemcpyAsync(host, st->status, kStLen * sizeof(double), hipMemcpyDeviceToHost, st->op->stream));
  return hipStreamSynchronize(st->op->stream);
}

// J dx = r from 0 until |r_cg| <= target, at most max_cg iterations; the scalars end in parity *par.  want_end: look once
// more when the last iteration was not a look; end (valid after a last look): the solve's scalars, end[kSLive] = 0 with
// end[kSGuard] = 0 when it reached the target.
hipError_t pcg(OpImplicit *st, double *contrib, double target, int *par, bool want_end, double (&end)[5]) {
  ModalOp *op = st->op;
  const int64_t n = n_dof(op);
  const int32_t nbn = imp_blocks(op->n_nodes), nbd = imp_blocks(n);
  double *pap_part = st->part, *cg_part = st->part + kImpMaxBlocks;
  double host[kStLen] = {};
  host[kStS0 + kSLive] = 1.0;
  int cur = 0;
  bool looked = false;
  for (int64_t it = 1; it <= st->max_cg; ++it) {
    double *s_in = st->status + (cur ? kStS1 : kStS0), *s_out = st->status + (cur ? kStS0 : kStS1);
    SAA_HIP_TRY(tangent_pass(st, st->x, st->p, contrib));
    hipLaunchKernelGGL((opimp_shifted_node_kernel<true, true>), dim3(nbn), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                       op->pairs, op->free_mask, contrib, st->shift, st->p, st->ap, pap_part, s_in + kSLive);
    hipLaunchKernelGGL(opimp_cg_update_kernel, dim3(nbd), dim3(kThreads), 0, op->stream, n, nbn, pap_part, s_in, st->status + kStA,
                       st->minv, st->p, st->ap, st->xcg, st->r, cg_part);
    hipLaunchKernelGGL(opimp_cg_direction_kernel, dim3(nbd), dim3(kThreads), 0, op->stream, n, nbd, cg_part, s_in, st->status + kStA,
                       s_out, target, st->minv, st->r, st->p);
    SAA_HIP_TRY(hipGetLastError());
    cur = 1 - cur;
    if (it % st->check_every == 0) {
      SAA_HIP_TRY(read_status(st, host));
      looked = true;
      if (host[(cur ? kStS1 : kStS0) + kSLive] == 0.0) break;
    } else {
      looked = false;
    }
  }
  if (want_end && !looked) SAA_HIP_TRY(read_status(st, host));
  for (int k = 0; k < 5; ++k) end[k] = host[(cur ? kStS1 : kStS0) + k];
  *par = cur;
  return hipSuccess;
}

}  // namespace

hipError_t operator_shifted_apply(ModalOp *op, int material, const double *u, const double *v, const double *shift, double *out,
                                  double *dot, int64_t *n_inverted) {
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  if (material == 0) {
    SAA_HIP_TRY(linear_pass(op, v, contrib));
  } else {
    SAA_HIP_TRY(operator_geometry(op));
    if (!op->fs_count) SAA_HIP_TRY(dev_alloc(&op->fs_count, 2));
    SAA_HIP_TRY(reset_counters(op->fs_count, op->stream));
    SAA_HIP_TRY(optan_element_pass(op, material, u, v, contrib, op->fs_count));
  }
  const int32_t nb = imp_blocks(op->n_nodes);
  if (dot && !op->imp_part) SAA_HIP_TRY(dev_alloc(&op->imp_part, static_cast<size_t>(kImpMaxBlocks)));
  const auto kernel = shift ? (dot ? opimp_shifted_node_kernel<true, true> : opimp_shifted_node_kernel<true, false>)
                            : (dot ? opimp_shifted_node_kernel<false, true> : opimp_shifted_node_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs, op->free_mask, contrib,
                     shift, v, out, op->imp_part, static_cast<const double *>(nullptr));
  SAA_HIP_TRY(hipGetLastError());
  if (dot) {
    hipLaunchKernelGGL(opimp_dot_final_kernel, dim3(1), dim3(kThreads), 0, op->stream, nb, op->imp_part, dot);
    SAA_HIP_TRY(hipGetLastError());
  }
  if (n_inverted) {
    unsigned long long host = 0;
    if (material != 0) SAA_HIP_TRY(hipMemcpyAsync(&host, op->fs_count, sizeof(host), hipMemcpyDeviceToHost, op->stream));
    SAA_HIP_TRY(hipStreamSynchronize(op->stream));
    *n_inverted = static_cast<int64_t>(host);
  }
  return hipSuccess;
}

void opimp_destroy(OpImplicit *st) {
  if (!st) return;
  (void)hipSetDevice(st->op->device);
  void *bufs[] = {st->mass, st->f, st->diag_k, st->shift, st->minv, st->d, st->v, st->a, st->x,
                  st->r,    st->p, st->ap,     st->xcg,   st->part, st->status, st->cnt};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete st;
}

int opimp_device(const OpImplicit *st) { return st->op->device; }
double opimp_alpha(const OpImplicit *st) { return st->alpha; }

hipError_t opimp_create(ModalOp *op, const double *mass, const double *f_ext, double dt, double alpha, int ramp, int material,
                        OpImplicit **out, std::string &err) {
  *out = nullptr;
  OpImplicit *st = new (std::nothrow) OpImplicit;
  if (!st) return hipErrorOutOfMemory;
  st->op = op;
  st->dt = dt;
  st->alpha = alpha;
  st->ramp = ramp;
  st->material = material;
  const size_t n = static_cast<size_t>(n_dof(op)), bytes = n * sizeof(double);
  st->max_cg = 20 * static_cast<int64_t>(n);
  int32_t *count = nullptr;
  int32_t bad = 0;
  double **vecs[] = {&st->mass, &st->f, &st->diag_k, &st->shift, &st->minv, &st->d, &st->v, &st->a, &st->x, &st->r, &st->p, &st->ap, &st->xcg};
  hipError_t e = hipSuccess;
  for (double **b : vecs)
    if (e == hipSuccess) e = dev_alloc(b, n);
  if (e == hipSuccess) e = dev_alloc(&st->part, static_cast<size_t>(8) * kImpMaxBlocks);
  if (e == hipSuccess) e = dev_alloc(&st->status, static_cast<size_t>(kStLen));
  if (e == hipSuccess) e = dev_alloc(&st->cnt, 2);
  if (e == hipSuccess) e = dev_alloc(&count, 1);
  if (e == hipSuccess) e = hipMemcpyAsync(st->mass, mass, bytes, hipMemcpyDeviceToDevice, op->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(st->f, f_ext, bytes, hipMemcpyDeviceToDevice, op->stream);
  double *zero[] = {st->d, st->v, st->a, st->x, st->r, st->p, st->ap, st->xcg};
  for (double *b : zero)
    if (e == hipSuccess) e = hipMemsetAsync(b, 0, n ? bytes : sizeof(double), op->stream);
  if (e == hipSuccess) e = hipMemsetAsync(st->status, 0, kStLen * sizeof(double), op->stream);
  if (e == hipSuccess) e = reset_counters(st->cnt, op->stream);
  if (e == hipSuccess) e = hipMemsetAsync(count, 0, sizeof(int32_t), op->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(opimp_mass_check_kernel, opstep_grid(op->n_nodes), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                       st->mass, count);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, count, sizeof(int32_t), hipMemcpyDeviceToHost, op->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(op->stream);
  if (count) (void)hipFree(count);
  if (e == hipSuccess && bad > 0) {
    err = "saa_operator_implicit_create: the mass is not > 0 at " + std::to_string(bad) + " node(s) that have elements";
    e = hipErrorInvalidValue;
  }
  if (e == hipSuccess) e = operator_diagonal(op, st->diag_k, nullptr);
  if (e == hipSuccess) e = setup(st);
  if (e == hipSuccess && material != 0) e = operator_geometry(op);
  if (e != hipSuccess) {
    opimp_destroy(st);
    return e;
  }
  st->fs.op = op;
  st->fs.material = material;
  st->fs.inverted = st->cnt;
  e = opimp_set_state(st, nullptr, nullptr, 0.0);  // a of the balance at rest: f / m without the ramp
  if (e != hipSuccess) {
    opimp_destroy(st);
    return e;
  }
  *out = st;
  return hipSuccess;
}

hipError_t opimp_set_state(OpImplicit *st, const double *d, const double *v, double t) {
  ModalOp *op = st->op;
  const int64_t n = n_dof(op);
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  st->t = t;
  if (op->n_nodes == 0) return hipSuccess;
  hipLaunchKernelGGL(opimp_mask_kernel, dim3(imp_blocks(n)), dim3(kThreads), 0, op->stream, n, st->minv, d, st->d);
  SAA_HIP_TRY(hipGetLastError());
  SAA_HIP_TRY(reset_counters(st->cnt, op->stream));
  SAA_HIP_TRY(force_pass(st, st->d, contrib));
  hipLaunchKernelGGL(opimp_accel_kernel, dim3(imp_blocks(op->n_nodes)), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets,
                     op->pairs, contrib, st->minv, st->mass, st->f, v, st->alpha, ramp_scale(st, t), st->v, st->a);
  return hipGetLastError();
}

hipError_t opimp_get_state(OpImplicit *st, double *d, double *v, double *a, double *t) {
  const size_t bytes = static_cast<size_t>(n_dof(st->op)) * sizeof(double);
  hipStream_t s = st->op->stream;
  if (d) SAA_HIP_TRY(hipMemcpyAsync(d, st->d, bytes, hipMemcpyDeviceToDevice, s));
  if (v) SAA_HIP_TRY(hipMemcpyAsync(v, st->v, bytes, hipMemcpyDeviceToDevice, s));
  if (a) SAA_HIP_TRY(hipMemcpyAsync(a, st->a, bytes, hipMemcpyDeviceToDevice, s));
  SAA_HIP_TRY(hipStreamSynchronize(s));
  if (t) *t = st->t;
  return hipSuccess;
}

void opimp_set_recorder(OpImplicit *st, double *traj, int64_t n_cols, int32_t save_every, int64_t next_step_index) {
  st->traj = traj;
  st->n_cols = n_cols;
  st->save_every = save_every;
  st->step_index = next_step_index;
}

bool opimp_set_option(OpImplicit *st, const char *name, double value) {
  if (!std::isfinite(value)) return false;
  if (std::strcmp(name, "tol") == 0 && value > 0.0 && value < 1.0) {
    st->tol = value;
    return true;
  }
  const bool whole = value >= 1.0 && value <= 2147483647.0 && value == std::floor(value);
  if (std::strcmp(name, "max_newton") == 0 && whole) {
    st->max_newton = static_cast<int32_t>(value);
    return true;
  }
  if (std::strcmp(name, "max_cg") == 0 && whole) {
    st->max_cg = static_cast<int64_t>(value);
    return true;
  }
  if (std::strcmp(name, "check_every") == 0 && whole) {
    st->check_every = static_cast<int32_t>(value);
    return true;
  }
  return false;
}

hipError_t opimp_set_dt(OpImplicit *st, double dt) {
  st->dt = dt;
  return setup(st);
}

hipError_t opimp_step(OpImplicit *st, int32_t nsteps, OpImplicitInfo *info) {
  ModalOp *op = st->op;
  *info = OpImplicitInfo();
  if (nsteps <= 0 || op->n_nodes == 0) return hipSuccess;
  const int64_t n = n_dof(op);
  const int32_t nbn = imp_blocks(op->n_nodes), nbd = imp_blocks(n);
  double *contrib = nullptr;
  SAA_HIP_TRY(operator_scratch(op, 1, &contrib));
  double *res_part = st->part + 3 * kImpMaxBlocks;
  const double dt = st->dt, c2 = 2.0 / dt, c4 = 4.0 / (dt * dt);
  double host[kStLen];
  SAA_HIP_TRY(hipMemsetAsync(st->status + kStCg, 0, sizeof(double), op->stream));
  for (int32_t k = 0; k < nsteps; ++k) {
    const double scale = ramp_scale(st, st->t + dt);
    SAA_HIP_TRY(reset_counters(st->cnt, op->stream));
    hipLaunchKernelGGL(opimp_predict_kernel, dim3(nbd), dim3(kThreads), 0, op->stream, n, st->minv, st->d, st->v, dt, st->x);
    SAA_HIP_TRY(hipGetLastError());
    double previous = -1.0;
    double solved = -1.0;  // linear material: |r_cg| of a solve that reached its target, until the scale at the solved x is known
    int reason = 0;
    for (int32_t newton = 0;; ++newton) {
      SAA_HIP_TRY(force_pass(st, st->x, contrib));
      hipLaunchKernelGGL(opimp_residual_kernel, dim3(nbn), dim3(kThreads), 0, op->stream, op->n_nodes, op->offsets, op->pairs, contrib,
                         st->minv, st->mass, st->f, st->x, st->d, st->v, st->a, dt, c2, c4, st->alpha, scale, st->r, st->p, st->xcg,
                         res_part);
      hipLaunchKernelGGL(opimp_newton_final_kernel, dim3(1), dim3(kThreads), 0, op->stream, nbn, res_part, st->cnt, st->status);
      SAA_HIP_TRY(hipGetLastError());
      SAA_HIP_TRY(read_status(st, host));
      const double rnorm = host[kStR];
      info->cg_iterations = static_cast<int64_t>(host[kStCg]);
      const double ref = std::fmax(host[kStExt], std::fmax(host[kStInt], host[kStIne]));
      const double goal = st->tol * ref;
      if (host[kStInv] > 0.0) {
        reason = 3;
        break;
      }
      if (!std::isfinite(rnorm)) {
        reason = 2;
        break;
      }
      info->residual = ref > 0.0 ? rnorm / ref : rnorm;
      if (rnorm <= goal) break;
      // the linear system, solved to the tolerance, is the step: a residual evaluated afresh has a round-off floor of its
      // own, which tol may lie below.  The recurrence residual is held to the scale at the solved x, as every other |r| is.
      if (solved >= 0.0 && solved <= goal) {
        info->residual = ref > 0.0 ? solved / ref : solved;
        break;
      }
      if (newton >= st->max_newton) {
        reason = 1;
        break;
      }
      // the forcing term of newton_solve_operator; the linear material solves its one system to the tolerance
      double eta = previous < 0.0 ? 0.1 : std::fmin(0.1, 0.9 * (rnorm / previous) * (rnorm / previous));
      eta = std::fmax(eta, 0.1 * goal / rnorm);
      const double target = st->material == 0 ? goal : eta * rnorm;
      int par = 0;
      double end[5];
      SAA_HIP_TRY(pcg(st, contrib, target, &par, st->material == 0, end));
      hipLaunchKernelGGL(opimp_newton_update_kernel, dim3(nbd), dim3(kThreads), 0, op->stream, n, st->status + (par ? kStS1 : kStS0),
                         st->xcg, st->p, st->x, st->status + kStCg);
      SAA_HIP_TRY(hipGetLastError());
      previous = rnorm;
      ++info->newton_iterations;
      solved = st->material == 0 && end[kSLive] == 0.0 && end[kSGuard] == 0.0 && end[kSNorm] <= target ? end[kSNorm] : -1.0;
    }
    if (reason != 0) {
      info->converged = 0;
      info->reason = reason;
      break;
    }
    hipLaunchKernelGGL(opimp_finish_kernel, dim3(nbd), dim3(kThreads), 0, op->stream, n, st->minv, st->x, st->d, st->v, st->a, dt, c2,
                       c4, st->traj, st->n_cols, recorder_column(st));
    SAA_HIP_TRY(hipGetLastError());
    st->t += dt;
    ++st->step_index;
    ++info->steps_done;
  }
  return hipStreamSynchronize(op->stream);
}

}  // namespace saa
