// gfx950 kernels of the modal analysis: the stable time step of the explicit solver and the lowest vibration modes.
//
//  * elem_bound_kernel - one element per lane: omega_e^2 = lambda_max(K_e) / (rho |V_e| / 4) = (4/rho) lambda_max(B^T D B),
//    the element's highest frequency with its share of the lumped mass.  The nonzero spectrum of the 12x12 B^T D B is that
//    of the 6x6 L^T (B B^T) L (D = L L^T, factored once on the host), which cyclic Jacobi diagonalises in fp64 registers.
//    max_e omega_e bounds omega_max of M_L^-1 K from above when every signed volume is > 0 (Irons-Treharne); the
//    maximum and its element come from a two-stage reduction (per workgroup, then one workgroup) with no float atomics.
//  * elem_apply_kernel + node_sum_kernel - K X and / or M X for up to 16 columns.  K is the element stiffness of
//    Local_K_coronary (/root/reference Tools/Mat_construction.py:79-119, signed detJ :93), M the consistent mass
//    rho V/20 (1 + delta_ab) I_3 that the 4-point rule of Tools/Qudrature.py:6-12 integrates exactly (Local_MKF,
//    Mat_construction.py:23-76).  The element pass evaluates the geometry once for all columns and writes every
//    (element, corner) contribution; the node pass sums a node's contributions in ascending element order through the
//    node -> (element, corner) CSR - the pattern of saa_setup.hip, bitwise repeatable and free of scattered fp64 atomics.
//    Dirichlet dofs are masked: inputs there are read as 0, outputs there are 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <new>
#include <vector>

#include "saa_hip_host.h"
#include "saa_modal.h"
#include "saa_modal_op.h"
#include "saa_stress_dev.h"

namespace saa {

namespace {

struct CholD {
  double l[21];  // lower triangle of L, row by row
};

__device__ __forceinline__ double lij(const CholD &L, int i, int j) { return j > i ? 0.0 : L.l[i * (i + 1) / 2 + j]; }

// lambda_max of the symmetric 6x6 `a` by cyclic Jacobi (rotations as in Golub & Van Loan 8.5); all indices are
// compile-time after unrolling, so `a` lives in registers.
__device__ __forceinline__ double jacobi_max_eig6(double a[6][6]) {
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      diag += a[p][p] * a[p][p];
#pragma unroll
      for (int q = p + 1; q < 6; ++q) off += a[p][q] * a[p][q];
    }
    if (!(off > 1e-34 * diag)) break;  // (also ends on NaN)
#pragma unroll
    for (int p = 0; p < 5; ++p) {
#pragma unroll
      for (int q = p + 1; q < 6; ++q) {
        const double apq = a[p][q];
        if (apq != 0.0) {
          const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
          const double at = fabs(theta);
          double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
          if (theta < 0.0) t = -t;
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] -= t * apq;
          a[q][q] += t * apq;
          a[p][q] = a[q][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            if (r == p || r == q) continue;
            const double arp = a[r][p], arq = a[r][q];
            const double np = c * arp - s * arq, nq = s * arp + c * arq;
            a[r][p] = a[p][r] = np;
            a[r][q] = a[q][r] = nq;
          }
        }
      }
    }
  }
  double m = a[0][0];
#pragma unroll
  for (int p = 1; p < 6; ++p) m = a[p][p] > m ? a[p][p] : m;
  return m;
}

// wave, then workgroup (kThreads lanes) reduction of (max, argmax, count); the result is valid in thread 0
__device__ __forceinline__ void block_reduce(double &v, int32_t &i, int32_t &cnt) {
  __shared__ double sv[kWaves];
  __shared__ int32_t si[kWaves], sc[kWaves];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int32_t oi = __shfl_xor(i, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
    max_merge(v, i, ov, oi);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[w] = v;
    si[w] = i;
    sc[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kWaves; ++k) {
      max_merge(v, i, sv[k], si[k]);
      cnt += sc[k];
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(kThreads) elem_bound_kernel(int32_t n_elems, const double *__restrict__ xyz,
                                                              const int32_t *__restrict__ tets, CholD L, double four_over_rho,
                                                              double *__restrict__ omega_e, double *__restrict__ part_val,
                                                              int32_t *__restrict__ part_idx, int32_t *__restrict__ part_cnt) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  double best = -1.0;
  int32_t arg = INT32_MAX, cnt = 0;
  if (e < n_elems) {
    int32_t v[4];
    double g[4][3];
    const double det = element_gradients(xyz, tets, e, v, g);
    cnt = det > 0.0 ? 0 : 1;
    // S = sum_a g_a g_a^T, then G = B B^T (B rows xx, yy, zz, yz, xz, xy: Mat_construction.py:99-104) in terms of S
    double sxx = 0, syy = 0, szz = 0, sxy = 0, sxz = 0, syz = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      sxx += g[a][0] * g[a][0];
      syy += g[a][1] * g[a][1];
      szz += g[a][2] * g[a][2];
      sxy += g[a][0] * g[a][1];
      sxz += g[a][0] * g[a][2];
      syz += g[a][1] * g[a][2];
    }
    const double G[6][6] = {{sxx, 0.0, 0.0, 0.0, sxz, sxy},           {0.0, syy, 0.0, syz, 0.0, sxy},
                            {0.0, 0.0, szz, syz, sxz, 0.0},           {0.0, syz, syz, syy + szz, sxy, sxz},
                            {sxz, 0.0, sxz, sxy, sxx + szz, syz},     {sxy, sxy, 0.0, sxz, syz, sxx + syy}};
    // A = L^T G L
    double GL[6][6], A[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = j; k < 6; ++k) s += G[i][k] * lij(L, k, j);
        GL[i][j] = s;
      }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = i; k < 6; ++k) s += lij(L, k, i) * GL[k][j];
        A[i][j] = A[j][i] = s;
      }
    const double w = sqrt(four_over_rho * jacobi_max_eig6(A));
    if (omega_e) omega_e[e] = w;
    best = w;
    arg = (int32_t)e;
  }
  block_reduce(best, arg, cnt);
  if (threadIdx.x == 0) {
    part_val[blockIdx.x] = best;
    part_idx[blockIdx.x] = arg;
    part_cnt[blockIdx.x] = cnt;
  }
}

__global__ void __launch_bounds__(kThreads) bound_final_kernel(int32_t n_parts, const double *__restrict__ part_val,
                                                               const int32_t *__restrict__ part_idx,
                                                               const int32_t *__restrict__ part_cnt, double *__restrict__ res_val,
                                                               int32_t *__restrict__ res_int) {
  double best = -1.0;
  int32_t arg = INT32_MAX, cnt = 0;
  for (int32_t k = threadIdx.x; k < n_parts; k += kThreads) {  // fixed assignment of partials to lanes: deterministic
    max_merge(best, arg, part_val[k], part_idx[k]);
    cnt += part_cnt[k];
  }
  block_reduce(best, arg, cnt);
  if (threadIdx.x == 0) {
    res_val[0] = best;
    res_int[0] = arg;
    res_int[1] = cnt;
  }
}

// Element pass of the block apply: contributions of element e to its four corners, column by column; out_* layout
// [column][4 * e + corner][component].
template <bool DO_K, bool DO_M>
__global__ void __launch_bounds__(kThreads) elem_apply_kernel(int32_t n_elems, int32_t m, const double *__restrict__ xyz,
                                                              const int32_t *__restrict__ tets, const double *__restrict__ free_mask,
                                                              double lam, double mu, double rho, const double *__restrict__ x,
                                                              int64_t ldx, double *__restrict__ out_k, double *__restrict__ out_m) {
  const int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (e >= n_elems) return;
  int32_t v[4];
  double g[4][3];
  const double det = element_gradients(xyz, tets, e, v, g);
  const double vol = det / 6.0;  // signed, like the reference's detJ
  const double mscale = rho * vol / 20.0;
  double fm[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) fm[a][c] = free_mask[3 * (int64_t)v[a] + c];
  const int64_t stride = 12 * (int64_t)n_elems;
  for (int32_t j = 0; j < m; ++j) {
    const double *xj = x + j * ldx;
    double u[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) u[a][c] = fm[a][c] * xj[3 * (int64_t)v[a] + c];
    if (DO_K) {
      // H = grad u, sigma = lam tr(H) I + mu (H + H^T) (commons.py:25-31), f_a = V sigma grad N_a
      double h[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[i][k] = u[0][i] * g[0][k] + u[1][i] * g[1][k] + u[2][i] * g[2][k] + u[3][i] * g[3][k];
      const double ltr = lam * (h[0][0] + h[1][1] + h[2][2]);
      double s[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[i][k] = vol * (mu * (h[i][k] + h[k][i]) + (i == k ? ltr : 0.0));
      double *o = out_k + j * stride + 12 * e;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i) o[3 * a + i] = s[i][0] * g[a][0] + s[i][1] * g[a][1] + s[i][2] * g[a][2];
    }
    if (DO_M) {
      double *o = out_m + j * stride + 12 * e;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double sum = (u[0][c] + u[1][c]) + (u[2][c] + u[3][c]);
#pragma unroll
        for (int a = 0; a < 4; ++a) o[3 * a + c] = mscale * (u[a][c] + sum);
      }
    }
  }
}

// Node pass: y[j][3v + c] = sum of node v's (element, corner) contributions in ascending element order; 0 on Dirichlet dofs.
__global__ void __launch_bounds__(kThreads) node_sum_kernel(int32_t n_nodes, int32_t m, const int64_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ pairs, const double *__restrict__ free_mask,
                                                            const double *__restrict__ contrib, int64_t stride, double *__restrict__ y,
                                                            int64_t ldy) {
  const int64_t v = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (v >= n_nodes) return;
  const int64_t b = offsets[v], end = offsets[v + 1];
  const double f0 = free_mask[3 * v], f1 = free_mask[3 * v + 1], f2 = free_mask[3 * v + 2];
  for (int32_t j = 0; j < m; ++j) {
    const double *cj = contrib + j * stride;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t i = b; i < end; ++i) {
      const double *q = cj + 3 * (int64_t)pairs[i];
      s0 += q[0];
      s1 += q[1];
      s2 += q[2];
    }
    double *yj = y + j * ldy + 3 * v;
    yj[0] = f0 != 0.0 ? s0 : 0.0;
    yj[1] = f1 != 0.0 ? s1 : 0.0;
    yj[2] = f2 != 0.0 ? s2 : 0.0;
  }
}

void modal_destroy(ModalOp *op) {
  if (!op) return;
  (void)hipSetDevice(op->device);
  void *bufs[] = {op->xyz, op->tets, op->free_mask, op->offsets, op->pairs, op->scratch_k, op->scratch_m,
                  op->part_val, op->part_idx, op->part_cnt, op->res_val, op->res_int, op->abs_vol, op->node_wsum,
                  op->st_part_w, op->st_part_vm, op->st_part_idx, op->geom, op->bits, op->fs_count, op->st_inverted,
                  op->dt_cnt, op->imp_part};
  for (void *b : bufs)
    if (b) (void)hipFree(b);
  delete op;
}

int modal_device(const ModalOp *op) { return op->device; }
int32_t modal_n_nodes(const ModalOp *op) { return op->n_nodes; }
void modal_set_stream(ModalOp *op, hipStream_t stream) { op->stream = stream; }

hipError_t modal_create(int device, int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets,
                        const int32_t *dirichlet_dofs, int32_t n_dirichlet, double lambda_, double mu, double rho,
                        ModalOp **out, std::string &err, int order) {
  *out = nullptr;
  // D (commons.py:25-31, Voigt xx, yy, zz, yz, xz, xy) = L L^T
  double D[6][6] = {};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) D[i][j] = lambda_;
    D[i][i] = lambda_ + 2.0 * mu;
    D[i + 3][i + 3] = mu;
  }
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double d = D[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) {
      err = "saa_operator_create: the elasticity matrix D is not positive definite (need mu > 0, 3 lambda + 2 mu > 0)";
      return hipErrorInvalidValue;
    }
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = D[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  // node -> (element, corner) CSR by a counting sort: entries of a node in ascending element order
  const int64_t n_pairs = (order == 2 ? 10 : 4) * static_cast<int64_t>(n_elems);
  std::vector<int64_t> offsets(static_cast<size_t>(n_nodes) + 1, 0);
  for (int64_t i = 0; i < n_pairs; ++i) ++offsets[static_cast<size_t>(tets[i]) + 1];
  for (int32_t v = 0; v < n_nodes; ++v) offsets[v + 1] += offsets[v];
  std::vector<int32_t> pairs(static_cast<size_t>(n_pairs));
  {
    std::vector<int64_t> pos(offsets.begin(), offsets.end() - 1);
    for (int64_t i = 0; i < n_pairs; ++i) pairs[static_cast<size_t>(pos[tets[i]]++)] = static_cast<int32_t>(i);
  }
  std::vector<double> mask(3 * static_cast<size_t>(n_nodes), 1.0);
  for (int32_t k = 0; k < n_dirichlet; ++k) mask[dirichlet_dofs[k]] = 0.0;

  ModalOp *op = new (std::nothrow) ModalOp;
  if (!op) return hipErrorOutOfMemory;
  op->device = device;
  op->order = order;
  op->n_nodes = n_nodes;
  op->n_elems = n_elems;
  op->lam = lambda_;
  op->mu = mu;
  op->rho = rho;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) op->L[i][j] = L[i][j];
  const int64_t n_parts = (n_elems + kThreads - 1) / kThreads;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = dev_alloc(&op->xyz, 3 * static_cast<size_t>(n_nodes));
  if (e == hipSuccess) e = dev_alloc(&op->tets, static_cast<size_t>(n_pairs));
  if (e == hipSuccess) e = dev_alloc(&op->free_mask, 3 * static_cast<size_t>(n_nodes));
  if (e == hipSuccess) e = dev_alloc(&op->offsets, static_cast<size_t>(n_nodes) + 1);
  if (e == hipSuccess) e = dev_alloc(&op->pairs, static_cast<size_t>(n_pairs));
  if (e == hipSuccess) e = dev_alloc(&op->part_val, static_cast<size_t>(n_parts));
  if (e == hipSuccess) e = dev_alloc(&op->part_idx, static_cast<size_t>(n_parts));
  if (e == hipSuccess) e = dev_alloc(&op->part_cnt, static_cast<size_t>(n_parts));
  if (e == hipSuccess) e = dev_alloc(&op->res_val, 1);
  if (e == hipSuccess) e = dev_alloc(&op->res_int, 2);
  if (e == hipSuccess) e = hipMemcpy(op->xyz, xyz, 3 * static_cast<size_t>(n_nodes) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && n_pairs)
    e = hipMemcpy(op->tets, tets, static_cast<size_t>(n_pairs) * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(op->free_mask, mask.data(), mask.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(op->offsets, offsets.data(), offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && n_pairs)
    e = hipMemcpy(op->pairs, pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    modal_destroy(op);
    return e;
  }
  *out = op;
  return hipSuccess;
}

namespace {
hipError_t ensure_scratch(double **buf, int32_t *cap, int32_t m, int32_t n_elems) {
  if (*cap >= m) return hipSuccess;
  if (*buf) {
    SAA_HIP_TRY(hipDeviceSynchronize());  // (a launch still reading the old buffer)
    SAA_HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
  }
  SAA_HIP_TRY(dev_alloc(buf, 12 * static_cast<size_t>(n_elems) * static_cast<size_t>(m)));
  *cap = m;
  return hipSuccess;
}
}  // namespace

hipError_t modal_apply(ModalOp *op, int32_t m, const double *x, int64_t ldx, double *kx, double *mx, int64_t ldy) {
  if (kx) SAA_HIP_TRY(ensure_scratch(&op->scratch_k, &op->cap_k, m, op->n_elems));
  if (mx) SAA_HIP_TRY(ensure_scratch(&op->scratch_m, &op->cap_m, m, op->n_elems));
  const int64_t stride = 12 * static_cast<int64_t>(op->n_elems);
  if (op->n_elems > 0) {
    const dim3 grid(static_cast<unsigned>((op->n_elems + kThreads - 1) / kThreads));
    if (kx && mx)
      hipLaunchKernelGGL((elem_apply_kernel<true, true>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                         op->free_mask, op->lam, op->mu, op->rho, x, ldx, op->scratch_k, op->scratch_m);
    else if (kx)
      hipLaunchKernelGGL((elem_apply_kernel<true, false>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                         op->free_mask, op->lam, op->mu, op->rho, x, ldx, op->scratch_k, nullptr);
    else
      hipLaunchKernelGGL((elem_apply_kernel<false, true>), grid, dim3(kThreads), 0, op->stream, op->n_elems, m, op->xyz, op->tets,
                         op->free_mask, op->lam, op->mu, op->rho, x, ldx, nullptr, op->scratch_m);
    SAA_HIP_TRY(hipGetLastError());
  }
  const dim3 ngrid(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads));
  if (kx)
    hipLaunchKernelGGL(node_sum_kernel, ngrid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs, op->free_mask,
                       op->scratch_k, stride, kx, ldy);
  if (mx)
    hipLaunchKernelGGL(node_sum_kernel, ngrid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs, op->free_mask,
                       op->scratch_m, stride, mx, ldy);
  return hipGetLastError();
}

hipError_t modal_elem_pass_k(ModalOp *op, const double *x, double *contrib) {
  if (op->n_elems == 0) return hipSuccess;
  const dim3 grid(static_cast<unsigned>((op->n_elems + kThreads - 1) / kThreads));
  hipLaunchKernelGGL((elem_apply_kernel<true, false>), grid, dim3(kThreads), 0, op->stream, op->n_elems, 1, op->xyz, op->tets,
                     op->free_mask, op->lam, op->mu, op->rho, x, static_cast<int64_t>(0), contrib, nullptr);
  return hipGetLastError();
}

hipError_t modal_node_sum(ModalOp *op, int32_t m, const double *contrib, int64_t stride, double *y, int64_t ldy) {
  const dim3 ngrid(static_cast<unsigned>((op->n_nodes + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(node_sum_kernel, ngrid, dim3(kThreads), 0, op->stream, op->n_nodes, m, op->offsets, op->pairs, op->free_mask,
                     contrib, stride, y, ldy);
  return hipGetLastError();
}

hipError_t modal_element_bound(ModalOp *op, double *omega_e, double *omega_max, int32_t *argmax, int32_t *n_nonpositive) {
  const int32_t n_parts = (op->n_elems + kThreads - 1) / kThreads;
  CholD L;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) L.l[i * (i + 1) / 2 + j] = op->L[i][j];
  if (n_parts > 0) {
    hipLaunchKernelGGL(elem_bound_kernel, dim3(static_cast<unsigned>(n_parts)), dim3(kThreads), 0, op->stream, op->n_elems, op->xyz,
                       op->tets, L, 4.0 / op->rho, omega_e, op->part_val, op->part_idx, op->part_cnt);
    SAA_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(bound_final_kernel, dim3(1), dim3(kThreads), 0, op->stream, n_parts, op->part_val, op->part_idx, op->part_cnt,
                     op->res_val, op->res_int);
  SAA_HIP_TRY(hipGetLastError());
  double val = 0.0;
  int32_t ints[2] = {0, 0};
  SAA_HIP_TRY(hipMemcpyAsync(&val, op->res_val, sizeof(double), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipMemcpyAsync(ints, op->res_int, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, op->stream));
  SAA_HIP_TRY(hipStreamSynchronize(op->stream));
  if (omega_max) *omega_max = val;
  if (argmax) *argmax = ints[0] == INT32_MAX ? -1 : ints[0];
  if (n_nonpositive) *n_nonpositive = ints[1];
  return hipSuccess;
}

}  // namespace saa
