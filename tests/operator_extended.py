"""Extended-precision reference of everything the ``saa_operator`` handle computes at orders 1 and 2, the cases that take
the operator kernels off the unit beam, and the bar they are held to.  Shared by tests/test_operator_extended.py (CPU) and
tests/test_gpu_operator_extended.py.  Lives under tests/: the product never imports it.

The reference.  :class:`Extended` is plain NumPy in ``np.longdouble`` (64-bit significand on x86-64): ``K X``, ``M X``, load
and diagonals; stress, von Mises and energy with totals, maxima and argmaxima; the volume-weighted nodal average; ``eta^2``
in both forms.  It is written so that nothing it does loses more than the working precision:

* coordinates are converted first and the element's first node is subtracted before the Jacobian is formed (the shape
  function derivatives sum to zero, so the Jacobian does not change);
* inverses are explicit adjugates (``np.linalg`` does not take longdouble);
* von Mises comes from ``2 mu (eps_i - eps_j)``, and the compliance form ``t^T C t`` is the sum of squares
  ``|dev t|^2 / (2 mu) + tr(t)^2 / (3 (3 lambda + 2 mu))``;
* every contraction is a Python loop over the small index with elementwise arithmetic on the large ones: no ``einsum``,
  ``dot`` or ``bincount`` (an einsum longdouble statement on un-centred coordinates at shift 1e6 agreed with its centred
  self only to 1.1e-10).

Shape functions and quadrature rules are the float64 tables of the package's ``Tools`` (the numbers the kernels' own
compile-time tables hold), converted exactly.  The same class runs in three more arithmetics: ``np.float64`` (the "stable
restatement"), ``np.float64`` with ``kernel_order=True`` (the two forms the kernels used before: von Mises from ``s_i -
s_j`` after ``lambda tr(eps)`` went into both, and the compliance as ``t.t - lambda / (3 lambda + 2 mu) tr^2``; only there
to prove that the bar can fail), and ``MP`` (object arrays of ``mpmath.mpf``, which checks the longdouble run itself).

Order 1 goes through the same statements as order 2: the linear element is the isoparametric element with four nodes, one
stress point (its stress is constant) and the 4-point rule for the mass and for the integral of the quadratic ``d^T C d``
of the nodal error form, which that rule integrates exactly.

The bar.  Per output field ``y`` against the reference ``r``, column by column, ``err = max|y - r| / max|r|`` has to stay
below ``1e-12 + 8 env``.  1e-12 is the project's own bar (``TOL`` of tests/test_gpu_p2_stress.py).  ``env`` is what rounding
the inputs once already costs: the largest relative change of ``r`` over 8 seeded draws in which every floating-point input
(coordinates, columns, ``lambda``, ``mu``, ``rho``, the force density) is multiplied by ``1 + d``, ``d`` uniform in
``+-2^-53``.  The factor 8 allows a backward-stable kernel several roundings per input; it is a condition, not a
measurement.  The bar is only meaningful where the stable float64 restatement stays within ``1e-12 + 2 env`` and ``env <=
1e-6``: tests/test_operator_extended.py asserts both on every case."""
from __future__ import annotations

import functools

import numpy as np

from synchronization_avoiding_algorithms_amd.Tools.Qudrature import Gauss_Legendre
from synchronization_avoiding_algorithms_amd.Tools.Shape_function_Deriv import Shape_Deri, Shape_Function
from synchronization_avoiding_algorithms_amd.mesh import TET10_EDGES

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no extended type here: the reference would be float64"

MP = "mp"                      # the arithmetic of mpmath.mpf objects (at the caller's mpmath.mp.prec)
TOL = 1e-12
KERNEL_FACTOR, STABLE_FACTOR, ENV_MAX, N_DRAWS = 8.0, 2.0, 1e-6, 8
N_COLUMNS = 5
FORCE = (1.0, -2.0, 0.5)


# ----------------------------------------------------------------------------------------------------------------------
# Arithmetic
# ----------------------------------------------------------------------------------------------------------------------

def conv(a, T):
    """``a`` in the arithmetic ``T`` (exact from float64 and from longdouble)."""
    if T is not MP:
        return np.asarray(a, dtype=T)
    import mpmath

    a = np.asarray(a)
    if a.dtype == object:
        return a
    hi = np.asarray(a, dtype=np.float64)
    lo = np.asarray(np.asarray(a, dtype=np.longdouble) - hi, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mpmath.mpf(float(hi[idx])) + mpmath.mpf(float(lo[idx]))
    return out


def scalar(x, T):
    return conv(x, T)[()]


def zeros(shape, T):
    if T is not MP:
        return np.zeros(shape, dtype=T)
    import mpmath

    out = np.empty(shape, dtype=object)
    out[...] = mpmath.mpf(0)
    return out


def sqrt(a, T):
    if T is not MP:
        return np.sqrt(a)
    import mpmath

    return np.frompyfunc(mpmath.sqrt, 1, 1)(a)


def log(a, T):
    if T is not MP:
        return np.log(a)
    import mpmath

    return np.frompyfunc(mpmath.log, 1, 1)(a)


def log1p(a, T):
    if T is not MP:
        return np.log1p(a)
    import mpmath

    return np.frompyfunc(mpmath.log1p, 1, 1)(a)


def to_longdouble(a):
    """An array of any of the arithmetics as longdouble (mpf: rounded through a float64 pair, 106 bits)."""
    a = np.asarray(a)
    if a.dtype != object:
        return np.asarray(a, dtype=np.longdouble)
    out = np.empty(a.shape, dtype=np.longdouble)
    for idx in np.ndindex(a.shape):
        hi = float(a[idx])
        out[idx] = np.longdouble(hi) + np.longdouble(float(a[idx] - hi))
    return out


def inverse3(J):
    """``(J^-1, det J)`` of ``J (..., 3, 3)`` by the adjugate, elementwise."""
    c00 = J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1]
    c01 = J[..., 1, 2] * J[..., 2, 0] - J[..., 1, 0] * J[..., 2, 2]
    c02 = J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]
    det = J[..., 0, 0] * c00 + J[..., 0, 1] * c01 + J[..., 0, 2] * c02
    G = np.empty_like(J)
    G[..., 0, 0], G[..., 1, 0], G[..., 2, 0] = c00 / det, c01 / det, c02 / det
    G[..., 0, 1] = (J[..., 0, 2] * J[..., 2, 1] - J[..., 0, 1] * J[..., 2, 2]) / det
    G[..., 1, 1] = (J[..., 0, 0] * J[..., 2, 2] - J[..., 0, 2] * J[..., 2, 0]) / det
    G[..., 2, 1] = (J[..., 0, 1] * J[..., 2, 0] - J[..., 0, 0] * J[..., 2, 1]) / det
    G[..., 0, 2] = (J[..., 0, 1] * J[..., 1, 2] - J[..., 0, 2] * J[..., 1, 1]) / det
    G[..., 1, 2] = (J[..., 0, 2] * J[..., 1, 0] - J[..., 0, 0] * J[..., 1, 2]) / det
    G[..., 2, 2] = (J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]) / det
    return G, det


def inverse_small(A, T):
    """Inverse of a small square matrix by Gauss-Jordan with partial pivoting, on scalars of ``T``."""
    n = len(A)
    M = [[A[i][j] for j in range(n)] + [scalar(1.0 if i == j else 0.0, T) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        M[c] = [v / piv for v in M[c]]
        for r in range(n):
            if r != c:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    out = zeros((n, n), T)
    for i in range(n):
        for j in range(n):
            out[i, j] = M[i][n + j]
    return out


def tables(order, n_quad, T):
    """``(w (nq,), N (nq, na), dN (nq, na, 3))`` of ``Gauss_Legendre(n_quad)``; ``n_quad = 0``: the centroid with the whole
    weight 1/6 (the one stress point of the linear element)."""
    if n_quad == 0:
        xi, w = np.full((1, 3), 0.25), np.array([1.0 / 6.0])
    else:
        xi, w = Gauss_Legendre(n_quad)
    N = np.array([Shape_Function(order, x) for x in xi], dtype=np.float64)
    dN = np.array([Shape_Deri(order, x) for x in xi], dtype=np.float64)
    return conv(w, T), conv(N, T), conv(dN, T)


# ----------------------------------------------------------------------------------------------------------------------
# The operator
# ----------------------------------------------------------------------------------------------------------------------

class Extended:
    """The handle's outputs on ``points (n, 3)``, ``cells (ne, 4 or 10)`` in the arithmetic ``T``; no Dirichlet dofs.
    Columns are ``(m, 3 n)`` arrays.  Stress fields have the shapes of ``stress.StressRecovery`` (order 1: ``sigma (m, ne,
    6)``) and ``stress.QuadraticStressRecovery`` (order 2: ``sigma (m, ne, 4, 6)``, point index ``4 e + q``)."""

    def __init__(self, points, cells, lmd, mu, rho, T=np.longdouble, kernel_order=False):
        self.T, self.kernel_order = T, bool(kernel_order)
        self.cells = np.asarray(cells, dtype=np.int64)
        self.n_nodes, (self.n_elems, self.na) = len(points), self.cells.shape
        self.order = 2 if self.na == 10 else 1
        self.lmd, self.mu, self.rho = scalar(lmd, T), scalar(mu, T), scalar(rho, T)
        P = conv(points, T)[self.cells]
        self.Pc = P - P[:, :1]                                         # centred on the element's first node
        self.wk, self.Nk, self.dNk = tables(self.order, 2 if self.order == 2 else 0, T)
        self.wm, self.Nm, self.dNm = tables(self.order, 4 if self.order == 2 else 2, T)
        self.nq = len(self.wk)
        Gk, self.detk = inverse3(self._jacobian(self.dNk))             # (ne, nq, 3, 3), (ne, nq)
        _, self.detm = inverse3(self._jacobian(self.dNm))
        self.grad = zeros((self.n_elems, self.nq, self.na, 3), T)      # grad N_a = dN_a/dxi J^-1
        for j in range(3):
            for k in range(3):
                self.grad[..., k] = self.grad[..., k] + self.dNk[None, :, :, j] * Gk[:, :, None, j, k]
        self.wdk = self.wk[None, :] * self.detk                        # signed, as K, M and the load use it
        self.wdm = self.wm[None, :] * self.detm
        self.vol = zeros(self.n_elems, T)                              # |V_e| = sum_q w_q |detJ_q|
        for q in range(self.nq):
            self.vol = self.vol + np.abs(self.wdk[:, q])
        if self.order == 2:                                            # vertex values of the linear field through 4 points
            xi = conv(Gauss_Legendre(2)[0], T)                         # barycentric weights that sum to one in T itself
            L4 = zeros((4, 4), T)
            for q in range(4):
                L4[q, 1:] = xi[q]
                L4[q, 0] = 1 - xi[q, 0] - xi[q, 1] - xi[q, 2]
            self.L4inv = inverse_small(L4, T)                          # c_v = sum_q L4inv[v, q] sigma_q

    def _jacobian(self, dN):
        J = zeros((self.n_elems, len(dN), 3, 3), self.T)               # J[i, j] = sum_a x_a[i] dN_a/dxi_j
        for a in range(self.na):
            for i in range(3):
                for j in range(3):
                    J[:, :, i, j] = J[:, :, i, j] + self.Pc[:, None, a, i] * dN[None, :, a, j]
        return J

    def min_det(self):
        """The smallest ``detJ`` over the points of both rules (a valid element: > 0)."""
        return min(self.detk.min(), self.detm.min())

    # ---- scatter / gather --------------------------------------------------------------------------------------------
    def _nodes(self, X):
        X = conv(X, self.T)
        return X.reshape(len(X), self.n_nodes, 3)[:, self.cells]      # (m, ne, na, 3)

    def _scatter(self, contrib):
        """``contrib (m, ne, na, 3)`` summed into ``(m, 3 n)``."""
        out = zeros((contrib.shape[0], 3 * self.n_nodes), self.T)
        for a in range(self.na):
            for c in range(3):
                np.add.at(out, (slice(None), 3 * self.cells[:, a] + c), contrib[:, :, a, c])
        return out

    # ---- K X, M X, load, diagonals -----------------------------------------------------------------------------------
    def _grad_u(self, U):
        H = zeros(U.shape[:2] + (self.nq, 3, 3), self.T)               # H[i, k] = sum_a u_a[i] dN_a/dx_k
        for a in range(self.na):
            for i in range(3):
                for k in range(3):
                    H[..., i, k] = H[..., i, k] + U[:, :, None, a, i] * self.grad[None, :, :, a, k]
        return H

    def apply_k(self, X):
        H = self._grad_u(self._nodes(X))
        ltr = self.lmd * (H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2])
        f = zeros(H.shape[:2] + (self.na, 3), self.T)
        for i in range(3):
            for k in range(3):
                s = self.mu * (H[..., i, k] + H[..., k, i]) + (ltr if i == k else 0)
                for q in range(self.nq):
                    f[..., i] = f[..., i] + (self.wdk[None, :, q] * s[:, :, q])[:, :, None] * self.grad[None, :, q, :, k]
        return self._scatter(f)

    def apply_m(self, X):
        U = self._nodes(X)
        f = zeros(U.shape, self.T)
        for q in range(len(self.wm)):
            val = zeros(U.shape[:2] + (3,), self.T)
            for a in range(self.na):
                val = val + self.Nm[q, a] * U[:, :, a]
            for a in range(self.na):
                f[:, :, a] = f[:, :, a] + (self.rho * self.wdm[None, :, q, None] * self.Nm[q, a]) * val
        return self._scatter(f)

    def load(self, force):
        fv = conv(np.asarray(force), self.T)
        s = zeros((self.n_elems, self.na), self.T)
        if self.order == 2:
            for q in range(self.nq):
                s = s + self.wdk[:, q, None] * self.Nk[None, q, :]
        else:                                                          # the 4-point rule, exact: V / 4
            for q in range(len(self.wm)):
                s = s + self.wdm[:, q, None] * self.Nm[None, q, :]
        return self._scatter((s[:, :, None] * fv[None, None, :])[None])[0]

    def diagonals(self):
        g2 = self.grad[..., 0] ** 2 + self.grad[..., 1] ** 2 + self.grad[..., 2] ** 2      # (ne, nq, na)
        dk = zeros((self.n_elems, self.na, 3), self.T)
        for q in range(self.nq):
            for k in range(3):
                gk2 = self.grad[:, q, :, k] ** 2
                dk[:, :, k] = dk[:, :, k] + self.wdk[:, q, None] * (self.lmd * gk2 + self.mu * (g2[:, q] + gk2))
        dm = zeros((self.n_elems, self.na, 3), self.T)
        for q in range(len(self.wm)):
            dm = dm + (self.rho * self.wdm[:, q, None] * self.Nm[None, q, :] ** 2)[:, :, None]
        return self._scatter(dk[None])[0], self._scatter(dm[None])[0]

    # ---- stress ------------------------------------------------------------------------------------------------------
    def _field(self, S):
        """Stress input as ``(m, ne, nq, 6)`` in ``T``."""
        S = conv(S, self.T)
        return S.reshape(S.shape[0], self.n_elems, self.nq, 6)

    def _out(self, S):
        return S[:, :, 0] if self.order == 1 else S

    def element(self, X):
        H = self._grad_u(self._nodes(X))
        eps = [H[..., 0, 0], H[..., 1, 1], H[..., 2, 2], H[..., 1, 2] + H[..., 2, 1], H[..., 0, 2] + H[..., 2, 0],
               H[..., 0, 1] + H[..., 1, 0]]
        ltr = self.lmd * (eps[0] + eps[1] + eps[2])
        two_mu = 2 * self.mu
        s = [ltr + two_mu * eps[0], ltr + two_mu * eps[1], ltr + two_mu * eps[2], self.mu * eps[3], self.mu * eps[4],
             self.mu * eps[5]]
        if self.kernel_order:
            d01, d12, d20 = s[0] - s[1], s[1] - s[2], s[2] - s[0]
        else:
            d01, d12, d20 = two_mu * (eps[0] - eps[1]), two_mu * (eps[1] - eps[2]), two_mu * (eps[2] - eps[0])
        vm = sqrt((d01 * d01 + d12 * d12 + d20 * d20) / 2 + 3 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]), self.T)
        dens = s[0] * eps[0] + s[1] * eps[1] + s[2] * eps[2] + s[3] * eps[3] + s[4] * eps[4] + s[5] * eps[5]
        W = zeros(dens.shape[:2], self.T)
        for q in range(self.nq):
            W = W + np.abs(self.wdk[None, :, q]) * dens[:, :, q] / 2
        sigma = zeros(dens.shape + (6,), self.T)
        for c in range(6):
            sigma[..., c] = s[c]
        flat = vm.reshape(vm.shape[0], -1)
        return {"sigma": self._out(sigma), "von_mises": self._out(vm), "energy": W, "energy_total": _sum(W, self.T),
                "von_mises_max": flat.max(axis=1), "von_mises_argmax": np.asarray(flat.argmax(axis=1), dtype=np.int64)}

    def _corner_delta(self, S):
        """``(r, delta)`` with ``sigma_h(node a) = r + delta_a``: ``r (m, ne, 6)`` the first point's value and ``delta (m, ne,
        na, 6)`` the element stress field at the element's nodes relative to it (order 1: zero, the field is constant; order
        2: the linear field through the four Gauss values at the vertices, the mean of its two vertices at an edge node).
        Formed from the differences ``S_q - r``, which are exact, so that a large common value never rounds a small
        variation; the weights of a vertex sum to one."""
        S = self._field(S)
        r = S[:, :, 0]
        delta = zeros(S.shape[:2] + (self.na, 6), self.T)
        if self.order == 2:
            for v in range(4):
                for q in range(1, 4):
                    delta[:, :, v] = delta[:, :, v] + self.L4inv[v, q] * (S[:, :, q] - r)
            for k, (a, b) in enumerate(TET10_EDGES):
                delta[:, :, 4 + k] = (delta[:, :, a] + delta[:, :, b]) / 2
        return r, delta

    def corner_values(self, S):
        """``(m, ne, na, 6)``: the element stress field ``sigma_h`` at the element's nodes."""
        r, delta = self._corner_delta(S)
        return r[:, :, None] + delta

    def nodal(self, S):
        """``(m, n, 6)``: the ``|V_e|``-weighted mean of :meth:`corner_values` over a node's elements."""
        corner = self.corner_values(S)
        num, den = zeros((corner.shape[0], self.n_nodes, 6), self.T), zeros(self.n_nodes, self.T)
        for a in range(self.na):
            np.add.at(num, (slice(None), self.cells[:, a]), self.vol[None, :, None] * corner[:, :, a])
            np.add.at(den, self.cells[:, a], self.vol)
        den = np.where(den == 0, 1, den)                               # (a node without elements: 0, as the kernels give)
        return num / den[None, :, None]

    def compliance(self, t):
        """``t^T C t`` of ``t (..., 6)``, ``C = D^-1`` with engineering shear."""
        shear = t[..., 3] * t[..., 3] + t[..., 4] * t[..., 4] + t[..., 5] * t[..., 5]
        tr = t[..., 0] + t[..., 1] + t[..., 2]
        three_k = 3 * self.lmd + 2 * self.mu
        if self.kernel_order:
            nn = t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1] + t[..., 2] * t[..., 2]
            return ((nn - (self.lmd / three_k) * (tr * tr)) + 2 * shear) / (2 * self.mu)
        d01, d12, d20 = t[..., 0] - t[..., 1], t[..., 1] - t[..., 2], t[..., 2] - t[..., 0]
        return ((d01 * d01 + d12 * d12 + d20 * d20) / 3 + 2 * shear) / (2 * self.mu) + (tr * tr) / (3 * three_k)

    def error(self, S, nodal=None, other=None):
        """``eta2 (m, ne)`` with total, maximum and argmax: against the nodal field (interpolated with the element's own
        shape functions, integrated with the mass rule) or against a second element field (the stress rule)."""
        if (nodal is None) == (other is None):
            raise ValueError("exactly one of nodal and other is needed")
        if nodal is not None:
            Nd = conv(nodal, self.T)
            r, delta = self._corner_delta(S)
            d = (Nd.reshape(Nd.shape[0], self.n_nodes, 6)[:, self.cells] - r[:, :, None]) - delta  # (m, ne, na, 6)
            eta2 = zeros(d.shape[:2], self.T)
            for p in range(len(self.wm)):
                dp = zeros(d.shape[:2] + (6,), self.T)
                for a in range(self.na):
                    dp = dp + self.Nm[p, a] * d[:, :, a]
                eta2 = eta2 + np.abs(self.wdm[None, :, p]) * self.compliance(dp)
        else:
            d = self._field(other) - self._field(S)
            eta2 = zeros(d.shape[:2], self.T)
            for q in range(self.nq):
                eta2 = eta2 + np.abs(self.wdk[None, :, q]) * self.compliance(d[:, :, q])
        return {"eta2": eta2, "eta2_total": _sum(eta2, self.T), "eta2_max": eta2.max(axis=1),
                "eta2_argmax": np.asarray(eta2.argmax(axis=1), dtype=np.int64)}

    # ---- the linear element's matrix (element_bound) -----------------------------------------------------------------
    def element_btdb(self):
        """``B^T D B (ne, 12, 12)`` of the linear element, dof ``3 a + i``: ``omega_e^2 = (4 / rho) lambda_max`` of it."""
        assert self.order == 1
        g = self.grad[:, 0]                                            # (ne, 4, 3)
        B = zeros((self.n_elems, 6, 12), self.T)
        for a in range(4):
            B[:, 0, 3 * a], B[:, 1, 3 * a + 1], B[:, 2, 3 * a + 2] = g[:, a, 0], g[:, a, 1], g[:, a, 2]
            B[:, 3, 3 * a + 1], B[:, 3, 3 * a + 2] = g[:, a, 2], g[:, a, 1]
            B[:, 4, 3 * a], B[:, 4, 3 * a + 2] = g[:, a, 2], g[:, a, 0]
            B[:, 5, 3 * a], B[:, 5, 3 * a + 1] = g[:, a, 1], g[:, a, 0]
        DB = zeros(B.shape, self.T)
        tr = self.lmd * (B[:, 0] + B[:, 1] + B[:, 2])
        for c in range(3):
            DB[:, c] = tr + 2 * self.mu * B[:, c]
            DB[:, 3 + c] = self.mu * B[:, 3 + c]
        A = zeros((self.n_elems, 12, 12), self.T)
        for c in range(6):
            A = A + B[:, c, :, None] * DB[:, c, None, :]
        return A


def _sum(a, T):
    out = zeros(a.shape[0], T)
    for e in range(a.shape[1]):
        out = out + a[:, e]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------

MESHES_P1 = ("structured2", "delaunay2")
MESHES_P2 = ("beam36", "straight288", "curved288")
MESHES = MESHES_P1 + MESHES_P2
NUS = (-0.3, 0.0, 0.3, 0.49, 0.4999, 0.499999)
SHIFTS = (10, 20)                                                      # s = 2^10, 2^20
UNITS = (+1, -1)                                                       # coordinates and columns 2^(40 u), lambda, mu 4^(10 u), rho 2^(20 u)


def case_ids():
    """Every (mesh, family, value) of the bar families; the units family (bitwise, no bar) is apart."""
    out = [(m, "nu", nu) for m in MESHES for nu in NUS]
    out += [(m, "shift", s) for m in MESHES for s in SHIFTS]
    out += [(m, "needle", 1e-3) for m in MESHES]
    out += [(m, "sliver", 1e-6) for m in MESHES]
    out += [(m, "curved", 0.2) for m in ("beam36", "straight288")]
    return out


def case_name(cid):
    m, fam, val = cid
    return f"{m}-{fam}-{val:g}"


@functools.lru_cache(maxsize=None)
def base_mesh(name):
    from conftest import load_golden
    from synchronization_avoiding_algorithms_amd.mesh import delaunay_beam, structured_beam, to_quadratic

    if name == "structured2":
        m = structured_beam(2)
        return m.points.copy(), np.asarray(m.tets, dtype=np.int64)
    if name == "delaunay2":
        m = delaunay_beam(2)
        return m.points.copy(), np.asarray(m.tets, dtype=np.int64)
    if name == "beam36":
        q = to_quadratic(structured_beam(1, length=6.0))
        return q.points.copy(), np.asarray(q.tets10, dtype=np.int64)
    g = load_golden("p2_beam.npz")
    return g["points_straight" if name == "straight288" else "points_curved"].copy(), np.asarray(g["cells10"], dtype=np.int64)


def _volume_h3(p):
    """``(V, h^3)`` of the straight tetrahedron ``p (4, 3)``: signed volume and the cube of its longest edge."""
    V = np.dot(p[1] - p[0], np.cross(p[2] - p[0], p[3] - p[0])) / 6.0
    h = max(np.linalg.norm(p[a] - p[b]) for a in range(4) for b in range(a))
    return V, h ** 3


def make_slivers(points, cells, ratio=1e-6, every=5):
    """Corner 3 of every ``every``-th element moved along the line to the centroid of the opposite face until ``V / h^3 =
    ratio`` (h the longest edge), the orientation kept.  The corner becomes a node of that element alone, so that no
    neighbour is distorted or inverted; at order 2 so do its six mid-edge nodes, on the mid-points of the straight edges."""
    points, cells = [p for p in np.asarray(points, dtype=np.float64)], np.array(cells, dtype=np.int64)
    for e in range(0, len(cells), every):
        p = np.array([points[v] for v in cells[e, :4]])
        c = p[:3].mean(axis=0)
        V0, _ = _volume_h3(p)
        assert V0 > 0
        t, q = 1.0, p.copy()
        for _ in range(8):                                             # V is linear in t, h nearly constant: a fixed point
            q[3] = c + t * (p[3] - c)
            t = ratio * _volume_h3(q)[1] / V0
        q[3] = c + t * (p[3] - c)
        cells[e, 3] = len(points)
        points.append(q[3])
        if cells.shape[1] == 10:
            for k, (a, b) in enumerate(TET10_EDGES):
                cells[e, 4 + k] = len(points)
                points.append(0.5 * (q[a] + q[b]))
    return np.array(points), cells


def make_curved(points, cells10, amount=0.2):
    """Every mid-edge node moved by ``amount`` of the edge length along a unit normal of the edge: the part of the z
    direction (of -x for an edge along z) that is perpendicular to the edge, so that neighbouring edges bend the same way.
    Normals that alternate in sign invert elements at 0.2; these do not (build_case asserts every detJ > 0)."""
    points = np.array(points, dtype=np.float64)
    done = set()
    for e in range(len(cells10)):
        for k, (a, b) in enumerate(TET10_EDGES):
            n = int(cells10[e, 4 + k])
            if n in done:
                continue
            done.add(n)
            t = points[cells10[e, b]] - points[cells10[e, a]]
            d = np.array([0.0, 0.0, 1.0] if np.abs(t[:2]).max() > 1e-9 * np.abs(t).max() else [-1.0, 0.0, 0.0])
            nrm = d - (d @ t) / (t @ t) * t
            points[n] = points[n] + amount * np.linalg.norm(t) * nrm / np.linalg.norm(nrm)
    return points


def lame(E, nu):
    return E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), E / (2.0 * (1.0 + nu))


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """The inputs of one case, all float64: ``points``, ``cells``, ``lmd``, ``mu``, ``rho``, ``force``, the displacement
    columns ``X`` and ``X_other (5, 3 n)``, and the stress fields that the node and error passes are given, which are the
    reference's own results rounded to float64: ``sig``, ``sig_other`` (element fields of ``X``, ``X_other``), ``nod`` (the
    nodal recovery of ``sig``), and ``psig``, ``pnod``: the same pair of the confined compression ``u = (a x, 0, 0)`` plus
    1e-3 of noise, whose difference is pressure-dominated at high ``nu``."""
    mesh, family, value = cid
    points, cells = base_mesh(mesh)
    E, nu, rho = 1e6, 0.3, 1.0
    if family == "nu":
        nu = value
    if family == "sliver":
        points, cells = make_slivers(points, cells, value)
    if family == "curved":
        points = make_curved(points, cells, value)
    n = len(points)
    seed = 1000 + sum(ord(c) for c in case_name(cid))
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, size=(N_COLUMNS, 3 * n)) * 1e-3
    X_other = rng.uniform(-0.5, 0.5, size=(N_COLUMNS, 3 * n)) * 1e-3
    a = 1e-3 * (1.0 + np.arange(N_COLUMNS))
    XP = np.zeros((N_COLUMNS, n, 3))
    XP[:, :, 0] = a[:, None] * points[None, :, 0]
    XP = XP.reshape(N_COLUMNS, -1)
    XP = XP + 1e-3 * np.abs(XP).max(axis=1, keepdims=True) * rng.uniform(-1.0, 1.0, size=XP.shape)
    if family == "needle":
        points = points * np.array([1.0, value, 1.0])
    if family == "shift":
        s = 2.0 ** value
        points = points + np.array([s, -s, s / 3.0])
    lmd, mu = lame(E, nu)
    case = {"id": cid, "points": np.ascontiguousarray(points), "cells": cells, "lmd": lmd, "mu": mu, "rho": rho,
            "force": np.array(FORCE), "X": X, "X_other": X_other}
    ext = Extended(points, cells, lmd, mu, rho)
    assert ext.min_det() > 0, (cid, ext.min_det())                     # every Gauss-point detJ of every case is positive
    r64 = lambda v: np.asarray(v, dtype=np.float64)
    case["sig"], case["sig_other"] = r64(ext.element(X)["sigma"]), r64(ext.element(X_other)["sigma"])
    case["nod"] = r64(ext.nodal(case["sig"]))
    case["psig"] = r64(ext.element(XP)["sigma"])
    case["pnod"] = r64(ext.nodal(case["psig"]))
    return case


FLOAT_INPUTS = ("points", "lmd", "mu", "rho", "force", "X", "X_other", "sig", "sig_other", "nod", "psig", "pnod")
ARG_OF = {"von_mises_argmax": "von_mises", "zz.eta2_argmax": "zz.eta2", "other.eta2_argmax": "other.eta2",
          "press.eta2_argmax": "press.eta2"}
PER_HANDLE = ("load", "diag_k", "diag_m")                              # one column each


def outputs(case, T=np.longdouble, kernel_order=False, only=None):
    """name -> array of every output of the handle on the case's inputs, in the arithmetic ``T``."""
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], T, kernel_order)
    out = {}
    if only is None or "apply" in only:
        out["kx"], out["mx"] = ext.apply_k(case["X"]), ext.apply_m(case["X"])
        out["load"] = ext.load(case["force"])
        out["diag_k"], out["diag_m"] = ext.diagonals()
    if only is None or "stress" in only:
        out.update(ext.element(case["X"]))
        out["nodal"] = ext.nodal(case["sig"])
    if only is None or "error" in only:
        for tag, res in (("zz", ext.error(case["sig"], nodal=case["nod"])),
                         ("other", ext.error(case["sig"], other=case["sig_other"])),
                         ("press", ext.error(case["psig"], nodal=case["pnod"]))):
            out.update({f"{tag}.{k}": v for k, v in res.items()})
    return out


def _columns(name, a):
    a = np.asarray(a)
    return a.reshape(1, -1) if name in PER_HANDLE else a.reshape(a.shape[0], -1)


def perturbed(case, rng):
    """The case with every floating-point input times ``1 + d``, ``d`` uniform in ``+-2^-53``, held in longdouble."""
    out = dict(case)
    for k in FLOAT_INPUTS:
        v = np.asarray(case[k], dtype=np.longdouble)
        d = np.asarray(rng.uniform(-1.0, 1.0, size=v.shape), dtype=np.longdouble) * np.longdouble(2.0) ** -53
        out[k] = v * (1 + d)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """``(case, ref, env)``: the longdouble outputs and, per floating-point output, ``env (columns,)``."""
    case = build_case(cid)
    ref = outputs(case)
    rng = np.random.default_rng(77)
    env = {k: np.zeros(len(_columns(k, v))) for k, v in ref.items() if k not in ARG_OF}
    for _ in range(N_DRAWS):
        alt = outputs(perturbed(case, rng))
        for k in env:
            r, a = _columns(k, ref[k]), _columns(k, alt[k])
            env[k] = np.maximum(env[k], np.asarray(np.abs(a - r).max(axis=1) / np.abs(r).max(axis=1), dtype=np.float64))
    return case, ref, env


def errors(name, got, ref):
    """``err (columns,)`` of one floating-point output against the reference, the difference taken in longdouble."""
    r = _columns(name, ref)
    g = _columns(name, np.asarray(got, dtype=np.longdouble))
    assert g.shape == r.shape, (name, g.shape, r.shape)
    return np.asarray(np.abs(g - r).max(axis=1) / np.abs(r).max(axis=1), dtype=np.float64)


def check(got, ref, env, factor, label, names=None, verbose=True):
    """Hold every output of ``got`` to ``err <= 1e-12 + factor env`` (argmaxima: the reference's value at the index is its
    maximum up to the bar).  Prints ``err``, ``env`` and ``err / env`` per output; returns name -> (worst err, its env)."""
    worst, bad = {}, []
    for name in (names or [k for k in ref if k in got]):
        if name in ARG_OF:
            field = ARG_OF[name]
            r = _columns(field, ref[field])
            idx = np.asarray(got[name], dtype=np.int64).reshape(-1)
            assert ((0 <= idx) & (idx < r.shape[1])).all(), (label, name, idx)
            bar = TOL + factor * env[field]
            at = r[np.arange(len(idx)), idx]
            if not (at >= r.max(axis=1) * (1 - bar)).all():
                bad.append((name, idx.tolist()))
            continue
        err = errors(name, got[name], ref[name])
        j = int(np.argmax(err - (TOL + factor * env[name])))
        worst[name] = (float(err[j]), float(env[name][j]))
        if verbose:
            print(f"{label:34s} {name:18s} err {err[j]:.2e}  env {env[name][j]:.2e}  err/env {err[j] / max(env[name][j], 1e-300):.2e}")
        if not (err <= TOL + factor * env[name]).all():
            bad.append((name, float(err[j]), float(env[name][j])))
    return worst, bad


# ----------------------------------------------------------------------------------------------------------------------
# Units: power-of-two scalings that every kernel must commute with bit for bit
# ----------------------------------------------------------------------------------------------------------------------

def scaled_case(case, u):
    """Coordinates and displacements times ``2^(40 u)``, ``lambda`` and ``mu`` times ``4^(10 u)``, ``rho`` times ``2^(20 u)``
    (stresses therefore times ``2^(20 u)``)."""
    L, S, R = 2.0 ** (40 * u), 4.0 ** (10 * u), 2.0 ** (20 * u)
    out = dict(case)
    out["points"] = case["points"] * L
    for k in ("X", "X_other"):
        out[k] = case[k] * L
    out["lmd"], out["mu"], out["rho"] = case["lmd"] * S, case["mu"] * S, case["rho"] * R
    for k in ("sig", "sig_other", "nod", "psig", "pnod"):
        out[k] = case[k] * S
    return out


# exponent of 2 (per unit u) that each output picks up: length 40, stress 20, density 20
_L, _S, _R = 40, 20, 20
UNIT_EXPONENT = {"kx": _S + 2 * _L, "mx": _R + 4 * _L, "load": 3 * _L, "diag_k": _S + _L, "diag_m": _R + 3 * _L,
                 "sigma": _S, "von_mises": _S, "von_mises_max": _S, "energy": _S + 3 * _L, "energy_total": _S + 3 * _L,
                 "nodal": _S, "omega_e": (_S - _R - 2 * _L) // 2, "omega_max": (_S - _R - 2 * _L) // 2}
for _tag in ("zz", "other", "press"):
    for _k in ("eta2", "eta2_total", "eta2_max"):
        UNIT_EXPONENT[f"{_tag}.{_k}"] = _S + 3 * _L


# ----------------------------------------------------------------------------------------------------------------------
# A few elements of a case on their own (the mpmath check), and the element bound
# ----------------------------------------------------------------------------------------------------------------------

def sub_mesh(points, cells, n_elems=4):
    """``(nodes, points, cells)`` of the first ``n_elems`` elements as a mesh of their own: the nodes they use (sorted, in
    the numbering of the whole mesh), those nodes' coordinates and the cells renumbered to them."""
    cells = np.asarray(cells)[:n_elems]
    nodes, inv = np.unique(cells, return_inverse=True)
    return nodes, np.asarray(points)[nodes], inv.reshape(cells.shape)


def sub_case(case, n_elems=4, n_columns=2):
    """The first ``n_elems`` elements of a case as a mesh of their own (nodes renumbered), with ``n_columns`` columns."""
    nodes, points, cells = sub_mesh(case["points"], case["cells"], n_elems)
    dof = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    out = dict(case)
    out["points"], out["cells"] = points, cells
    for k in ("X", "X_other"):
        out[k] = case[k][:n_columns][:, dof]
    for k in ("sig", "sig_other", "psig"):
        out[k] = case[k][:n_columns, :n_elems]
    for k in ("nod", "pnod"):
        out[k] = case[k][:n_columns][:, nodes]
    return out


BOUND_MESHES = MESHES_P1


def bound_case_ids():
    return [(m, "nu", nu) for m in BOUND_MESHES for nu in NUS] + [(m, "needle", 1e-3) for m in BOUND_MESHES] + \
           [(m, "sliver", 1e-6) for m in BOUND_MESHES]


def element_omega(case, T=np.longdouble):
    """``omega_e (ne,)`` float64: ``sqrt((4 / rho) lambda_max(B^T D B))`` with ``B^T D B`` built in ``T``, rounded to float64
    and given to ``eigvalsh`` (symmetric eigenvalues are perfectly conditioned)."""
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], T)
    A = np.asarray(ext.element_btdb(), dtype=np.float64)
    scale = np.abs(A).max(axis=(1, 2), keepdims=True)                  # (eigvalsh on entries of order 1: a power of two)
    scale = 2.0 ** np.round(np.log2(scale))
    lam = np.linalg.eigvalsh(A / scale)[:, -1] * scale[:, 0, 0]
    return np.sqrt(4.0 / float(case["rho"]) * lam)


@functools.lru_cache(maxsize=None)
def bound_reference(cid):
    """``(case, omega_e, env)`` of the element bound: env is one number, the field has one column."""
    case = build_case(cid)
    ref = element_omega(case)
    rng = np.random.default_rng(78)
    env = 0.0
    for _ in range(N_DRAWS):
        alt = perturbed(case, rng)
        env = max(env, float(np.abs(element_omega(alt) - ref).max() / ref.max()))
    return case, ref, env


def omega_true(case):
    """``omega_max`` of ``K x = omega^2 M_L x`` on all dofs of the case's order-1 mesh (no Dirichlet dofs), by the dense
    generalised eigensolver on the matrix assembled from the longdouble element matrices."""
    import scipy.linalg as sl

    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"])
    vol = np.asarray(ext.wdk[:, 0], dtype=np.float64)                  # signed V_e (positive on every case)
    Ke = np.asarray(ext.element_btdb(), dtype=np.float64) * vol[:, None, None]
    cells, n = ext.cells, ext.n_nodes
    dof = (3 * cells[:, :, None] + np.arange(3)[None, None, :]).reshape(len(cells), 12)
    K = np.zeros((3 * n, 3 * n))
    np.add.at(K, (dof[:, :, None], dof[:, None, :]), Ke)
    mass = np.zeros(n)
    np.add.at(mass, cells.ravel(), np.repeat(float(case["rho"]) * np.abs(vol) / 4.0, 4))
    s = 1.0 / np.sqrt(np.repeat(mass, 3))
    A = K * s[:, None] * s[None, :]
    top = sl.eigh(0.5 * (A + A.T), eigvals_only=True, subset_by_index=[3 * n - 1, 3 * n - 1])[0]
    return float(np.sqrt(top))
