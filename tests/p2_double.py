"""NumPy statement of the quadratic (10-node) tetrahedron: the element formulas of the reference's ``Local_MKF(2, 10, ...)``
(``Tools/Mat_construction.py:23-76``) vectorised over elements, and the matrix-free ``K X``, ``M X``, load and diagonals
that ``csrc/saa_p2.hip`` computes.  ``K`` and the load use ``Gauss_Legendre(2)`` (4 points) like the reference, ``M`` uses
``Gauss_Legendre(4)`` (14 points; ``mass_rule=2`` gives the reference's singular 4-point mass).  Shape functions and
rules come from the package's ``Tools`` (pinned against the reference by tests/test_tools_dropin.py).

Used by the CPU tests against the reference's fixture (tests/golden/p2_beam.npz), and on the GPU at sizes where the
reference's dense route is impossible."""
from __future__ import annotations

import numpy as np

from synchronization_avoiding_algorithms_amd.Tools.Qudrature import Gauss_Legendre
from synchronization_avoiding_algorithms_amd.Tools.Shape_function_Deriv import Shape_Deri, Shape_Function


def tables(n_quad):
    """``(w (nq,), N (nq,10), dN (nq,10,3))`` of the rule ``Gauss_Legendre(n_quad)``."""
    xi, w = Gauss_Legendre(n_quad)
    return w, np.array([Shape_Function(2, x) for x in xi]), np.array([Shape_Deri(2, x) for x in xi])


def geometry(points, cells10, n_quad):
    """``(w detJ (ne,nq), grad N (ne,nq,10,3), N (nq,10))``: ``J[i,j] = sum_a x_a[i] dN_a/dxi_j`` from all ten nodes,
    ``grad N = dN/dxi J^-1`` (``Mat_construction.py:38-42``), detJ signed."""
    w, N, dN = tables(n_quad)
    P = np.asarray(points, dtype=np.float64)[np.asarray(cells10)]                    # (ne, 10, 3)
    J = np.einsum("eai,qaj->eqij", P, dN)
    g = np.einsum("qaj,eqjk->eqak", dN, np.linalg.inv(J))
    return w[None, :] * np.linalg.det(J), g, N


def _free(n_dof, dirichlet):
    free = np.ones(n_dof)
    if len(dirichlet):
        free[np.asarray(dirichlet, dtype=np.int64)] = 0.0
    return free


def _scatter(cells10, contrib, n_nodes):
    """``contrib (..., ne, 10, 3)`` summed into ``(..., 3 n_nodes)``."""
    dof = (3 * np.asarray(cells10)[:, :, None] + np.arange(3)[None, None, :]).ravel()
    lead = contrib.shape[:-3]
    flat = contrib.reshape(-1, dof.size)
    out = np.stack([np.bincount(dof, weights=row, minlength=3 * n_nodes) for row in flat])
    return out.reshape(*lead, 3 * n_nodes)


def apply_k(points, cells10, dirichlet, lmd, mu, X):
    """``K X`` for the rows of ``X (m, 3n)`` with Dirichlet rows and columns masked."""
    n = len(points)
    free = _free(3 * n, dirichlet)
    wd, g, _ = geometry(points, cells10, 2)
    U = (np.atleast_2d(X) * free).reshape(-1, n, 3)[:, np.asarray(cells10)]         # (m, ne, 10, 3)
    H = np.einsum("meai,eqak->meqik", U, g)                                          # grad u
    tr = np.trace(H, axis1=3, axis2=4)
    S = mu * (H + np.swapaxes(H, 3, 4)) + lmd * tr[..., None, None] * np.eye(3)      # commons.py:25-31
    f = np.einsum("eq,meqik,eqak->meai", wd, S, g)
    return _scatter(cells10, f, n) * free


def apply_m(points, cells10, dirichlet, rho, X, mass_rule=4):
    """``M X`` with the consistent mass of the 14-point rule (``mass_rule=2``: the reference's 4-point mass)."""
    n = len(points)
    free = _free(3 * n, dirichlet)
    wd, _, N = geometry(points, cells10, mass_rule)
    U = (np.atleast_2d(X) * free).reshape(-1, n, 3)[:, np.asarray(cells10)]
    val = np.einsum("qa,meai->meqi", N, U)
    f = rho * np.einsum("eq,qa,meqi->meai", wd, N, val)
    return _scatter(cells10, f, n) * free


def load(points, cells10, dirichlet, f):
    """Consistent body-force vector ``sum_q w detJ N_a f`` with the K rule (``Fe`` of ``Local_MKF`` assembled)."""
    n = len(points)
    wd, _, N = geometry(points, cells10, 2)
    s = np.einsum("eq,qa->ea", wd, N)
    return _scatter(cells10, s[:, :, None] * np.asarray(f, dtype=np.float64).reshape(1, 1, 3), n) * _free(3 * n, dirichlet)


def diagonals(points, cells10, dirichlet, lmd, mu, rho):
    """``(diag K, diag M)`` of the masked operator."""
    n = len(points)
    free = _free(3 * n, dirichlet)
    wd, g, _ = geometry(points, cells10, 2)
    g2 = (g ** 2).sum(axis=3, keepdims=True)
    dk = np.einsum("eq,eqak->eak", wd, lmd * g ** 2 + mu * (g2 + g ** 2))
    wd14, _, N14 = geometry(points, cells10, 4)
    dm = rho * np.einsum("eq,qa->ea", wd14, N14 ** 2)[:, :, None] * np.ones(3)
    return _scatter(cells10, dk, n) * free, _scatter(cells10, dm, n) * free


def element_matrices(points, cells10, lmd, mu, rho, f, mass_rule=4):
    """``(Me, Ke, Fe)`` per element, ``(ne,30,30)``, ``(ne,30,30)``, ``(ne,30)``, dof ``3 a + A`` (``Local_MKF``)."""
    wd, g, N = geometry(points, cells10, 2)
    ne, nq = wd.shape
    B = np.zeros((ne, nq, 6, 10, 3))                                                  # Mat_construction.py:48-53
    B[:, :, 0, :, 0] = g[..., 0]
    B[:, :, 1, :, 1] = g[..., 1]
    B[:, :, 2, :, 2] = g[..., 2]
    B[:, :, 3, :, 1], B[:, :, 3, :, 2] = g[..., 2], g[..., 1]
    B[:, :, 4, :, 0], B[:, :, 4, :, 2] = g[..., 2], g[..., 0]
    B[:, :, 5, :, 0], B[:, :, 5, :, 1] = g[..., 1], g[..., 0]
    B = B.reshape(ne, nq, 6, 30)
    D = np.zeros((6, 6))
    D[:3, :3] = lmd
    D[np.arange(3), np.arange(3)] = lmd + 2.0 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    Ke = np.einsum("eq,eqsp,st,eqtr->epr", wd, B, D, B)
    Fe = (np.einsum("eq,qa->ea", wd, N)[:, :, None] * np.asarray(f, dtype=np.float64).reshape(1, 1, 3)).reshape(ne, 30)
    wdm, _, Nm = geometry(points, cells10, mass_rule)
    Me = rho * np.einsum("eq,qa,qb->eab", wdm, Nm, Nm)
    Me = np.einsum("eab,AB->eaAbB", Me, np.eye(3)).reshape(ne, 30, 30)
    return Me, Ke, Fe


def assemble(points, cells10, dirichlet, lmd, mu, rho, mass_rule=4):
    """Dense ``(K, M)`` of a small mesh with Dirichlet rows and columns left out (zero), like ``Global_Assembly``."""
    n = len(points)
    Me, Ke, _ = element_matrices(points, cells10, lmd, mu, rho, (0.0, 0.0, 0.0), mass_rule)
    dof = (3 * np.asarray(cells10)[:, :, None] + np.arange(3)[None, None, :]).reshape(len(cells10), 30)
    K, M = np.zeros((3 * n, 3 * n)), np.zeros((3 * n, 3 * n))
    np.add.at(K, (dof[:, :, None], dof[:, None, :]), Ke)
    np.add.at(M, (dof[:, :, None], dof[:, None, :]), Me)
    free = _free(3 * n, dirichlet)
    return K * free[:, None] * free[None, :], M * free[:, None] * free[None, :]


def pcg(apply, b, diag, tol=1e-13, max_iter=20000):
    """Jacobi-PCG on a callable: ``(x, iterations)``."""
    minv = np.where(diag > 0, 1.0 / np.where(diag > 0, diag, 1.0), 0.0)
    x = np.zeros_like(b)
    r = b.copy()
    z = minv * r
    p = z.copy()
    rz = r @ z
    bn = np.linalg.norm(b)
    for it in range(1, max_iter + 1):
        ap = apply(p)
        alpha = rz / (p @ ap)
        x += alpha * p
        r -= alpha * ap
        if np.linalg.norm(r) <= tol * bn:
            return x, it
        z = minv * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_iter
