"""Counterpart of the reference's ``Tools/Steady_solvers.py``: the steady solve and the modal analysis.

``Steady_Elasticity_solver`` keeps the reference's signature (``Steady_solvers.py:13``) and returns the same
``(3N,1)`` array, but never forms the dense ``(3N)^2`` matrix of ``Global_Assembly``: the system is solved by
preconditioned conjugate gradients on the GPU with the matrix-free element kernel as the operator.  ``Eigen_mode`` keeps the reference's signature and output
(``Steady_solvers.py:25-40``); its lowest modes come from shift-invert subspace iteration on the GPU block apply
(:mod:`..modal`) instead of a dense ``eigh`` of the ``(3N)^2`` pair.

Both take ``p = 1`` (4-node cells) and ``p = 2`` (10-node cells in the reference's local order,
``Shape_function_Deriv.py:14-23``).  For ``p = 2`` the work goes through an order-2 operator handle
(:class:`..modal.ModalOperator`): ``K`` and the load with the reference's 4-point rule, ``M`` with the 14-point rule
(the reference's 4-point mass is singular)."""
from __future__ import annotations

import numpy as np

from ..fem_setup import device_setup_fields
from ..modal import ModalOperator, device_lowest_modes
from ..solver import HipExplicitSolver
from ..steady import steady_solve, steady_solve_operator, stiffness_diagonal


def _cells10(Cells):
    """The 10-node cells of a ``p = 2`` call.  Cells with fewer columns are not elevated here (the reference does not
    either: it would index past them): elevate the mesh first, ``mesh.to_quadratic``."""
    Cells = np.asarray(Cells)
    if Cells.ndim != 2 or Cells.shape[1] < 10:
        raise NotImplementedError("p = 2 takes 10-node cells; 4-node cells are not elevated here (mesh.to_quadratic does it)")
    return np.ascontiguousarray(Cells[:, :10], dtype=np.int32)


def Steady_Elasticity_solver(p, Cells, Points, Dirichlet, elas, t=None, Facets=None, Neumann=None, device=0,
                             tol=1e-12):
    """Solve ``K d = F`` with ``d[Dirichlet] = 0`` (``Steady_solvers.py:13-22``).  ``Cells`` hold global node ids,
    ``Dirichlet`` global dofs (``node_to_dof``), ``elas`` the un-ramped ``elasticity`` object
    (``Data_prepare.py:161``); ``p`` is 1 (4-node cells) or 2 (10-node cells)."""
    if p not in (1, 2):
        raise NotImplementedError("linear and quadratic tetrahedra only on the GPU path")
    if Neumann is not None or Facets is not None:
        raise NotImplementedError("the reference passes Facets=None, Neumann=None (Data_prepare.py:163)")
    Points = np.ascontiguousarray(Points, dtype=np.float64)
    scale = 1.0
    if getattr(elas, "R", False) and t is not None:  # ramped load evaluated at time t (commons.py:35-41)
        scale = t if t <= 1 else 1.0
    if p == 2:
        Cells = _cells10(Cells)
        dirichlet = np.asarray(sorted(Dirichlet), dtype=np.int32)
        with ModalOperator(Points, Cells, dirichlet, elas.lmd, elas.mu, elas.rho, device) as op:
            d, _, _ = steady_solve_operator(op, op.load((0.0, -elas.fz * scale, -elas.fz * scale)), tol=tol)
        return d.reshape(-1, 1)
    Cells = np.ascontiguousarray(np.asarray(Cells)[:, :4], dtype=np.int32)
    lumped, load, _ = device_setup_fields(Points, Cells, elas.rho, elas.fz * scale, device)
    dirichlet = np.asarray(sorted(Dirichlet), dtype=np.int32)
    sol = HipExplicitSolver(Points, Cells, lumped, load, dirichlet, elas.lmd, elas.mu, 1.0, 0.0, device=device)
    try:
        d, _, _ = steady_solve(sol, load, dirichlet, diag=stiffness_diagonal(Points, Cells, elas.lmd, elas.mu), tol=tol)
    finally:
        sol.close()
    return d


def Eigen_mode(deg, Cells, Points, Dirichlet, elas, t=None, Facets=None, Neumann=None, device=0, tol=1e-8):
    """Print the first 50 natural frequencies ``sqrt(omega^2)/2pi`` of the reference's matrix pair and return 0
    (``Steady_solvers.py:25-40``).

    In that pair ``Global_Assembly`` leaves out the Dirichlet rows and columns of ``K`` and ``M``
    (``Mat_construction.py:176-192``) and ``Eigen_mode`` puts 1 on ``M``'s diagonal there, so its spectrum is the reduced
    problem ``K x = omega^2 M x`` on the free dofs plus ``n_D`` zero frequencies, which come first.  They are printed as
    exact zeros (the reference's dense ``eigh`` gives round-off there, whose square root may be nan), followed by the
    lowest ``50 - n_D`` frequencies of the reduced problem (:func:`modal.lowest_modes`, relative residual ``tol``).
    Printed with 16 digits, ``np.printoptions(precision=16)``.

    ``deg = 2``: the same on 10-node cells, with the 14-point consistent mass in place of the reference's singular
    4-point one (with which the reference's own ``eigh(K, M)`` fails)."""
    if deg not in (1, 2):
        raise NotImplementedError("linear and quadratic tetrahedra only on the GPU path")
    if Neumann is not None or Facets is not None:
        raise NotImplementedError("the reference passes Facets=None, Neumann=None")
    Points = np.ascontiguousarray(Points, dtype=np.float64)
    Cells = _cells10(Cells) if deg == 2 else np.ascontiguousarray(np.asarray(Cells)[:, :4], dtype=np.int32)
    dirichlet = np.unique(np.asarray(list(Dirichlet), dtype=np.int64))
    n_dof = 3 * len(Points)
    n_print = min(50, n_dof)
    n_zero = min(len(dirichlet), n_print)
    freqs = np.zeros(n_print)
    k = min(n_print - n_zero, n_dof - len(dirichlet))
    if k > 0:
        with ModalOperator(Points, Cells, dirichlet, elas.lmd, elas.mu, elas.rho, device) as op:
            modes = device_lowest_modes(op, Points, Cells, elas.lmd, elas.mu, k, tol=tol)
        freqs[n_zero:n_zero + k] = modes["frequencies_hz"]
    with np.printoptions(precision=16):
        print(freqs)
    return 0
