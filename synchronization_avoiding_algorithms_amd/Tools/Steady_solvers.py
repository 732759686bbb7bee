"""Counterpart of the reference's ``Tools/Steady_solvers.py``: the steady solve and the modal analysis.

``Steady_Elasticity_solver`` keeps the reference's signature (``Steady_solvers.py:13``) and returns the same
``(3N,1)`` array, but never forms the dense ``(3N)^2`` matrix of ``Global_Assembly``: the system is solved by
preconditioned conjugate gradients on the GPU with the matrix-free element kernel as the operator.  ``Eigen_mode`` keeps the reference's signature and output
(``Steady_solvers.py:25-40``); its lowest modes come from shift-invert subspace iteration on the GPU block apply
(:mod:`..modal`) instead of a dense ``eigh`` of the ``(3N)^2`` pair."""
from __future__ import annotations

import numpy as np

from ..fem_setup import device_setup_fields
from ..modal import ModalOperator, device_lowest_modes
from ..solver import HipExplicitSolver
from ..steady import steady_solve, stiffness_diagonal


def Steady_Elasticity_solver(p, Cells, Points, Dirichlet, elas, t=None, Facets=None, Neumann=None, device=0,
                             tol=1e-12):
    """Solve ``K d = F`` with ``d[Dirichlet] = 0`` (``Steady_solvers.py:13-22``).  ``Cells`` hold global node ids,
    ``Dirichlet`` global dofs (``node_to_dof``), ``elas`` the un-ramped ``elasticity`` object
    (``Data_prepare.py:161``); ``p`` must be 1 here (linear tetrahedra)."""
    if p != 1:
        raise NotImplementedError("linear tetrahedra only on the GPU path")
    if Neumann is not None or Facets is not None:
        raise NotImplementedError("the reference passes Facets=None, Neumann=None (Data_prepare.py:163)")
    Points = np.ascontiguousarray(Points, dtype=np.float64)
    Cells = np.ascontiguousarray(np.asarray(Cells)[:, :4], dtype=np.int32)
    scale = 1.0
    if getattr(elas, "R", False) and t is not None:  # ramped load evaluated at time t (commons.py:35-41)
        scale = t if t <= 1 else 1.0
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
    Printed with 16 digits, ``np.printoptions(precision=16)``."""
    if deg != 1:
        raise NotImplementedError("linear tetrahedra only on the GPU path")
    if Neumann is not None or Facets is not None:
        raise NotImplementedError("the reference passes Facets=None, Neumann=None")
    Points = np.ascontiguousarray(Points, dtype=np.float64)
    Cells = np.ascontiguousarray(np.asarray(Cells)[:, :4], dtype=np.int32)
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
