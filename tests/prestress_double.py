"""Dense float64 double of the prestressed modal analysis: ``K_T(u) x = omega^2 M x`` with the dense tangent of
``tangent_double.Tangent.tangent_matrix``, the dense consistent mass of the handle and ``scipy.linalg.eigh``.  Shared by
tests/test_prestress.py (CPU) and tests/test_gpu_prestress.py.  Lives under tests/: the product never imports it; it is not a
test.

The load case: the 6 x 1 x 1 beams ``structured288`` (order 1) and ``beam36`` (order 2), clamped on ``x = 0``, under the axial
body force ``(fx, 0, 0)``, ``fx = -2000`` (compression) and ``+2000`` (tension); equilibria from ``tangent_double.newton`` in four
load steps.  ``3 u*(fx = -2000)`` is a state (not an equilibrium) at which the tangent has negative eigenvalues and no element is
inverted."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import p2_double
import tangent_double as td

LMD, MU = fd.lame(fd.E, fd.NU)
MESHES = ("structured288", "beam36")
FX = (-2000.0, 2000.0)
# lowest omega^2 over the unstressed value, to the digits of the float64 run that sized the tests: [fx][mesh][material]
RATIO = {-2000.0: {"structured288": {"svk": 0.590, "neo_hookean": 0.628}, "beam36": {"svk": 0.336, "neo_hookean": 0.378}},
         2000.0: {"structured288": {"svk": 1.402, "neo_hookean": 1.365}, "beam36": {"svk": 1.650, "neo_hookean": 1.609}}}
# lowest omega^2 at 3 u*(fx = -2000) and the number of negative eigenvalues there
UNSTABLE = {"structured288": {"svk": -286.0, "neo_hookean": -196.0, "negative": 1},
            "beam36": {"svk": -793.0, "neo_hookean": -748.0, "negative": 2}}


@functools.lru_cache(maxsize=None)
def problem(name):
    """``(points, cells, dirichlet_dofs, Tangent in float64)``."""
    pts, cells, dd = fd.mesh(name)
    return pts, cells, dd, td.Tangent(pts, cells, LMD, MU, dd, T=np.float64)


@functools.lru_cache(maxsize=None)
def mass_matrix(name):
    """The dense consistent mass of the handle, Dirichlet rows and columns 0.  Order 1: ``rho V/20 (1 + delta_ab) I_3`` per
    element; order 2: the 14-point rule of ``p2_double.assemble(..., mass_rule=4)``."""
    pts, cells, dd, fs = problem(name)
    n = 3 * len(pts)
    if cells.shape[1] == 10:
        return p2_double.assemble(pts, cells, dd, LMD, MU, fd.RHO, mass_rule=4)[1]
    p = pts[cells]
    vol = np.abs(np.linalg.det(p[:, 1:] - p[:, :1])) / 6.0
    Me = fd.RHO * vol[:, None, None] / 20.0 * (np.ones((4, 4)) + np.eye(4))[None]
    Me = np.einsum("eab,AB->eaAbB", Me, np.eye(3)).reshape(len(cells), 12, 12)
    dof = (3 * cells[:, :, None] + np.arange(3)[None, None, :]).reshape(len(cells), 12)
    M = np.zeros((n, n))
    np.add.at(M, (dof[:, :, None], dof[:, None, :]), Me)
    free = np.asarray(fs.free, dtype=np.float64)
    return M * free[:, None] * free[None, :]


def load(name, f):
    """The consistent body-force vector of the density ``f``, 0 on Dirichlet dofs."""
    fs = problem(name)[3]
    return np.where(fs.free, np.asarray(fs.ext.load(tuple(float(c) for c in f)), dtype=np.float64), 0.0)


@functools.lru_cache(maxsize=None)
def equilibrium(name, material, fx):
    """``(u*, relative residual)`` under ``(fx, 0, 0)``, ``tangent_double.newton`` in four load steps."""
    u, res, _ = td.newton(problem(name)[3], load(name, (fx, 0.0, 0.0)), material, load_steps=4)
    return u, res


def pair(name, material, u):
    """``(K_T(u), M, free dof indices)``, dense."""
    fs = problem(name)[3]
    K = fs.tangent_matrix(np.asarray(u, dtype=np.float64), material)
    return 0.5 * (K + K.T), mass_matrix(name), np.nonzero(fs.free)[0]


def eigenvalues(name, material, u):
    """All ``omega^2`` of ``K_T(u) x = omega^2 M x`` on the free dofs, ascending."""
    from scipy.linalg import eigh

    K, M, free = pair(name, material, u)
    return eigh(K[np.ix_(free, free)], M[np.ix_(free, free)], eigvals_only=True)


@functools.lru_cache(maxsize=None)
def unstressed(name):
    return eigenvalues(name, "svk", np.zeros(3 * len(problem(name)[0])))


@functools.lru_cache(maxsize=None)
def prestressed(name, material, fx):
    return eigenvalues(name, material, equilibrium(name, material, fx)[0])


@functools.lru_cache(maxsize=None)
def unstable(name, material):
    """``(u = 3 u*(fx = -2000), omega^2 ascending)``."""
    u = 3.0 * equilibrium(name, material, -2000.0)[0]
    return u, eigenvalues(name, material, u)
