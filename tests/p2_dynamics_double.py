"""NumPy statement of the explicit dynamics on the operator handle (``csrc/saa_opstep.hip``): the HRZ and row-sum lumped
masses of the quadratic tetrahedron from the 14-point rule of tests/p2_double.py, the sharp stability limit from a dense
``eigh``, and the damped central-difference step of ``Tools/Dynamic_solver.py:12-20`` on a dense ``K`` from
``p2_double.assemble``."""
from __future__ import annotations

import numpy as np

import p2_double as p2


def _nodal(cells10, per_corner, n_nodes):
    node = np.bincount(np.asarray(cells10).ravel(), weights=per_corner.ravel(), minlength=n_nodes)
    return np.repeat(node, 3)


def hrz_element_masses(points, cells10, rho):
    """``(ne, 10)``: ``m_a = rho (sum_q w detJ) I_a / sum_b I_b``, ``I_a = sum_q w detJ N_a^2`` (14-point rule)."""
    wd, _, N = p2.geometry(points, cells10, 4)
    I = np.einsum("eq,qa->ea", wd, N ** 2)
    return rho * wd.sum(axis=1)[:, None] * I / I.sum(axis=1, keepdims=True)


def hrz_mass(points, cells10, rho):
    """The HRZ lumped mass ``(3 n,)``, one value on a node's three dofs, no Dirichlet mask."""
    return _nodal(cells10, hrz_element_masses(points, cells10, rho), len(points))


def row_sum_element_masses(points, cells10, rho):
    """``(ne, 10)``: the reference's lumping (``commons.py:103-107``), ``sum_b M_ab = rho integral N_a`` (14-point rule)."""
    wd, _, N = p2.geometry(points, cells10, 4)
    return rho * np.einsum("eq,qa->ea", wd, N)


def omega_extremes(K, mass, dirichlet):
    """``(omega_min, omega_max)`` of ``M_L^-1 K`` on the free dofs: dense ``eigh`` of ``M_L^-1/2 K M_L^-1/2``."""
    free = np.ones(len(mass), dtype=bool)
    free[np.asarray(dirichlet, dtype=np.int64)] = False
    s = 1.0 / np.sqrt(mass[free])
    w2 = np.linalg.eigvalsh(K[np.ix_(free, free)] * s[:, None] * s[None, :])
    return float(np.sqrt(w2[0])), float(np.sqrt(w2[-1]))


def run(K, mass, f, dirichlet, dt, alpha, ramp, nsteps, d0=None, dn=None, tn=0.0, record=None):
    """``nsteps`` steps of

        f_int = K d0,  f_ext = f * (min(tn, 1) if ramp else 1)
        d1 = (dt^2 (f_ext - f_int) + 2 m d0 - m dn + dt/2 m alpha dn) / (m + alpha m dt / 2),  d1[Dirichlet] = 0,  tn += dt

    (``K`` with Dirichlet rows and columns zero).  Returns ``(d0, dn, tn)``; ``record(step, d1)`` sees every step."""
    n = len(mass)
    d0 = np.zeros(n) if d0 is None else np.array(d0, dtype=np.float64)
    dn = np.zeros(n) if dn is None else np.array(dn, dtype=np.float64)
    dd = np.asarray(dirichlet, dtype=np.int64)
    den = mass + alpha * mass * dt / 2.0
    for i in range(nsteps):
        f_ext = f * (min(tn, 1.0) if ramp else 1.0)
        d1 = (dt * dt * (f_ext - K @ d0) + 2.0 * mass * d0 - mass * dn + dt / 2.0 * mass * alpha * dn) / den
        d1[dd] = 0.0
        if record is not None:
            record(i, d1)
        dn, d0 = d0, d1
        tn += dt
    return d0, dn, tn
