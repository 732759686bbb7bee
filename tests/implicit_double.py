"""NumPy double of the implicit stepper of ``csrc/saa_opimp.hip``: Newmark with ``beta = 1/4``, ``gamma = 1/2`` (the trapezoidal
rule) in float64 with the dense tangent and a direct solve.  Shared by tests/test_implicit.py (CPU) and
tests/test_gpu_implicit.py.  Lives under tests/: the product never imports it; it is not a test.

Built only on the existing doubles: :class:`tangent_double.Tangent` (``f_int``, the dense ``K_T``), the meshes and materials of
tests/finite_strain_double.py, ``p2_dynamics_double.hrz_mass``.  With the diagonal mass ``m``, the un-ramped load ``f``, ``scale(t)
= min(t, 1)`` if ``ramp`` else 1 and ``live`` the free dofs at nodes with elements (``d = v = a = 0`` elsewhere):

    m a + alpha m v + f_int(d) = scale(t) f
    d1 = x,   v1 = 2/dt (x - d) - v,   a1 = 4/dt^2 (x - d - dt v) - a
    r(x) = scale(t + dt) f - f_int(x) - m (a1 + alpha v1),   J(x) = K_T(x) + diag(s),   s = (4/dt^2 + 2 alpha/dt) m

Per step the predictor ``x = d + dt v`` and full Newton steps ``x += J^-1 r`` (``np.linalg.solve`` on the live dofs) until ``|r| <=
tol max(|scale f|, |f_int(x)|, |m (a1 + alpha v1)|)``, 2-norms over the live dofs.  A step is not accepted when ``max_newton``
iterations did not converge it (reason 1), a residual is not finite (2) or neo-Hooke finds an inverted element at a trial ``x``
(3); the state then stays that of the last accepted step.  The linear material makes one solve per step and takes its result:
the kernel's one PCG runs to ``tol`` on the recurrence residual, and a residual evaluated afresh has a round-off floor of its own
(``eps`` times the cancellation inside ``f_int``, about 3e-12 of the scale for the lowest mode of these beams)."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import p2_dynamics_double as pdd
import tangent_double as td

LMD, MU = fd.lame(fd.E, fd.NU)


def lumped_mass(points, cells, rho):
    """``(3 n,)``: order 1 the row sum ``rho |V| / 4``, order 2 ``p2_dynamics_double.hrz_mass``."""
    cells = np.asarray(cells, dtype=np.int64)
    if cells.shape[1] == 10:
        return np.asarray(pdd.hrz_mass(points, cells, rho), dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)[cells]
    vol = np.abs(np.linalg.det(p[:, 1:] - p[:, :1])) / 6.0
    node = np.bincount(cells.ravel(), weights=np.repeat(rho * vol / 4.0, 4), minlength=len(points))
    return np.repeat(node, 3)


class Problem:
    """A clamped mesh of tests/finite_strain_double.py in float64: ``fs`` (a :class:`tangent_double.Tangent`), ``mass``, ``live``,
    the linear ``K`` (dense, Dirichlet rows and columns 0) and the eigenpairs of ``M_L^-1 K`` on the live dofs."""

    def __init__(self, name):
        self.name = name
        self.pts, self.cells, self.dd = fd.mesh(name)
        self.n = 3 * len(self.pts)
        self.fs = td.Tangent(self.pts, self.cells, LMD, MU, self.dd, T=np.float64)
        self.mass = lumped_mass(self.pts, self.cells, fd.RHO)
        self.live = self.fs.free.copy()
        self.live[np.repeat(np.bincount(self.cells.ravel(), minlength=len(self.pts)) == 0, 3)] = False
        self.idx = np.nonzero(self.live)[0]
        self.K = self.fs.tangent_matrix(np.zeros(self.n), "svk")          # = the handle's K
        s = 1.0 / np.sqrt(self.mass[self.idx])
        w2, y = np.linalg.eigh(self.K[np.ix_(self.idx, self.idx)] * s[:, None] * s[None, :])
        self.omega = np.sqrt(w2)                                       # ascending
        self._y, self._s = y, s
        self.dt_crit = 2.0 / float(self.omega[-1])

    def mode(self, j):
        """``phi_j (3 n,)`` of ``M_L^-1 K`` (``K phi = omega_j^2 m phi``), scaled to ``max|phi| = 1``."""
        phi = np.zeros(self.n)
        phi[self.idx] = self._s * self._y[:, j]
        return phi / np.abs(phi).max()

    def load(self, fz):
        """The consistent body force ``(0, -fz, -fz)`` of the drivers, masked."""
        return np.where(self.fs.free, np.asarray(self.fs.ext.load((0.0, -fz, -fz)), dtype=np.float64), 0.0)


@functools.lru_cache(maxsize=None)
def problem(name):
    return Problem(name)


class Newmark:
    """The stepper on a :class:`Problem`.  ``material``: ``linear``, ``svk``, ``neo_hookean``."""

    def __init__(self, prob, mass, load, dt, alpha, ramp=True, material="linear", tol=1e-10, max_newton=25, at_floor=False):
        self.p, self.material = prob, material
        # at_floor (reference runs only): a step is also accepted once Newton has stopped halving the residual below 100 tol
        # - float64 resolves no better there (``delaunay2``: it stays at 2.1e-13 .. 2.2e-13 of the scale for ever)
        self.at_floor = bool(at_floor)
        self.mass, self.load = np.asarray(mass, dtype=np.float64), np.asarray(load, dtype=np.float64)
        self.dt, self.alpha, self.ramp, self.tol, self.max_newton = float(dt), float(alpha), bool(ramp), float(tol), int(max_newton)
        n = prob.n
        self.d, self.v, self.a, self.t = np.zeros(n), np.zeros(n), np.zeros(n), 0.0
        self.steps_done = 0
        self.newton_per_step = []
        self.watch = None                                              # watch(x): called with every accepted state

    def scale(self, t):
        return min(t, 1.0) if self.ramp else 1.0

    def force(self, x):
        """``(f_int(x), inverted?)``."""
        if self.material == "linear":
            return self.p.K @ x, False
        f, _, inv = self.p.fs.evaluate(x, self.material)
        return np.asarray(f, dtype=np.float64), bool(inv.any())

    def tangent(self, x):
        return self.p.K if self.material == "linear" else self.p.fs.tangent_matrix(x, self.material)

    def set_state(self, d=None, v=None, t=0.0):
        live = self.p.live
        self.d = np.where(live, np.zeros(self.p.n) if d is None else np.asarray(d, dtype=np.float64), 0.0)
        self.v = np.where(live, np.zeros(self.p.n) if v is None else np.asarray(v, dtype=np.float64), 0.0)
        self.t = float(t)
        f = self.force(self.d)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.a = np.where(live, (self.scale(self.t) * self.load - f - self.alpha * self.mass * self.v) / self.mass, 0.0)

    def rates(self, x):
        dt = self.dt
        v1 = 2.0 / dt * (x - self.d) - self.v
        a1 = 4.0 / (dt * dt) * (x - self.d - dt * self.v) - self.a
        return v1, a1

    def residual(self, x, scale):
        """``(r, |r|, reference scale, inverted?)`` at the trial ``x``."""
        live = self.p.live
        f, inv = self.force(x)
        v1, a1 = self.rates(x)
        ext, ine = scale * self.load, self.mass * (a1 + self.alpha * v1)
        r = np.where(live, ext - f - ine, 0.0)
        ref = max(np.linalg.norm(ext[live]), np.linalg.norm(f[live]), np.linalg.norm(ine[live]))
        return r, float(np.linalg.norm(r)), float(ref), inv

    def step(self, n=1):
        """``info`` with the keys of ``dynamics.ImplicitStepper.step`` (``cg_iterations`` 0: the solves are direct)."""
        info = {"steps_done": 0, "converged": True, "reason": 0, "newton_iterations": 0, "cg_iterations": 0, "residual": 0.0}
        idx, dt = self.p.idx, self.dt
        s = (4.0 / (dt * dt) + 2.0 * self.alpha / dt) * self.mass
        for _ in range(int(n)):
            scale = self.scale(self.t + dt)
            x = np.where(self.p.live, self.d + dt * self.v, 0.0)
            reason, its, last = 0, 0, np.inf
            while True:
                r, rn, ref, inv = self.residual(x, scale)
                if inv:
                    reason = 3
                    break
                if not np.isfinite(rn):
                    reason = 2
                    break
                info["residual"] = rn / ref if ref > 0 else rn
                if rn <= self.tol * ref or (self.at_floor and rn > 0.5 * last and rn <= 100.0 * self.tol * ref):
                    break
                last = rn
                if its >= self.max_newton:
                    reason = 1
                    break
                J = self.tangent(x)[np.ix_(idx, idx)]
                J[np.diag_indices_from(J)] += s[idx]
                x = x.copy()
                x[idx] += np.linalg.solve(J, r[idx])
                its += 1
                info["newton_iterations"] += 1
                if self.material == "linear":                          # the one system, solved: no second look
                    if not np.isfinite(x).all():
                        reason = 2
                    break
            if reason:
                info["converged"], info["reason"] = False, reason
                break
            v1, a1 = self.rates(x)
            self.d, self.v, self.a = x, np.where(self.p.live, v1, 0.0), np.where(self.p.live, a1, 0.0)
            self.t += dt
            self.steps_done += 1
            info["steps_done"] += 1
            self.newton_per_step.append(its)
            if self.watch is not None:
                self.watch(self.d)
        return info

    def energy(self):
        """Linear material: ``T + U - f . d`` at the current state."""
        return 0.5 * float(self.mass @ (self.v * self.v)) + 0.5 * float(self.d @ (self.p.K @ self.d)) - float(self.load @ self.d)


# ---- the cases of the tests -------------------------------------------------------------------------------------------------

MODAL_MESHES = ("structured288", "beam36")
MODAL_STEPS = 40
NONLINEAR_STEPS = 12


def modal_cases(prob):
    """``(j, dt / dt_crit)``: the lowest, a middle and the highest mode."""
    return [(0, 50.0), (len(prob.omega) // 2, 5.0), (len(prob.omega) - 1, 3.0)]


def modal_exact(prob, j, dt, n):
    """``d`` after ``n`` undamped, unloaded trapezoidal steps from ``d = phi_j``, ``v = 0``: ``phi_j cos(n theta)``, ``theta = 2 atan(omega_j
    dt / 2)``."""
    return prob.mode(j) * np.cos(n * 2.0 * np.arctan(0.5 * prob.omega[j] * dt))


def modal_kappa(prob, dt):
    """The condition number of ``J = K + 4/dt^2 M_L`` in the mass norm: ``(1 + (omega_max dt/2)^2) / (1 + (omega_1 dt/2)^2)``."""
    return (1.0 + (0.5 * prob.omega[-1] * dt) ** 2) / (1.0 + (0.5 * prob.omega[0] * dt) ** 2)


def nonlinear_start(prob):
    return fd.bend(prob.pts, 0.5, prob.dd)


def nonlinear_run(prob, material, tol, steps=NONLINEAR_STEPS, watch=None, record=None, at_floor=False):
    """The nonlinear case: from ``fd.bend(points, 0.5, dd)`` at rest, load ``fz = 200`` un-ramped, ``alpha = 0.5``, ``dt = 5 dt_crit``.
    Returns the stepper after ``steps`` steps; ``record``: a list that receives ``(d, v, a)`` of every accepted state, the start
    included."""
    nm = Newmark(prob, prob.mass, prob.load(200.0), 5.0 * prob.dt_crit, 0.5, ramp=False, material=material, tol=tol,
                 at_floor=at_floor)
    nm.set_state(nonlinear_start(prob))
    nm.watch = watch
    if record is not None:
        record.append((nm.d.copy(), nm.v.copy(), nm.a.copy()))
    for _ in range(steps):
        info = nm.step(1)
        assert info["converged"], (prob.name, material, tol, info)
        if record is not None:
            record.append((nm.d.copy(), nm.v.copy(), nm.a.copy()))
    return nm


@functools.lru_cache(maxsize=None)
def nonlinear_reference(name, material):
    """``d`` after the 12 steps at ``tol = 1e-13`` - or at the round-off floor of the residual where that lies above (``at_floor``) -,
    computed once per process."""
    return nonlinear_run(problem(name), material, 1e-13, at_floor=True).d.copy()


SECOND_ORDER_END, SECOND_ORDER_FACTORS = 0.05, (1, 2, 4, 8)


def second_order_case(prob):
    """``(load, dt_explicit, n_explicit)``: ramped ``fz = 0.5``, ``alpha = 0.5``, end time 0.05, the explicit step the largest at most
    ``0.9 dt_crit`` that divides the end time into a multiple of 8 steps."""
    n = 8 * int(np.ceil(SECOND_ORDER_END / (0.9 * prob.dt_crit) / 8.0))
    return prob.load(0.5), SECOND_ORDER_END / n, n


def explicit_run(prob, load, dt, n):
    """``fd.run`` with the linear force from rest: ``d`` at ``t = n dt``.  (``fd.run`` returns ``d0`` at ``tn``.)"""
    return fd.run(lambda x: prob.K @ x, prob.mass, load, prob.live, dt, 0.5, True, n)[0]
