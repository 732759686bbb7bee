"""NumPy double of ``csrc/saa_opdt.hip``: the per-element bound of ``omega_max(M_L^-1 K_T(u))``, the exact change of ``dt`` and the
variable-step central-difference scheme it continues.  Shared by tests/test_dt_follow.py (CPU) and tests/test_gpu_dt_follow.py.
Lives under tests/: the product never imports it; it is not a test.

Built on :class:`tangent_double.Tangent` (its ``gradient``, ``dstress`` and dense ``tangent_matrix``) in the same arithmetics.  At
each point ``q`` of the K rule, with ``g_a = grad_X N_a(q)`` and ``m_a`` the element's share of the lumped mass (order 1: ``rho
|V_e| / 4``; order 2: ``p2_dynamics_double.hrz_element_masses``):

    C_q = sum_a g_a g_a^T / m_a = R R^T,   T_q = (I_3 (x) R)^T A_q (I_3 (x) R),   A_q = dP/dF at H = grad_X u,
    mu_q = w_q |detJ_q| max(lambda_max(T_q), 0),   omega_e = sqrt(sum_q mu_q).

``A_q`` is dense here: column ``(j, l)`` of ``T_q`` is ``Tangent.dstress`` of the direction ``dH[j][k] = R[k][l]``, rows ``sum_k
dP[i][k] R[k][k']``, and ``lambda_max`` is ``numpy.linalg.eigvalsh`` of the float64 matrix.  ``linear`` is ``svk`` at ``H = 0``.

:func:`set_dt` is the change of step as the header states it; :func:`run_variable` is the VELOCITY form of the variable-step
scheme, which never forms the replaced ``dn``:

    m (v+ - v-)/h + alpha m (v+ + v-)/2 + s = scale f,   h = (dt_prev + dt)/2,   d1 = d0 + dt v+ ."""
from __future__ import annotations

import numpy as np

import finite_strain_double as fd
import p2_dynamics_double as pd
import tangent_double as td
from operator_extended import conv, scalar, sqrt, zeros

N_DRAWS = 8
STATES = ("zero", "strain", "bend")


class Bound(td.Tangent):
    """``omega_e(u)`` next to ``K_T(u)`` of :class:`tangent_double.Tangent`, with the density ``rho``."""

    def __init__(self, points, cells, lmd, mu, rho, dirichlet_dofs=(), T=np.longdouble):
        super().__init__(points, cells, lmd, mu, dirichlet_dofs, T=T)
        self.rho = scalar(rho, T)
        self.points64 = np.asarray(points, dtype=np.float64)

    def element_masses(self):
        """``(ne, na)``: the element's shares of the lumped mass."""
        if self.na == 4:
            vol = np.abs(self.ext.wdk[:, 0])                           # |detJ| / 6
            return (self.rho * vol / 4)[:, None] + zeros((self.n_elems, 4), self.T)
        return conv(pd.hrz_element_masses(self.points64, self.cells, float(self.rho)), self.T)

    def lumped_mass(self):
        """``(3 n,)`` float64: the shares summed per node, one value on a node's three dofs."""
        m = np.asarray(self.element_masses(), dtype=np.float64)
        return np.repeat(np.bincount(self.cells.ravel(), weights=m.ravel(), minlength=self.n_nodes), 3)

    def point_matrices(self, u, material):
        """``(T (ne, nq, 9, 9), inverted (ne,) bool)`` in the arithmetic of the class."""
        T = self.T
        law = "svk" if material == "linear" else material
        H = zeros((self.n_elems, self.nq, 3, 3), T) if material == "linear" else self.gradient(u)
        g, m = self.ext.grad, self.element_masses()
        Cq = zeros((self.n_elems, self.nq, 3, 3), T)
        for a in range(self.na):
            for i in range(3):
                for k in range(3):
                    Cq[..., i, k] = Cq[..., i, k] + g[:, :, a, i] * g[:, :, a, k] / m[:, a, None]
        R = zeros(Cq.shape, T)                                         # lower triangular, C = R R^T
        with np.errstate(invalid="ignore", divide="ignore"):
            R[..., 0, 0] = sqrt(Cq[..., 0, 0], T)
            R[..., 1, 0] = Cq[..., 0, 1] / R[..., 0, 0]
            R[..., 2, 0] = Cq[..., 0, 2] / R[..., 0, 0]
            R[..., 1, 1] = sqrt(Cq[..., 1, 1] - R[..., 1, 0] * R[..., 1, 0], T)
            R[..., 2, 1] = (Cq[..., 1, 2] - R[..., 2, 0] * R[..., 1, 0]) / R[..., 1, 1]
            R[..., 2, 2] = sqrt(Cq[..., 2, 2] - R[..., 2, 0] * R[..., 2, 0] - R[..., 2, 1] * R[..., 2, 1], T)
            out = zeros((self.n_elems, self.nq, 9, 9), T)
            inverted = np.zeros(self.n_elems, dtype=bool)
            for j in range(3):
                for l in range(3):
                    dH = zeros(H.shape, T)
                    for k in range(3):
                        dH[..., j, k] = R[..., k, l]
                    dP, inverted = self.dstress(H, dH, law)
                    for i in range(3):
                        for k2 in range(3):
                            for k in range(3):
                                out[..., 3 * i + k2, 3 * j + l] = out[..., 3 * i + k2, 3 * j + l] + dP[..., i, k] * R[..., k, k2]
        return out, inverted

    def omega_e(self, u, material):
        """``{"omega_e" (ne,) float64, "inverted" (ne,) bool, "n_nonpositive"}``: an inverted element (neo-Hooke, ``!(J > 0)`` at
        a point) has ``omega_e = 0``; a point whose matrix is not finite makes ``omega_e`` NaN."""
        Tq, inverted = self.point_matrices(u, material)
        A = np.asarray(Tq, dtype=np.float64)
        A = 0.5 * (A + np.swapaxes(A, -1, -2))
        finite = np.isfinite(A).all(axis=(-1, -2))
        lam = np.linalg.eigvalsh(np.where(finite[..., None, None], A, 0.0))[..., -1]
        lam = np.where(finite, np.maximum(lam, 0.0), np.nan)
        wd = np.abs(np.asarray(self.ext.wdk, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            om = np.sqrt((wd * lam).sum(axis=1))
        om = np.where(inverted, 0.0, om)
        return {"omega_e": om, "inverted": inverted, "n_nonpositive": int((np.asarray(self.ext.wdk) <= 0).any(axis=1).sum())}

    def bound(self, u, material):
        """What ``saa_operator_tangent_bound`` returns: ``omega_max`` over the elements that are neither inverted nor
        non-finite, its lowest ``element`` (0 and -1 when there is none) and the three counts."""
        r = self.omega_e(u, material)
        om, inv = r["omega_e"], r["inverted"]
        ok = ~inv & np.isfinite(om)
        top = float(om[ok].max()) if ok.any() else 0.0
        arg = int(np.nonzero(ok & (om == top))[0][0]) if ok.any() else -1
        return {"omega_max": top, "element": arg, "n_nonpositive": r["n_nonpositive"], "n_inverted": int(inv.sum()),
                "n_nonfinite": int((~inv & ~np.isfinite(om)).sum()), "omega_e": om}

    def omega_dense(self, u, material):
        """``omega_max`` of ``M_L^-1 K_T(u)`` on the free dofs, dense ``eigvalsh`` in float64."""
        law = "svk" if material == "linear" else material
        K = self.tangent_matrix(np.zeros(3 * self.n_nodes) if material == "linear" else u, law)
        free = self.free
        s = 1.0 / np.sqrt(self.lumped_mass()[free])
        w2 = np.linalg.eigvalsh(K[np.ix_(free, free)] * s[:, None] * s[None, :])
        return float(np.sqrt(w2[-1]))


def problem(name, T=np.float64):
    """``(points, cells, dd, Bound)`` of a mesh of ``finite_strain_double.MESHES`` with its material and ``rho``."""
    pts, cells, dd = fd.mesh(name)
    lmd, mu = fd.lame(fd.E, fd.NU)
    return pts, cells, dd, Bound(pts, cells, lmd, mu, fd.RHO, dd, T=T)


def state(name, pts, fs):
    """The three states of the tests: ``zero``, ``strain`` (``smooth_random_field`` seed 1 at ``max|H| = 0.3``) and ``bend`` (the
    finite bend with the tip rotated by 1 rad), masked on the Dirichlet dofs."""
    if name == "zero":
        return np.zeros(3 * len(pts))
    if name == "strain":
        return np.where(fs.free, fd.scale_to_strain(fs, fd.smooth_random_field(pts, 1), 0.3)[0], 0.0)
    if name == "bend":
        return fd.bend(pts, 1.0, np.nonzero(~fs.free)[0])
    raise ValueError(name)


def envelope(pts, cells, dd, u, material, ref):
    """The largest relative change of ``omega_e`` (max-norm over the elements, against ``max|ref|``) over ``N_DRAWS`` draws that
    perturb the points, ``lambda``, ``mu``, ``rho`` and ``u`` by ``+-2^-53`` (seed 77), in longdouble."""
    rng = np.random.default_rng(77)
    lmd, mu = fd.lame(fd.E, fd.NU)
    eps = np.longdouble(2.0) ** -53

    def jitter(a):
        a = np.asarray(a, dtype=np.longdouble)
        return a * (1 + np.asarray(rng.uniform(-1.0, 1.0, size=a.shape), dtype=np.longdouble) * eps)

    env = 0.0
    for _ in range(N_DRAWS):
        fs = Bound(jitter(pts), cells, jitter(lmd), jitter(mu), jitter(fd.RHO), dd)
        alt = fs.omega_e(jitter(u), material)["omega_e"]
        env = max(env, float(np.abs(alt - ref).max() / np.abs(ref).max()))
    return env


# ---- the change of step and the scheme it continues ---------------------------------------------------------------------

def set_dt(s, mass, load, live, d0, dn, dt_old, dt_new, alpha, scale):
    """``dn'`` of ``saa_operator_stepper_set_dt`` from ``s = f_int(d0)``: 0 where ``live`` is false."""
    with np.errstate(invalid="ignore", divide="ignore"):
        vm = (d0 - dn) / dt_old
        a = (scale * load - s) / mass
        rh = 2.0 / (dt_old + dt_new)
        vp = ((rh - 0.5 * alpha) * vm + a) / (rh + 0.5 * alpha)
        vq = ((1.0 / dt_new + 0.5 * alpha) * vp - a) / (1.0 / dt_new - 0.5 * alpha)
        return np.where(live, d0 - dt_new * vq, 0.0)


def run_variable(dts, force, mass, load, live, alpha, ramp, d0, dn, dt_prev, tn=0.0, record=None, T=np.float64):
    """One step per entry of ``dts`` of the variable-step scheme in velocity form, from ``d0`` with ``v- = (d0 - dn)/dt_prev``.
    Returns ``(d0, v, tn)``; ``record(step, d1)`` sees every step.  ``T = np.longdouble`` runs the same loop in extended
    precision (``force`` must then return that)."""
    mass, load = np.asarray(mass, dtype=T), np.asarray(load, dtype=T)
    d0, alpha = np.array(d0, dtype=T), T(alpha)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(live, (d0 - np.asarray(dn, dtype=T)) / T(dt_prev), T(0))
        for i, dt in enumerate(dts):
            dt = T(dt)
            scale = T(min(tn, 1.0) if ramp else 1.0)
            a = (scale * load - np.asarray(force(d0), dtype=T)) / mass
            rh = 2 / (T(dt_prev) + dt)
            v = np.where(live, ((rh - alpha / 2) * v + a) / (rh + alpha / 2), T(0))
            d0 = np.where(live, d0 + dt * v, T(0))
            if record is not None:
                record(i, d0)
            dt_prev = dt
            tn = tn + float(dt)
    return d0, v, tn


def per_step(changes, n_steps):
    """The ``dt`` of every step from the ``[(step, dt)]`` list of a followed run (``dt`` in use from ``step`` on)."""
    out = np.zeros(int(n_steps))
    for j, (step, dt) in enumerate(changes):
        out[int(step):] = dt
    return out


def follow_target(mode, gamma, omega, omega_l, omega_0):
    """The target of ``OperatorStepper.follow_time_step``."""
    if mode == "certified":
        return gamma * 2.0 / omega
    return gamma * (2.0 / omega_l) * min(1.0, omega_0 / omega)


def follow_move(dt, target, grow=1.05):
    """The ``dt`` after a check: a lower target at once, a higher one by at most ``grow``, inside the band nothing."""
    if target < dt:
        return target
    if target > grow * dt:
        return grow * dt
    return dt


def release_problem(name, material, strain=0.3):
    """The scenario of the tests: ``(fs, live, mass, load, u_s, dt, omega_l)`` - the mesh released at rest from the
    ``strain`` state, no load, ``dt = 0.9 * 2/omega_max`` of the linear operator (dense)."""
    pts, cells, dd, fs = problem(name)
    u = np.where(fs.free, fd.scale_to_strain(fs, fd.smooth_random_field(pts, 1), strain)[0], 0.0)
    mass = fs.lumped_mass()
    has = np.repeat(np.bincount(cells.ravel(), minlength=len(pts)) > 0, 3)
    omega_l = fs.omega_dense(None, "linear")
    return fs, fs.free & has, mass, np.zeros_like(mass), u, 0.9 * 2.0 / omega_l, omega_l


def followed_run(fs, material, live, mass, load, u, dt, omega_l, mode, n_steps=40, every=5, gamma=0.9, alpha=0.5, fixed=False):
    """The float64 run of the scenario: constant-step updates (``finite_strain_double.run``) with :func:`set_dt` at the checks,
    which are before step 0 and after every ``every`` steps.  Returns ``(d0, changes [(step, dt)], worst dt / dt_crit dense at a
    check, inverted element-steps, max|d| seen)``; ``fixed``: no check changes anything."""
    count = [0]

    def force(d):
        f, _, inv = fs.evaluate(d, material)
        count[0] += int(inv.sum())
        return np.asarray(f, dtype=np.float64)

    d0, dn, tn = u.copy(), u.copy(), 0.0
    omega_0 = fs.bound(None, "linear")["omega_max"]
    changes, worst, top = [], 0.0, float(np.abs(u).max())
    for done in range(0, n_steps, every):
        if not fixed:
            omega = fs.bound(d0, material)["omega_max"]
            new = follow_move(dt, follow_target(mode, gamma, omega, omega_l, omega_0))
            if new != dt:
                dn = set_dt(force(d0), mass, load, live, d0, dn, dt, new, alpha, 1.0)
                dt = new
            if not changes or changes[-1][1] != dt:
                changes.append((done, dt))
            worst = max(worst, dt * fs.omega_dense(d0, material) / 2.0)
        for _ in range(min(every, n_steps - done)):
            d0, dn, tn = fd.run(force, mass, load, live, dt, alpha, False, 1, d0, dn, tn)
            top = max(top, float(np.abs(d0).max()))
            if not np.isfinite(top) or top > 1e6:
                return d0, changes, worst, count[0], top
    return d0, changes, worst, count[0], top
