"""Helpers of the edge tests of the implicit stepper of ``csrc/saa_opimp.hip``: a float64 double that ITERATES as the kernel does
(:class:`NewmarkPCG`), meshes padded with element-less nodes up to the launch and fold thresholds of the kernels
(:func:`padded`), a model of the kernels' two-level sums with the mutants the tests must catch (:func:`kernel_sum`), and the
scaled and off-the-unit-beam problems.  Shared by tests/test_implicit_edges.py (CPU, which qualifies every case and bar on
these references alone) and tests/test_gpu_implicit_edges.py.  Lives under tests/: the product never imports it; it is not a
test.

Thresholds, read from ``imp_blocks``, ``imp_fold`` and the launch sites: a pass over ``n`` items (dofs, or nodes) runs ``min(ceil(n
/ 256), 2048)`` workgroups of 256 lanes; item ``i`` belongs to workgroup ``(i // 256) % 2048``; the fold's lane ``t`` adds the
partials ``t, t + 256, ...``.  So a second partial per lane appears at ``n = 65537`` items and a second trip of the grid-stride
loop at ``n = 524289``: in nodes ``N = 21845 | 21846`` and ``174762 | 174763`` for the dof-wise passes (``3 N`` items), ``65536 |
65537`` and ``524288 | 524289`` for the node passes."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import implicit_double as imp
import operator_extended as ox
import tangent_double as td

THREADS, MAX_BLOCKS = 256, 2048
PADDED_NODES = (21845, 21846, 65536, 65537, 174762, 174763, 524288, 524289)
LARGE_NODES = PADDED_NODES[4:]                                         # the two largest pairs: once per material
EDGE_MESHES = ("structured288", "curved288")                           # order 1, order 2
EPS = float(np.finfo(np.float64).eps)


# ---- problems off the unit beam ---------------------------------------------------------------------------------------------

class EdgeProblem(imp.Problem):
    """:class:`implicit_double.Problem` of any mesh and material constants (the base class builds those of
    ``finite_strain_double.mesh`` at ``E = 1e6``, ``nu = 0.3`` only)."""

    def __init__(self, name, pts, cells, dd, lmd, mu, rho, spectrum=True):
        self.name = name
        self.pts, self.cells, self.dd = np.asarray(pts, dtype=np.float64), np.asarray(cells, dtype=np.int64), np.asarray(dd, dtype=np.int64)
        self.lmd, self.mu, self.rho = float(lmd), float(mu), float(rho)
        self.n = 3 * len(self.pts)
        self.fs = td.Tangent(self.pts, self.cells, lmd, mu, self.dd, T=np.float64)
        self.mass = imp.lumped_mass(self.pts, self.cells, rho)
        self.live = self.fs.free.copy()
        self.live[np.repeat(np.bincount(self.cells.ravel(), minlength=len(self.pts)) == 0, 3)] = False
        self.idx = np.nonzero(self.live)[0]
        self.K = self.fs.tangent_matrix(np.zeros(self.n), "svk")
        if spectrum:
            s = 1.0 / np.sqrt(self.mass[self.idx])
            w2, y = np.linalg.eigh(self.K[np.ix_(self.idx, self.idx)] * s[:, None] * s[None, :])
            self.omega, self._y, self._s = np.sqrt(np.maximum(w2, 0.0)), y, s
            self.dt_crit = 2.0 / float(self.omega[-1])


OFF_BEAM = ("nu-0.499999", "sliver-1e-06")


@functools.lru_cache(maxsize=None)
def off_beam_problem(name, family):
    """``nu = 0.499999`` (the highest of ``operator_extended.NUS``) or every fifth element a sliver of ``V / h^3 = 1e-6``
    (``operator_extended.make_slivers``) on a mesh of ``finite_strain_double.mesh``."""
    pts, cells, dd = fd.mesh(name)
    lmd, mu = imp.LMD, imp.MU
    if family == "nu-0.499999":
        lmd, mu = fd.lame(fd.E, 0.499999)
    elif family == "sliver-1e-06":
        pts, cells = ox.make_slivers(pts, cells, 1e-6)                 # new nodes are appended: dd keeps its numbers
    else:
        raise ValueError(family)
    return EdgeProblem(f"{name}-{family}", pts, cells, dd, lmd, mu, fd.RHO)


# Power-of-two units with time.  operator_extended.scaled_case: lengths 2^(40 u), moduli 2^(20 u), density 2^(20 u).  The wave
# speed sqrt(modulus / density) is unchanged, so a time is a length over it: dt, t and 1 / alpha pick up 2^(40 u).  Then
#   d: a length                              40          v = d / t:                    0
#   a = d / t^2:                            -40          mass = density length^3:      20 + 120 = 140
#   load = m a = K d (K: kx / x = 20 + 40): 100          4 / dt^2:                    -80,  shift = 4 m / dt^2: 60
#   |r|^2, |f|^2:                           200          tol, eta, all counts:         0
UNIT_EXPONENT = {"d": 40, "v": 0, "a": -40, "mass": 140, "load": 100, "dt": 40, "alpha": -40, "points": 40, "modulus": 20,
                 "density": 20}


@functools.lru_cache(maxsize=None)
def scaled_problem(name, u):
    """The mesh ``name`` in the units ``u`` of ``operator_extended.UNITS`` (exponents: ``UNIT_EXPONENT`` times ``u``: ``d`` 40, ``v`` 0,
    ``a`` -40, ``mass`` 140, ``load`` 100, ``dt`` and ``1 / alpha`` 40).  No spectrum: ``dt`` is the unscaled one times ``2^(40 u)``."""
    pts, cells, dd = fd.mesh(name)
    return EdgeProblem(f"{name}-units{u:+d}", pts * 2.0 ** (40 * u), cells, dd, imp.LMD * 2.0 ** (20 * u), imp.MU * 2.0 ** (20 * u),
                       fd.RHO * 2.0 ** (20 * u), spectrum=False)


def unit(key, u):
    return 2.0 ** (UNIT_EXPONENT[key] * u)


# ---- the double that iterates as the kernel does ----------------------------------------------------------------------------

class NewmarkPCG(imp.Newmark):
    """``implicit_double.Newmark`` with the solves of ``opimp_step`` / ``pcg``: per Newton pass a Jacobi-PCG from 0 with ``1 / (diag
    K_linear + s)`` on ``J = K_T(x) + s`` (the dense ``K_T`` of ``tangent_double.Tangent`` is the matvec) until ``|r_cg| <= target`` -
    ``tol ref`` for the linear material, else ``eta |r|`` with ``eta = max(min(0.1, 0.9 (|r| / |r_prev|)^2), 0.1 goal / |r|)``, 0.1 on the
    first pass -, at most ``max_cg`` iterations (None: ``20 n_dof``), stopped with nothing updated when ``p . J p <= 0``; ``x += x_cg``, or
    ``+= minv r`` when no iteration was made.  The linear material takes the solve's result when the recurrence residual reached
    the target and is within ``tol`` of the scale at the solved ``x`` (the next residual pass gives it), else it makes another pass.
    ``newton_iterations`` and ``cg_iterations`` count what the kernel counts.

    ``order``: a ``numpy`` generator; every dot product and squared norm is then summed in a fresh random order.  ``trace``: a list
    that receives ``(p . J p, |p|, |J p|)`` of every PCG iteration begun.  ``seen``: ``[lo, hi]`` of the magnitudes of every nonzero
    intermediate, when a list is given.  ``late_clamp`` / ``keep_shift``: the two mutants of the time tests - the ramp clamped by the
    time before the step, the shift of the ``dt`` before ``set_dt``."""

    def __init__(self, prob, mass, load, dt, alpha, ramp=True, material="linear", tol=1e-10, max_newton=25, max_cg=None,
                 order=None, trace=None, seen=None, late_clamp=False, keep_shift=False):
        super().__init__(prob, mass, load, dt, alpha, ramp=ramp, material=material, tol=tol, max_newton=max_newton)
        self.max_cg = 20 * prob.n if max_cg is None else int(max_cg)
        self.order, self.trace, self.seen = order, trace, seen
        self.late_clamp, self.keep_shift = bool(late_clamp), bool(keep_shift)
        self.shift_dt = self.dt
        self.cg_per_solve = []
        self._k_live = prob.K[np.ix_(prob.idx, prob.idx)]
        self._diag = np.diag(prob.K)[prob.idx].copy()

    def set_dt(self, dt):
        self.dt = float(dt)
        if not self.keep_shift:
            self.shift_dt = self.dt

    def scale(self, t):
        if self.ramp and self.late_clamp:
            return t if t - self.dt < 1.0 else 1.0
        return super().scale(t)

    def _see(self, *arrays):
        if self.seen is None:
            return
        for a in arrays:
            m = np.abs(np.atleast_1d(np.asarray(a, dtype=np.float64)))
            m = m[m > 0]
            if m.size:
                self.seen[0], self.seen[1] = min(self.seen[0], float(m.min())), max(self.seen[1], float(m.max()))

    def dot(self, a, b):
        prod = a * b
        self._see(prod)
        out = float(a @ b) if self.order is None else float(np.sum(prod[self.order.permutation(len(prod))]))
        self._see(out)
        return out

    def residual(self, x, scale):
        live, i = self.p.live, self.p.idx
        f, inv = self.force(x)
        v1, a1 = self.rates(x)
        ext, ine = scale * self.load, self.mass * (a1 + self.alpha * v1)
        r = np.where(live, ext - f - ine, 0.0)
        self._see(x[i], v1[i], a1[i], ext[i], f[i], ine[i], r[i])
        with np.errstate(over="ignore", invalid="ignore"):
            rn = np.sqrt(self.dot(r[i], r[i]))
            ref = max(np.sqrt(self.dot(ext[i], ext[i])), np.sqrt(self.dot(f[i], f[i])), np.sqrt(self.dot(ine[i], ine[i])))
        return r, float(rn), float(ref), inv

    def pcg(self, x, r, minv, s, target):
        """``(dx, iterations, live, guard, |r_cg|)`` on the live dofs."""
        kt = self._k_live if self.material == "linear" else self.tangent(x)[np.ix_(self.p.idx, self.p.idx)]
        p = minv * r
        rz, xcg, iters, live, guard, norm = self.dot(r, p), np.zeros_like(r), 0, True, False, float(np.sqrt(r @ r))
        for _ in range(self.max_cg):
            ap = kt @ p + s * p
            pap = self.dot(p, ap)
            self._see(p, ap)
            if self.trace is not None:
                self.trace.append((pap, float(np.linalg.norm(p)), float(np.linalg.norm(ap))))
            if not pap > 0.0:
                live, guard = False, True
                break
            a = rz / pap
            xcg = xcg + a * p
            r = r - a * ap
            z = minv * r
            rz_new, rr = self.dot(r, z), self.dot(r, r)
            beta = rz_new / rz if rz > 0.0 else 0.0
            self._see(a, beta, xcg, r)
            p = z + beta * p
            rz, iters, norm = rz_new, iters + 1, float(np.sqrt(rr))
            if norm <= target:
                live = False
                break
        return (xcg if iters else p), iters, live, guard, norm

    def step(self, n=1):
        info = {"steps_done": 0, "converged": True, "reason": 0, "newton_iterations": 0, "cg_iterations": 0, "residual": 0.0}
        idx, dt = self.p.idx, self.dt
        c = 4.0 / (self.shift_dt * self.shift_dt) + 2.0 * self.alpha / self.shift_dt
        s = (c * self.mass)[idx]
        jd = self._diag + s
        self._see(c, 4.0 / (dt * dt), s, jd)
        minv = np.where(jd > 0.0, 1.0 / np.where(jd > 0.0, jd, 1.0), 1.0)
        linear = self.material == "linear"
        for _ in range(int(n)):
            scale = self.scale(self.t + dt)
            x = np.where(self.p.live, self.d + dt * self.v, 0.0)
            reason, its, previous, solved = 0, 0, -1.0, -1.0
            while True:
                r, rn, ref, inv = self.residual(x, scale)
                if inv:
                    reason = 3
                    break
                if not np.isfinite(rn):
                    reason = 2
                    break
                info["residual"] = rn / ref if ref > 0 else rn
                goal = self.tol * ref
                if rn <= goal:
                    break
                if 0.0 <= solved <= goal:                              # the recurrence residual over the scale at the solved x
                    info["residual"] = solved / ref if ref > 0 else solved
                    break
                if its >= self.max_newton:
                    reason = 1
                    break
                eta = 0.1 if previous < 0.0 else min(0.1, 0.9 * (rn / previous) * (rn / previous))
                eta = max(eta, 0.1 * goal / rn)
                target = goal if linear else eta * rn
                dx, iters, live, guard, norm = self.pcg(x, r[idx], minv, s, target)
                x = x.copy()
                x[idx] += dx
                previous, its = rn, its + 1
                info["newton_iterations"] += 1
                info["cg_iterations"] += iters
                self.cg_per_solve.append(iters)
                solved = norm if linear and not live and not guard and norm <= target else -1.0
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


def nonlinear_stepper(prob, material, cls=NewmarkPCG, amplitude=1.0, **kw):
    """The stepper of ``implicit_double.nonlinear_run`` at its start (times ``amplitude``), of class ``cls``."""
    kw.setdefault("tol", 1e-10)
    nm = cls(prob, prob.mass, prob.load(200.0), 5.0 * prob.dt_crit, 0.5, ramp=False, material=material, **kw)
    nm.set_state(amplitude * imp.nonlinear_start(prob))
    return nm


def run(nm, steps):
    """``steps`` calls of ``step(1)``: the totals, the Newton count of every step, the last ``info``."""
    total = {"newton_iterations": 0, "cg_iterations": 0, "steps_done": 0}
    info = None
    for _ in range(steps):
        info = nm.step(1)
        for k in total:
            total[k] += info[k]
        if not info["converged"]:
            break
    return total, list(nm.newton_per_step), info


EDGE_STEPS = 3


@functools.lru_cache(maxsize=None)
def reference3(name, material):
    """``d`` of the direct double after 3 steps of the nonlinear case at ``tol = 1e-13`` (or at the round-off floor)."""
    return imp.nonlinear_run(imp.problem(name), material, 1e-13, steps=EDGE_STEPS, at_floor=True).d.copy()


@functools.lru_cache(maxsize=None)
def mirror3(name, material):
    """``(d, totals, Newton per step)`` of :class:`NewmarkPCG` after the same 3 steps at the kernel's default ``tol = 1e-10``."""
    nm = nonlinear_stepper(imp.problem(name), material)
    total, per_step, info = run(nm, EDGE_STEPS)
    assert info["converged"], (name, material, info)
    return nm.d.copy(), total, per_step


# S: the largest relative spread of ``cg_iterations`` of :class:`NewmarkPCG` over 8 draws of random summation orders, measured
# by tests/test_implicit_edges.py::test_iteration_counts_under_random_summation_orders over the 3-step nonlinear cases and the
# modal cases (see its docstring for the figures); the GPU's total may differ from the double's by max(2 per solve, 2 S total).
S_SPREAD = 0.059


def count_bar(total):
    """The allowed difference of a call's ``cg_iterations`` from the double's ``total``."""
    return max(2 * total["newton_iterations"], 2.0 * S_SPREAD * total["cg_iterations"])


# ---- padding with element-less nodes ----------------------------------------------------------------------------------------

def n_blocks(n):
    return max(1, min(-(-int(n) // THREADS), MAX_BLOCKS))


def padded(prob, n_nodes, seed):
    """``(points, cells, dirichlet_dofs, node_map)``: the mesh of ``prob`` inside ``n_nodes`` points of which only its own have an
    element.  ``node_map`` is strictly increasing (every node keeps its ascending-element CSR order): a quarter of the mesh's
    nodes (at most 40) at random places among the first 85 points - the first workgroup of the dof-wise passes -, as many
    among the last 85 with the last point one of them, the others anywhere between.  :func:`places` is asserted to find
    live dofs wherever the passes of this size have a place of the kind."""
    rng = np.random.default_rng(seed)
    n_mesh, n_nodes = len(prob.pts), int(n_nodes)
    k = min(n_mesh // 4, 40)
    assert n_nodes >= n_mesh + 170
    head = rng.choice(85, size=k, replace=False)
    tail = n_nodes - 1 - np.concatenate([[0], 1 + rng.choice(84, size=k - 1, replace=False)])
    body = 85 + rng.choice(n_nodes - 170, size=n_mesh - 2 * k, replace=False)
    node_map = np.sort(np.concatenate([head, body, tail])).astype(np.int64)
    assert len(node_map) == n_mesh and (np.diff(node_map) > 0).all() and node_map[-1] == n_nodes - 1
    points = np.random.default_rng(seed + 1).uniform(prob.pts.min(axis=0), prob.pts.max(axis=0), size=(n_nodes, 3))
    points[node_map] = prob.pts
    dd = 3 * node_map[prob.dd // 3] + prob.dd % 3
    found = places(prob, node_map, n_nodes)
    for kind, want in found["wanted"].items():
        assert not want or found[kind], (prob.name, n_nodes, kind)
    return points, node_map[prob.cells], dd, node_map


def dof_map(node_map):
    return (3 * np.asarray(node_map)[:, None] + np.arange(3)[None, :]).ravel()


def places(prob, node_map, n_nodes):
    """Per pass kind (``dof``, ``node``): does a live dof sit in the first workgroup, in one with index >= 256, in the last one,
    and at an item index >= 2048 * 256, where the launch strides - and which of these exist at this size (``wanted``)."""
    live_dofs = dof_map(node_map)[prob.live]
    out = {"wanted": {}}
    for kind, items, n in (("dof", live_dofs, 3 * n_nodes), ("node", np.unique(live_dofs // 3), n_nodes)):
        last = (n - 1) // THREADS
        block = items // THREADS
        out[kind + "-first"] = bool((block == 0).any())
        out[kind + "-fold"] = bool(((block >= THREADS) & (block < MAX_BLOCKS)).any())
        out[kind + "-last"] = bool((block == last).any())
        out[kind + "-stride"] = bool((items >= MAX_BLOCKS * THREADS).any())
        out["wanted"].update({kind + "-first": True, kind + "-fold": last >= THREADS, kind + "-last": True,
                              kind + "-stride": n > MAX_BLOCKS * THREADS})
    return out


def scatter(vec, node_map, n_nodes, fill=0.0):
    out = np.full(3 * int(n_nodes), fill, dtype=np.float64)
    out[dof_map(node_map)] = vec
    return out


def kernel_sum(items, values, n, mutant=None):
    """The sum of ``values`` at the item indices ``items`` of a pass over ``n`` items as the kernels form it - one partial per
    workgroup ``(i // 256) % 2048``, then the fold - in float64.  ``mutant``: ``"fold"`` drops the partials at and above 256 (a fold
    whose lanes add one partial only), ``"tail"`` the items at and above ``2048 * 256`` (a stride loop that makes one trip)."""
    items, values = np.asarray(items, dtype=np.int64), np.asarray(values, dtype=np.float64)
    nb = n_blocks(n)
    if mutant == "tail":
        keep = items < MAX_BLOCKS * THREADS
        items, values = items[keep], values[keep]
    part = np.bincount((items // THREADS) % nb, weights=values, minlength=nb)
    if mutant == "fold":
        part = part[:THREADS]
    return float(part.sum())


@functools.lru_cache(maxsize=None)
def _long_fs(prob):
    return td.Tangent(prob.pts, prob.cells, getattr(prob, "lmd", imp.LMD), getattr(prob, "mu", imp.MU), prob.dd)


def true_residual(prob, material, mass, load, dt, alpha, scale, d0, v0, a0, d1, T=np.float64):
    """``|r| / ref`` of the trial ``d1`` after the state ``(d0, v0, a0)`` - what ``info["residual"]`` reports - evaluated afresh in the
    arithmetic ``T``: ``np.float64`` with the double's ``f_int``, ``np.longdouble`` with the longdouble ``f_int`` and sums."""
    d1 = np.asarray(d1, dtype=np.float64)
    if T is np.float64:
        f = imp.Newmark(prob, mass, load, dt, alpha, ramp=False, material=material).force(d1)[0]
    elif material == "linear":
        f = _long_fs(prob).tangent(np.zeros(prob.n), d1, "svk")
    else:
        f = _long_fs(prob).force(d1, material)
    f, d0, v0, a0, d1, m, ld = (np.asarray(x, dtype=T) for x in (f, d0, v0, a0, d1, mass, load))
    dt, alpha, scale = T(dt), T(alpha), T(scale)
    v1 = T(2) / dt * (d1 - d0) - v0
    a1 = T(4) / (dt * dt) * (d1 - d0 - dt * v0) - a0
    ext, ine = scale * ld, m * (a1 + alpha * v1)
    i = prob.idx
    r = (ext - f - ine)[i]
    norm = lambda x: np.sqrt((x * x).sum(dtype=T))
    return float(norm(r) / max(norm(ext[i]), norm(f[i]), norm(ine[i])))


# 10 x the largest relative difference between the float64 and the longdouble evaluation of the accepted residual of one
# step at tol = 1e-6, measured by tests/test_implicit_edges.py::test_residual_margin_and_the_fold_mutants (unit beam) and
# ::test_off_beam_cases_converge_and_their_residual_resolves; the figures are in their docstrings.
RESIDUAL_MARGIN = 1e-6
OFF_BEAM_MARGIN = 5e-5
OFF_BEAM_AMPLITUDE = 1.0

# max_cg: chosen by tests/test_implicit_edges.py::test_iteration_caps_give_both_outcomes
CAP_FAILS, CAP_CONVERGES, CAP_LINEAR = 3, 5, 20


# ---- the cases of the shifted apply, the guard, the time tests and the units ------------------------------------------------

def apply_vectors(prob):
    """``(u, v)`` of the padded shifted apply: the start of the nonlinear case and a smooth random direction, both masked."""
    return imp.nonlinear_start(prob), np.where(prob.fs.free, fd.smooth_random_field(prob.pts, 7), 0.0)


def apply_shift(prob, v):
    """A positive diagonal that makes ``s v`` comparable with ``K v``: ``(0.5 .. 1.5) max|K v| / max|v|``."""
    rng = np.random.default_rng(4242 + len(prob.pts))
    return rng.uniform(0.5, 1.5, size=prob.n) * float(np.abs(prob.K @ v).max() / np.abs(v).max())


@functools.lru_cache(maxsize=None)
def linear_direct3(name):
    p = imp.problem(name)
    nm = nonlinear_stepper(p, "linear", cls=imp.Newmark)
    nm.step(EDGE_STEPS)
    return nm.d.copy()


GUARD_COMPRESSION, GUARD_DT_FACTOR = 0.2, 100.0


@functools.lru_cache(maxsize=None)
def guard_case(name):
    """``(u, dt, k, trace, info)``: the uniform compression ``u_x = -0.2 x`` (masked) under ``svk`` with ``dt = 100 dt_crit``, ``fz = 200``, no
    damping, at rest - ``K_T(u) + s`` is indefinite - and what the mirrored double does there with ``max_newton = 1``: the PCG makes
    ``k`` iterations and stops in the next at ``p . J p <= 0``; ``trace`` has ``(p . J p, |p|, |J p|)`` of the ``k + 1`` iterations."""
    p = imp.problem(name)
    u = np.zeros((len(p.pts), 3))
    u[:, 0] = -GUARD_COMPRESSION * p.pts[:, 0]
    u = np.where(p.live, u.ravel(), 0.0)
    dt, trace = GUARD_DT_FACTOR * p.dt_crit, []
    nm = NewmarkPCG(p, p.mass, p.load(200.0), dt, 0.0, ramp=False, material="svk", max_newton=1, trace=trace)
    nm.set_state(u)
    info = nm.step(1)
    return u, dt, info["cg_iterations"], trace, info


TIME_DT, TIME_DT_NEW, TIME_AMPLITUDE, TIME_FZ = 5.0, 12.5, 0.05, {"ramp": 2000.0, "set_dt": 200.0}


def time_run(cls, prob, material, kind, **kw):
    """The two time cases, from 0.05 of the nonlinear case's start at rest, ``alpha = 0.5``, ``dt = 5 dt_crit``.  ``"ramp"``: ``ramp=True``, ``fz =
    2000``, from ``t = 1 - 1.5 dt``, 3 steps (at ``fz = 200`` from the full start the late clamp moves ``d`` by 1.2e-8 only on ``curved288``,
    next to the bar).  ``"set_dt"``: un-ramped, ``fz = 200``, 2 steps, then ``12.5 dt_crit``, 2 steps (from 0.2 of the start or more the
    direct double's Newton does not converge at ``12.5 dt_crit`` under ``svk``, or the two doubles end 0.5 of ``max|d|`` apart).  Returns the stepper,
    the ``info`` of its last step in ``last``; it stops at a step that is not accepted."""
    dt = TIME_DT * prob.dt_crit
    nm = cls(prob, prob.mass, prob.load(TIME_FZ[kind]), dt, 0.5, ramp=kind == "ramp", material=material, **kw)
    if kind == "ramp":
        nm.set_state(TIME_AMPLITUDE * imp.nonlinear_start(prob), None, 1.0 - 1.5 * dt)
        legs = (3,)
    else:
        nm.set_state(TIME_AMPLITUDE * imp.nonlinear_start(prob))
        legs = (2, 2)
    for k, n in enumerate(legs):
        if k:
            if hasattr(nm, "set_dt"):
                nm.set_dt(TIME_DT_NEW * prob.dt_crit)
            else:
                nm.dt = TIME_DT_NEW * prob.dt_crit
        for _ in range(n):
            nm.last = nm.step(1)
            if not nm.last["converged"]:
                return nm
    return nm


@functools.lru_cache(maxsize=None)
def time_reference(name, material, kind):
    """``(the direct double after the case, the bar on max|d - d_ref| / max|d_ref|, the options of the run under test)``: linear at
    ``tol = 1e-12`` with ``10 N tol kappa`` (``kappa`` of the largest ``dt`` of the run), ``svk`` at the default ``tol`` with 1e-8 against the
    double at 1e-13."""
    p = imp.problem(name)
    if material == "linear":
        n, dt = (3, TIME_DT) if kind == "ramp" else (4, TIME_DT_NEW)
        return time_run(imp.Newmark, p, material, kind), 10 * n * 1e-12 * imp.modal_kappa(p, dt * p.dt_crit), {"tol": 1e-12}
    return time_run(imp.Newmark, p, material, kind, tol=1e-13, at_floor=True), 1e-8, {"tol": 1e-10}


def units_inputs(name, u):
    """``(mass, load, dt, alpha, start)`` of the nonlinear case in the units ``u``: the unscaled ones times their powers of two."""
    p = imp.problem(name)
    return (p.mass * unit("mass", u), p.load(200.0) * unit("load", u), 5.0 * p.dt_crit * unit("dt", u), 0.5 * unit("alpha", u),
            imp.nonlinear_start(p) * unit("d", u))


def _units_run(name, material, u, seen):
    prob = scaled_problem(name, u) if u else imp.problem(name)
    mass, load, dt, alpha, start = units_inputs(name, u)
    nm = NewmarkPCG(prob, mass, load, dt, alpha, ramp=False, material=material, seen=seen)
    nm.set_state(start)
    total, per_step, info = run(nm, EDGE_STEPS)
    assert info["converged"]
    return (nm.d.copy(), nm.v.copy(), nm.a.copy()), total, per_step


_units_cache = {}


def units_run(name, material, u, seen=None):
    """``((d, v, a), totals, Newton per step)`` of :class:`NewmarkPCG` after 3 steps of the nonlinear case in the units ``u`` (0: the
    plain one, cached)."""
    if u == 0 and seen is None:
        if (name, material) not in _units_cache:
            _units_cache[name, material] = _units_run(name, material, 0, None)
        return _units_cache[name, material]
    return _units_run(name, material, u, seen)
