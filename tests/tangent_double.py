"""NumPy double of the tangent element pass of ``csrc/saa_optan.hip``, the cases it is tested on and a float64 Newton with the
dense tangent.  Shared by tests/test_tangent.py (CPU) and tests/test_gpu_tangent.py.  Lives under tests/: the product never
imports it; it is not a test.

Built on :class:`finite_strain_double.FiniteStrain` (its ``gradient``, ``_cofactors`` and the scatter of its geometry), in the
same arithmetics (``np.longdouble`` by default, ``np.float64`` as the stable restatement, ``operator_extended.MP``).  With ``H =
grad_X u`` and ``dH = grad_X v`` (both masked on Dirichlet dofs) at every point of the K rule

* ``svk``: ``dE = (dH + dH^T + H^T dH + dH^T H)/2``, ``dS = lam tr(dE) I + 2 mu dE``, ``dP = dH S + F dS``;
* ``neo_hookean``: ``dP = mu dH + (mu - lam ln J) F^-T dH^T F^-T + lam (F^-T : dH) F^-T`` with ``F^-T - I`` and ``ln J`` from ``H`` as
  ``FiniteStrain.stress`` has them (cofactors of ``H``, ``log1p(J - 1)``);

``kv_a[i] = sum_q w_q detJ_q sum_k dP_q[i][k] dN_a/dX_k(q)``, summed over the elements and set to 0 on Dirichlet dofs.  Under
``neo_hookean`` an element with ``!(J > 0)`` at any point is dropped, as in ``FiniteStrain.evaluate``.

The cases are those of tests/finite_strain_extended.py (``build_case``, ``perturbed``, ``sub_case`` by import) with two
directions ``v`` each - uniform noise and ``smooth_random_field`` - and the same bar: ``err = max|y - r| / max|r| <= 1e-12 + 8
env``, ``env`` from 8 draws that perturb ``points, lmd, mu, u, v`` by ``+-2^-53``."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import finite_strain_extended as fx
import operator_extended as ox
from operator_extended import conv, log1p, zeros

DIRECTIONS = ("random", "smooth")


class Tangent(fd.FiniteStrain):
    """``K_T(u) v`` next to ``f_int(u)`` of :class:`finite_strain_double.FiniteStrain`."""

    def dstress(self, H, dH, material):
        """``(dP (ne, nq, 3, 3), inverted (ne,) bool)``: the derivative of ``P`` at ``H`` in the direction ``dH``."""
        dP = zeros(H.shape, self.T)
        if material == "svk":
            F = self._f(H)
            Em, dE = zeros(H.shape, self.T), zeros(H.shape, self.T)
            for i in range(3):
                for k in range(3):
                    Em[..., i, k] = H[..., i, k] + H[..., k, i]
                    dE[..., i, k] = dH[..., i, k] + dH[..., k, i]
                    for l in range(3):
                        Em[..., i, k] = Em[..., i, k] + H[..., l, i] * H[..., l, k]
                        dE[..., i, k] = dE[..., i, k] + H[..., l, i] * dH[..., l, k] + dH[..., l, i] * H[..., l, k]
            Em, dE = Em / 2, dE / 2
            S, dS = 2 * self.mu * Em, 2 * self.mu * dE
            tr, dtr = Em[..., 0, 0] + Em[..., 1, 1] + Em[..., 2, 2], dE[..., 0, 0] + dE[..., 1, 1] + dE[..., 2, 2]
            for i in range(3):
                S[..., i, i] = S[..., i, i] + self.lmd * tr
                dS[..., i, i] = dS[..., i, i] + self.lmd * dtr
            for i in range(3):
                for k in range(3):
                    for l in range(3):
                        dP[..., i, k] = dP[..., i, k] + dH[..., i, l] * S[..., l, k] + F[..., i, l] * dS[..., l, k]
            return dP, np.zeros(self.n_elems, dtype=bool)
        if material != "neo_hookean":
            raise ValueError(f"unknown material {material!r}")
        A, det_h = self._cofactors(H)
        rest = A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2] + det_h
        x = H[..., 0, 0] + H[..., 1, 1] + H[..., 2, 2] + rest
        J = 1 + x
        ok = np.asarray(J > 0, dtype=bool)
        inverted = ~ok.all(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            xs, Js = np.where(ok, x, conv(0.0, self.T)), np.where(ok, J, conv(1.0, self.T))
            c = self.mu - self.lmd * log1p(xs, self.T)
            Fi = zeros(H.shape, self.T)                                # F^-T = I + (F^-T - I)
            for i in range(3):
                for k in range(3):
                    D = A[..., i, k] - H[..., k, i]
                    if i == k:
                        D = D - rest
                    Fi[..., i, k] = (1 if i == k else 0) + D / Js
            M = zeros(H.shape, self.T)                                 # F^-T dH^T
            for i in range(3):
                for k in range(3):
                    for l in range(3):
                        M[..., i, k] = M[..., i, k] + Fi[..., i, l] * dH[..., k, l]
            t = M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2]             # F^-T : dH
            for i in range(3):
                for k in range(3):
                    B = zeros(H.shape[:2], self.T)
                    for l in range(3):
                        B = B + M[..., i, l] * Fi[..., l, k]
                    dP[..., i, k] = self.mu * dH[..., i, k] + c * B + self.lmd * t * Fi[..., i, k]
        return dP, inverted

    def tangent_full(self, u, v, material):
        """``(kv (3 n,), inverted (ne,) bool)``; inverted elements contribute 0."""
        ext = self.ext
        dP, inverted = self.dstress(self.gradient(u), self.gradient(v), material)
        zero = conv(0.0, self.T)
        f = zeros((self.n_elems, self.na, 3), self.T)
        for q in range(self.nq):
            for i in range(3):
                for k in range(3):
                    f[..., i] = f[..., i] + (ext.wdk[:, q] * dP[:, q, i, k])[:, None] * ext.grad[:, q, :, k]
        f = np.where(inverted[:, None, None], zero, f)
        return np.where(self.free, ext._scatter(f[None])[0], zero), inverted

    def tangent(self, u, v, material):
        return self.tangent_full(u, v, material)[0]

    def tangent_matrix(self, u, material):
        """The dense ``K_T(u)`` as float64 ``(3 n, 3 n)``, column by column (small meshes); rows and columns of Dirichlet dofs
        are 0."""
        ext, n = self.ext, 3 * self.n_nodes
        H = self.gradient(u)
        Ke = np.zeros((self.n_elems, self.na, 3, self.na, 3))         # [e, row corner, row comp, column corner, column comp]
        inverted = np.zeros(self.n_elems, dtype=bool)
        for a in range(self.na):                                       # the unit dof (a, j) of every element at once
            for j in range(3):
                dH = zeros(H.shape, self.T)
                dH[..., j, :] = ext.grad[:, :, a, :]
                dP, inverted = self.dstress(H, dH, material)
                f = zeros((self.n_elems, self.na, 3), self.T)
                for q in range(self.nq):
                    for i in range(3):
                        for k in range(3):
                            f[..., i] = f[..., i] + (ext.wdk[:, q] * dP[:, q, i, k])[:, None] * ext.grad[:, q, :, k]
                Ke[:, :, :, a, j] = np.asarray(f, dtype=np.float64)
        Ke[inverted] = 0.0
        dof = (3 * self.cells[:, :, None] + np.arange(3)[None, None, :]).reshape(self.n_elems, -1)
        K = np.zeros((n, n))
        np.add.at(K, (dof[:, :, None], dof[:, None, :]), Ke.reshape(self.n_elems, 3 * self.na, 3 * self.na))
        K[~self.free, :] = 0.0
        K[:, ~self.free] = 0.0
        return K


def newton(fs, b, material, tol=1e-12, load_steps=8, max_iter=40):
    """A float64 Newton iteration with the dense tangent of ``fs`` (a :class:`Tangent` in ``np.float64``) for ``f_int(u) = b`` on
    the free dofs, from 0: the load in ``load_steps`` equal fractions, per fraction full Newton steps (dense solve) halved
    while ``Pi(u) - b_k . u`` does not fall or an element inverts.  ``(u, relative residual, iterations)``."""
    free = np.nonzero(fs.free)[0]
    b = np.where(fs.free, np.asarray(b, dtype=np.float64), 0.0)
    u = np.zeros_like(b)
    bn, its = np.linalg.norm(b), 0
    for step in range(1, load_steps + 1):
        bk = b * (step / load_steps)

        def look(x):
            f, en, inv = fs.evaluate(x, material)
            return np.where(fs.free, bk - f, 0.0), float(en.sum() - bk @ x), bool(inv.any()) or float(fs.det_f(x).min()) <= 0

        r, phi, _ = look(u)
        for _ in range(max_iter):
            if np.linalg.norm(r) <= tol * bn:
                break
            du = np.zeros_like(u)
            du[free] = np.linalg.solve(fs.tangent_matrix(u, material)[np.ix_(free, free)], r[free])
            t = 1.0
            while True:
                rt, phit, bad = look(u + t * du)
                if (not bad and phit <= phi + 1e-12 * abs(phi)) or t < 1e-8:
                    break
                t *= 0.5
            u, r, phi = u + t * du, rt, phit
            its += 1
    r = np.where(fs.free, b - np.asarray(fs.force(u, material), dtype=np.float64), 0.0)
    return u, float(np.linalg.norm(r) / bn), its


# ---- the cases --------------------------------------------------------------------------------------------------------------

def case_ids():
    """The families of the parity test as case ids of tests/finite_strain_extended.py."""
    out = []
    for m in fd.MESHES:
        out += [(m, "strain", 0, s) for s in (0.3, 1e-4, 1e-8)]
        out += [(m, "nu", 0.499999, s) for s in (0.3, 1e-6)]
        out += [(m, "mindet", 1e-2, 0), (m, "rotation", 0.5, 1e-6), (m, "shift", 20, 0.3), (m, "sliver", 1e-6, 0.3)]
    out += [("beam36", "curved", 0.2, 0.3)]
    return out


def unit_cases():
    return [(m, "strain", 0, 0.3) for m in fd.MESHES]


FLOAT_INPUTS = fx.FLOAT_INPUTS + tuple("v_" + d for d in DIRECTIONS)
# lengths times 2^(40 u), moduli times 4^(10 u): K_T carries stress times length, v a length
KV_UNIT_EXPONENT = ox.UNIT_EXPONENT["kx"]


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """``finite_strain_extended.build_case`` plus the two directions ``v_random`` and ``v_smooth`` (``(3 n,)`` float64, of the
    size of the mesh's displacement scale 1)."""
    case = dict(fx.build_case(cid))
    seed = 5000 + sum(ord(c) for c in fx.case_name(cid))
    n = case["points"].shape[0]
    case["v_random"] = np.random.default_rng(seed).uniform(-1.0, 1.0, size=3 * n)
    case["v_smooth"] = fd.smooth_random_field(case["points"], seed + 1)
    return case


def perturbed(case, rng):
    """``finite_strain_extended.perturbed`` with the directions perturbed too."""
    out = fx.perturbed(case, rng)
    for d in DIRECTIONS:
        v = np.asarray(case["v_" + d], dtype=np.longdouble)
        out["v_" + d] = v * (1 + np.asarray(rng.uniform(-1.0, 1.0, size=v.shape), dtype=np.longdouble) * np.longdouble(2.0) ** -53)
    return out


def scaled_case(case, u):
    out = fx.scaled_case(case, u)
    for d in DIRECTIONS:
        out["v_" + d] = case["v_" + d] * 2.0 ** (40 * u)
    return out


def sub_case(case, n_elems=4):
    """``finite_strain_extended.sub_case`` with the directions renumbered like the displacement."""
    nodes = ox.sub_mesh(case["points"], case["cells"], n_elems)[0]
    old = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    out = fx.sub_case(case, n_elems)
    for d in DIRECTIONS:
        out["v_" + d] = case["v_" + d][old]
    return out


def outputs(case, material, T=np.longdouble):
    """``({"random": kv (1, 3 n), "smooth": ...}, inverted, Tangent)`` of the case in the arithmetic ``T``."""
    fs = Tangent(case["points"], case["cells"], case["lmd"], case["mu"], case["dd"], T=T)
    out, inverted = {}, None
    for d in DIRECTIONS:
        kv, inverted = fs.tangent_full(case["u"], case["v_" + d], material)
        out[d] = kv[None]
    return out, inverted, fs


def envelope(case, ref_of, outputs_of):
    """``env``: per name the largest relative change of ``outputs_of(case)`` over ``N_DRAWS`` perturbed draws (seed 77)."""
    rng = np.random.default_rng(77)
    env = {k: np.zeros(1) for k in ref_of}
    for _ in range(ox.N_DRAWS):
        alt = outputs_of(perturbed(case, rng))
        for k in env:
            env[k] = np.maximum(env[k], np.asarray(np.abs(alt[k] - ref_of[k]).max(axis=1) / np.abs(ref_of[k]).max(axis=1),
                                                   dtype=np.float64))
    return env


@functools.lru_cache(maxsize=None)
def reference(cid):
    """``(case, ref, env)``: per material the longdouble ``ref[material][direction] (1, 3 n)`` and its envelope ``(1,)``."""
    case = build_case(cid)
    ref, env = {}, {}
    for material in fd.MATERIALS:
        ref[material], inverted, _ = outputs(case, material)
        assert not inverted.any(), (cid, material)
        env[material] = envelope(case, ref[material], lambda c: outputs(c, material)[0])
    return case, ref, env


def check(got, cid, material, factor, label=None, verbose=True):
    """``operator_extended.check`` of ``got`` (direction -> ``(3 n,)``) against the reference of the case: ``(worst, bad)``."""
    _, ref, env = reference(cid)
    names = [d for d in DIRECTIONS if d in got]
    return ox.check({d: np.asarray(got[d])[None] for d in names}, ref[material], env[material], factor,
                    label or f"{fx.case_name(cid)} {material}", names=names, verbose=verbose)


def stretched_state(points, fs):
    """A dilation-plus-field state with every ``det F > 0``: ``u = 0.1 X`` plus ``smooth_random_field`` at ``max|H| = 0.05``,
    masked on the Dirichlet dofs of ``fs``."""
    field = fd.smooth_random_field(points, 17)
    u = 0.1 * np.asarray(points, dtype=np.float64).reshape(-1) + field * (0.05 / float(np.abs(fs.gradient(field)).max()))
    u = np.where(fs.free, u, 0.0)
    assert float(fs.det_f(u).min()) > 0.2
    return u


# ---- the static problem of the Newton tests -----------------------------------------------------------------------------

NEWTON_MESHES = ("structured288", "beam36")                            # order 1 and order 2, clamped on x = 0
TIP_OVER_LENGTH = 0.25                                                 # the LINEAR tip deflection the load is sized for


def tip_deflection(points, cells, d):
    """The mean of ``-d_y`` over the vertices of the plane ``x = max`` (what the drivers report)."""
    points = np.asarray(points)
    n_vert = int(np.asarray(cells)[:, :4].max()) + 1
    tip = np.nonzero(np.abs(points[:n_vert, 0] - points[:, 0].max()) < 1e-9)[0]
    return float(-np.asarray(d, dtype=np.float64).reshape(-1, 3)[tip, 1].mean())


@functools.lru_cache(maxsize=None)
def newton_problem(name):
    """``(points, cells, dd, fz, b, d_lin, K)`` in float64: the load ``b`` is the consistent body force ``(0, -fz, -fz)`` with
    ``fz`` such that the LINEAR solution ``d_lin = K^-1 b`` has the tip deflection ``TIP_OVER_LENGTH`` times the beam length."""
    pts, cells, dd = fd.mesh(name)
    lmd, mu = fd.lame(fd.E, fd.NU)
    fs = Tangent(pts, cells, lmd, mu, dd, T=np.float64)
    K = fs.tangent_matrix(np.zeros(3 * len(pts)), "svk")               # = the handle's K
    free = np.nonzero(fs.free)[0]
    unit = np.where(fs.free, np.asarray(fs.ext.load((0.0, -1.0, -1.0)), dtype=np.float64), 0.0)
    d = np.zeros_like(unit)
    d[free] = np.linalg.solve(K[np.ix_(free, free)], unit[free])
    fz = TIP_OVER_LENGTH * float(pts[:, 0].max() - pts[:, 0].min()) / tip_deflection(pts, cells, d)
    return pts, cells, dd, fz, fz * unit, fz * d, K
