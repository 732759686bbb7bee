"""The cases that take the finite-strain element passes of ``csrc/saa_opfs.hip`` off the moderate-strain unit beam, their
longdouble reference and the bar.  Shared by tests/test_finite_strain_extended.py (CPU) and
tests/test_gpu_finite_strain_extended.py.  Lives under tests/: the product never imports it; it is not a test.

The reference is :class:`finite_strain_double.FiniteStrain` in ``np.longdouble``, which evaluates neo-Hooke from ``H`` without
a cancellation at any strain.  The bar, the envelope and the mesh transforms are those of tests/operator_extended.py: per
output (``f``, ``energy_elem``) ``err = max|y - r| / max|r| <= 1e-12 + 8 env``, ``env`` the largest relative change of the
reference over 8 seeded draws in which every floating-point input (points, ``lambda``, ``mu``, the displacement) is
multiplied by ``1 + d``, ``d`` uniform in ``+-2^-53``.

Meshes: the four of ``finite_strain_double.MESHES``, clamped on ``x = 0`` (rotation and dilation: no Dirichlet dofs).  The
displacement is ``smooth_random_field`` scaled to ``max|H|`` (computed on the transformed, unshifted mesh).  A case is
``(mesh, family, value, max|H|)``:

* ``strain``: ``max|H|`` 1e-2, 1e-4, 1e-6, 1e-8 (0.3 is tests/test_gpu_finite_strain.py);
* ``nu``: 0.49, 0.4999, 0.499999 at ``max|H|`` 0.3 and 1e-6, -0.3 at 0.3;
* ``mindet``: the field scaled up by bisection until the reference's ``min det F`` over all points is 1e-1, 1e-2, 1e-3 (to
  1 %), positive everywhere;
* ``rotation``: ``rigid_motion(points, 0.5)`` plus the field at ``max|H|`` 1e-4, 1e-6 (the sum rounded to float64 once);
* ``dilation``: ``u = 0.02 X`` plus the field at ``max|H|`` 1e-3, no Dirichlet dofs: ``y = J^2 - 1`` lies in (1/16, 1/4) at
  every point, where the kernel takes ``y - log1p(y)`` as the difference (above its threshold 1/16) and the reference its
  series (below its threshold 1/4);
* ``shift`` by ``(s, -s, s/3)``, ``s = 2^10, 2^20``; ``needle`` (y times 1e-3); ``sliver`` (``V / h^3 = 1e-6`` in every fifth
  element); ``curved`` (order 2, the straight 36-element beam with mid-edge nodes moved by 0.2 of the edge): each at
  ``max|H|`` 0.3 and 1e-6.

Every case is qualified on the CPU (tests/test_finite_strain_extended.py: the stable float64 restatement within ``1e-12 + 2
env`` and ``env <= 1e-6``) with the parameters above; none had to be adjusted for that.  One deviation, in the check of the
longdouble reference against mpmath at 2^-58 (four elements per family): the rotation family enters it with ``max|H| = 0.3``
next to the rotation, not with the 1e-4 and 1e-6 of its cases here.  At a strain ``s`` a rotation amplifies every rounding by
``|H| / s``, in any form and either material, so longdouble itself is 5e-12 from mpmath at ``s = 1e-6`` - 2^-11 of the
envelope, 1e6 times 2^-58; for those cases the reference is held to ``2^-58 + 2^-11 * 8 env`` instead, a looser bound than
2^-58, which leaves it 2^-11 of the bar from the truth.  The largest envelopes: 2e-8 (rotation plus a
strain of 1e-6: the rotation amplifies the rounding of ``u`` by ``|H| / strain``), 1e-9 (shift by 2^20), 2e-10 (slivers) and,
for neo-Hooke alone, 2e-12 at ``min det F = 1e-3`` (``1/J`` and ``log J``); the bar follows them.

Units (no bar): coordinates and displacements times ``2^(40 u)``, ``lambda`` and ``mu`` times ``4^(10 u)``; ``H`` and ``J`` do
not change, so ``f`` is the unscaled one times ``2^(100 u)`` and ``energy_elem`` times ``2^(140 u)``, bit for bit."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import operator_extended as ox

STRAINS = (1e-2, 1e-4, 1e-6, 1e-8)
NUS = (0.49, 0.4999, 0.499999)
MIN_DETS = (1e-1, 1e-2, 1e-3)
DILATION = 0.02                                                        # J = 1.02^3: J^2 - 1 = 0.126
OUTPUTS = ("f", "energy_elem")
UNIT_EXPONENT = {"f": ox.UNIT_EXPONENT["sigma"] + 2 * 40, "energy_elem": ox.UNIT_EXPONENT["energy"]}
ORDER2 = ("beam36", "curved288")
FLOAT_INPUTS = ("points", "lmd", "mu", "u")


def case_ids():
    out = []
    for m in fd.MESHES:
        out += [(m, "strain", 0, s) for s in STRAINS]
        out += [(m, "nu", nu, s) for nu in NUS for s in (0.3, 1e-6)] + [(m, "nu", -0.3, 0.3)]
        out += [(m, "mindet", d, 0) for d in MIN_DETS]
        out += [(m, "rotation", 0.5, s) for s in (1e-4, 1e-6)]
        out += [(m, "dilation", DILATION, 1e-3)]
        out += [(m, "shift", v, s) for v in ox.SHIFTS for s in (0.3, 1e-6)]
        out += [(m, "needle", 1e-3, s) for s in (0.3, 1e-6)]
        out += [(m, "sliver", 1e-6, s) for s in (0.3, 1e-6)]
    out += [("beam36", "curved", 0.2, s) for s in (0.3, 1e-6)]
    return out


def case_name(cid):
    m, fam, val, s = cid
    return f"{m}-{fam}-{val:g}-{s:g}"


def scale_to_min_det(fs, u, target):
    """``u`` scaled by bisection on the factor until ``min det F`` of the double ``fs`` is within 1 % of ``target`` from
    above: ``H`` is linear in ``u``, so only ``det(I + s H)`` is evaluated again.  ``min det F`` is 1 at ``s = 0`` and
    continuous; the bracket is the first doubling that goes below the target."""
    H = fs.gradient(u)

    def min_det(s):
        return float(fs._cofactors(fs._f(s * H))[1].min())

    lo, hi = 0.0, 1.0 / float(np.abs(H).max())
    while min_det(hi) > target:
        lo, hi = hi, 2.0 * hi
        assert hi < 1e6
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        d = min_det(mid)
        if d < target:
            hi = mid
        else:
            lo = mid
            if d <= 1.01 * target:
                break
    return np.asarray(u, dtype=np.float64) * lo


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """The float64 inputs of one case: ``points``, ``cells``, ``dd`` (Dirichlet dofs), ``lmd``, ``mu``, ``u (3 n,)``."""
    mesh, family, value, hmax = cid
    points, cells, dd = fd.mesh(mesh)
    nu = value if family == "nu" else fd.NU
    if family == "sliver":
        points, cells = ox.make_slivers(points, cells, value)
    if family == "curved":
        points = ox.make_curved(points, cells, value)
    if family == "needle":
        points = points * np.array([1.0, value, 1.0])
    if family in ("rotation", "dilation"):
        dd = np.zeros(0, dtype=np.int64)
    points = np.ascontiguousarray(points)
    lmd, mu = fd.lame(fd.E, nu)
    fs = fd.FiniteStrain(points, cells, lmd, mu, dd)
    assert fs.ext.min_det() > 0, (cid, fs.ext.min_det())
    seed = 2000 + sum(ord(c) for c in case_name(cid))
    field = fd.smooth_random_field(points, seed)
    if family == "mindet":
        u = scale_to_min_det(fs, field, value)
    else:
        u = field * (hmax / float(np.abs(fs.gradient(field)).max()))
    if family == "rotation":
        u = np.asarray(fd.rigid_motion(points, value) + np.asarray(u, dtype=np.longdouble), dtype=np.float64)
    if family == "dilation":
        u = value * points.reshape(-1) + u
    if family == "shift":
        s = 2.0 ** value
        points = points + np.array([s, -s, s / 3.0])
    return {"id": cid, "points": points, "cells": cells, "dd": np.asarray(dd, dtype=np.int64), "lmd": lmd, "mu": mu, "u": u}


def outputs(case, material, T=np.longdouble, textbook=False):
    """``({"f", "energy_elem"}, inverted, FiniteStrain)`` of the case in the arithmetic ``T``."""
    fs = fd.FiniteStrain(case["points"], case["cells"], case["lmd"], case["mu"], case["dd"], T=T, textbook=textbook)
    f, en, inv = fs.evaluate(case["u"], material)
    return {"f": f[None], "energy_elem": en[None]}, inv, fs


def perturbed(case, rng):
    """As ``operator_extended.perturbed``, on this module's inputs."""
    out = dict(case)
    for k in FLOAT_INPUTS:
        v = np.asarray(case[k], dtype=np.longdouble)
        d = np.asarray(rng.uniform(-1.0, 1.0, size=v.shape), dtype=np.longdouble) * np.longdouble(2.0) ** -53
        out[k] = v * (1 + d)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """``(case, ref, env, info)``: per material the longdouble outputs ``ref[material][name] (1, ...)`` and the envelope
    ``env[material][name] (1,)`` as ``operator_extended.reference`` computes it; ``info`` holds ``det`` (``det F (ne, nq)``),
    ``min_det`` and ``hmax`` of the reference and ``inverted[material]``."""
    case = build_case(cid)
    ref, env, info = {}, {}, {"inverted": {}}
    for material in fd.MATERIALS:
        ref[material], info["inverted"][material], fs = outputs(case, material)
        env[material] = {k: np.zeros(1) for k in OUTPUTS}
    info["det"] = fs.det_f(case["u"])
    info["min_det"], info["hmax"] = float(info["det"].min()), float(np.abs(fs.gradient(case["u"])).max())
    rng = np.random.default_rng(77)
    for _ in range(ox.N_DRAWS):
        alt_case = perturbed(case, rng)
        for material in fd.MATERIALS:
            alt = outputs(alt_case, material)[0]
            for k in OUTPUTS:
                r = ref[material][k]
                env[material][k] = np.maximum(env[material][k], np.asarray(np.abs(alt[k] - r).max(axis=1) / np.abs(r).max(axis=1),
                                                                           dtype=np.float64))
    return case, ref, env, info


def check(got, cid, material, factor, label=None, names=OUTPUTS, verbose=True):
    """``operator_extended.check`` of ``got`` (name -> array) against the reference of the case: ``(worst, bad)``."""
    _, ref, env, _ = reference(cid)
    got = {k: np.asarray(got[k])[None] for k in names}
    return ox.check(got, ref[material], env[material], factor, label or f"{case_name(cid)} {material}", names=list(names),
                    verbose=verbose)


def scaled_case(case, u):
    """``operator_extended.scaled_case`` for the force and the energy: lengths times ``2^(40 u)``, moduli ``4^(10 u)``."""
    L, S = 2.0 ** (40 * u), 4.0 ** (10 * u)
    out = dict(case)
    out["points"], out["u"] = case["points"] * L, case["u"] * L
    out["lmd"], out["mu"] = case["lmd"] * S, case["mu"] * S
    return out


def unit_cases():
    """The cases of the units family: every mesh at ``nu = 0.3``, at ``max|H|`` 0.3 and 1e-6 (the series of ``y - log1p(y)``)."""
    return [(m, "strain", 0, s) for m in fd.MESHES for s in (0.3, 1e-6)]


def sub_case(case, n_elems=4):
    """The first elements of a case as a mesh of their own (``operator_extended.sub_mesh``), displacement and Dirichlet dofs
    renumbered with the nodes."""
    nodes, points, cells = ox.sub_mesh(case["points"], case["cells"], n_elems)
    old = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    out = dict(case)
    out["points"], out["cells"], out["u"] = points, cells, case["u"][old]
    out["dd"] = np.nonzero(np.isin(old, case["dd"]))[0]
    return out


def partial_inversion_state(fs, points, background=None, margin=1e-3):
    """``(u (3 n,), partial)``: ``background`` plus one free vertex moved alone - its mid-edge nodes stay, so that ``det F``
    varies strongly inside its elements - such that in the double ``fs`` (order 2) at least one element has ``J > 0`` at some
    of its Gauss points and ``J <= 0`` at others (``partial``, sorted), with ``|J| >= margin`` at every point of the mesh so
    that no rounding decides a sign.  A deterministic search in the style of ``finite_strain_double.inversion_state`` over the
    free vertices, a fixed list of directions and four lengths; the first hit is returned."""
    points = np.asarray(points, dtype=np.float64)
    base = np.zeros(3 * len(points)) if background is None else np.asarray(background, dtype=np.float64)
    dirs = [np.array(d, dtype=np.float64) for d in ((1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, 1, 1), (0, 1, 1), (0, -1, 1))]
    for node in np.unique(fs.cells[:, :4]):
        if not fs.free[3 * node:3 * node + 3].all():
            continue
        for d in dirs:
            for length in (0.5, 0.75, 1.0, 1.5):
                u = base.copy()
                u[3 * node:3 * node + 3] += length * d / np.linalg.norm(d)
                det = np.asarray(fs.det_f(u), dtype=np.float64)
                partial = np.nonzero((det > 0).any(axis=1) & (det <= 0).any(axis=1))[0]
                if len(partial) and np.abs(det).min() >= margin:
                    return u, partial
    raise AssertionError("no vertex of this mesh inverts an element at some of its points only")
