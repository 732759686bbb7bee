"""The cases that take the finite-strain stress recovery of ``csrc/saa_stress_fs.hip`` (``saa_operator_stress_finite``) off
the moderate-strain beam, their longdouble reference and the bar.  Shared by tests/test_fs_stress_extended.py (CPU) and
tests/test_gpu_fs_stress_extended.py.  Lives under tests/: the product never imports it; it is not a test.

The reference is :class:`fs_stress_double.FsStress` in ``np.longdouble``, which takes the differences of the normal stresses
before the common pressure goes in.  The cases, their builder, the perturbation, the unit scaling and the sub-meshes are those
of tests/finite_strain_extended.py (``fx``), the bar and the envelope those of tests/operator_extended.py (``ox``): per output
and per ``(material, measure)``, ``err = max|y - r| / max|r| <= 1e-12 + 8 env``, ``env`` the largest relative change of the
reference over 8 seeded draws (seed 77) in which every floating-point input (points, ``lambda``, ``mu``, the displacement) is
multiplied by ``1 + d``, ``d`` uniform in ``+-2^-53``; the argmax by ``ox.check``'s rule.  Outputs: ``stress``, ``von_mises``,
``det_f``, ``energy``, ``energy_total``, ``von_mises_max``, ``von_mises_argmax``.

The stress passes ignore the Dirichlet mask, and ``fx.build_case`` sizes ``u`` through the masked gradient: :func:`build_case`
sets ``u`` to 0 on the case's ``dd``, so that the unmasked ``max|H|`` and ``min det F`` are the nominal ones
(tests/test_fs_stress_extended.py asserts that to 1 %, and that nothing is inverted).

Cases, a trimmed list of ``fx.case_ids()`` (four evaluations per case): per mesh of ``finite_strain_double.MESHES``

* ``strain`` 1e-4 and 1e-8;
* ``nu`` 0.499999 at ``max|H|`` 0.3 and 1e-6, 0.4999 at 1e-6;
* ``mindet`` 1e-2 and 1e-3;
* ``rotation`` 0.5 rad at 1e-6;
* ``dilation``;
* ``shift`` by 2^20 at 0.3 and 1e-6;
* ``needle`` 1e-3 at 1e-6;
* ``sliver`` 1e-6 at 0.3;

plus the curved 36-element beam at 0.3 and 1e-6: 54 cases.  Every one is qualified on the CPU with the parameters above (the
stable float64 restatement within ``1e-12 + 2 env``, ``env <= 1e-6``); none had to be replaced.  The largest envelopes, over
the four combinations and every output: 2.1e-8 (rotation next to a strain of 1e-6: the rotation amplifies the rounding of ``u``
by ``|H| / strain``), 2.0e-9 and 1.3e-9 (shift by 2^20, at 0.3 and 1e-6), 6.5e-10 (slivers), 6.1e-12 and 3.0e-13 (``min det F``
1e-3 and 1e-2: ``1 / J``), 4.5e-13 (dilation: the deviator is a twentieth of ``H``), 6.6e-14 (``eta^2`` at ``nu = 0.499999``) and
1e-14 to 2e-14 everywhere else (``delaunay2``, whose elements are the least regular); the bar follows them.  One deviation, in
the check of the longdouble reference against mpmath at 2^-58 (four elements per family): the rotation family is held as
tests/finite_strain_extended.py explains, and the von Mises value of the dilation family in the same way (longdouble is 2.0e-17
from mpmath there, at an envelope of 3e-14: the deviator sees the rounding of ``H = 0.02 I`` amplified twenty times and more).

The composite cases (:func:`composite_ids`: ``nu = 0.499999`` at both strains and ``sliver``, on every mesh) carry, for the PK2
field of each material, the nodal recovery and the Zienkiewicz-Zhu ``eta^2`` of ``operator_extended.Extended.nodal`` /
``.error`` applied to the longdouble PK2 field, with the envelope taken over the whole chain from the inputs.

Units (no bar): coordinates and displacements times ``2^(40 u)``, ``lambda`` and ``mu`` times ``4^(10 u)``; ``H`` and ``J`` do
not change, so the stresses are the unscaled ones times ``2^(20 u)``, the energies times ``2^(140 u)`` and ``det_f`` is the
same, bit for bit."""
from __future__ import annotations

import functools

import numpy as np

import finite_strain_double as fd
import finite_strain_extended as fx
import fs_stress_double as sd
import operator_extended as ox

COMBOS = [(material, measure) for material in fd.MATERIALS for measure in sd.MEASURES]
OUTPUTS = ("stress", "von_mises", "det_f", "energy", "energy_total", "von_mises_max", "von_mises_argmax")
COMPOSITE = ("nodal", "eta2", "eta2_total")
UNIT_EXPONENT = {"stress": ox.UNIT_EXPONENT["sigma"], "von_mises": ox.UNIT_EXPONENT["sigma"],
                 "von_mises_max": ox.UNIT_EXPONENT["sigma"], "energy": ox.UNIT_EXPONENT["energy"],
                 "energy_total": ox.UNIT_EXPONENT["energy"], "det_f": 0}


def case_ids():
    out = []
    for m in fd.MESHES:
        out += [(m, "strain", 0, s) for s in (1e-4, 1e-8)]
        out += [(m, "nu", 0.499999, 0.3), (m, "nu", 0.499999, 1e-6), (m, "nu", 0.4999, 1e-6)]
        out += [(m, "mindet", d, 0) for d in (1e-2, 1e-3)]
        out += [(m, "rotation", 0.5, 1e-6)]
        out += [(m, "dilation", fx.DILATION, 1e-3)]
        out += [(m, "shift", 20, s) for s in (0.3, 1e-6)]
        out += [(m, "needle", 1e-3, 1e-6)]
        out += [(m, "sliver", 1e-6, 0.3)]
    out += [("beam36", "curved", 0.2, s) for s in (0.3, 1e-6)]
    return out


def composite_ids():
    return [c for c in case_ids() if (c[1] == "nu" and c[2] == 0.499999) or c[1] == "sliver"]


def suspect_ids():
    """The cases on which differences of the finished ``svk`` Cauchy stress lose ``lambda / mu`` times the rounding."""
    return [(m, "nu", 0.499999, 1e-6) for m in fd.MESHES]


case_name = fx.case_name


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """``fx.build_case(cid)`` with ``u`` set to 0 on the case's Dirichlet dofs: the stress passes apply no mask."""
    case = dict(fx.build_case(cid))
    u = np.array(case["u"], dtype=np.float64)
    u[case["dd"]] = 0.0
    case["u"] = u
    return case


def outputs(case, T=np.longdouble, kernel_order=False, composite=False, combos=None):
    """``({(material, measure): {name: (1, ...) array}}, FsStress)`` of the case in the arithmetic ``T``; ``n_inverted`` rides
    along as an int.  ``composite``: the PK2 entries gain ``nodal (1, n, 6)``, ``eta2 (1, ne)`` and ``eta2_total (1,)`` of
    their own stress field."""
    dbl = sd.FsStress(case["points"], case["cells"], case["lmd"], case["mu"], T=T, kernel_order=kernel_order)
    res = dbl.recover_all(case["u"], combos)
    out = {}
    for key, r in res.items():
        out[key] = {k: np.asarray(r[k])[None] for k in OUTPUTS}
        out[key]["von_mises_argmax"] = np.asarray([r["von_mises_argmax"]], dtype=np.int64)
        out[key]["n_inverted"] = r["n_inverted"]
        if composite and key[1] == "pk2":
            ext = dbl.fs.ext
            S = r["stress"] if ext.order == 2 else r["stress"][:, 0]
            nodal = ext.nodal(S[None])
            err = ext.error(S[None], nodal=nodal)
            out[key].update({"nodal": nodal, "eta2": err["eta2"], "eta2_total": err["eta2_total"]})
    return out, dbl


def reference_of(case, composite=False):
    """``(ref, env, info)`` of a case: per ``(material, measure)`` the longdouble outputs ``ref[key][name] (1, ...)`` and the
    envelopes ``env[key][name] (1,)``; ``info`` holds ``hmax`` (the unmasked ``max|H|``), ``min_det`` and ``n_inverted[key]``."""
    ref, dbl = outputs(case, composite=composite)
    info = {"n_inverted": {key: r.pop("n_inverted") for key, r in ref.items()},
            "hmax": float(np.abs(dbl.fs.gradient(case["u"])).max()),
            "min_det": float(ref["svk", "pk2"]["det_f"].min())}
    env = {key: {k: np.zeros(1) for k in r if k not in ox.ARG_OF} for key, r in ref.items()}
    rng = np.random.default_rng(77)
    for _ in range(ox.N_DRAWS):
        alt = outputs(fx.perturbed(case, rng), composite=composite)[0]
        for key, e in env.items():
            for k in e:
                r, a = ref[key][k].reshape(1, -1), alt[key][k].reshape(1, -1)
                e[k] = np.maximum(e[k], np.asarray(np.abs(a - r).max(axis=1) / np.abs(r).max(axis=1), dtype=np.float64))
    return ref, env, info


@functools.lru_cache(maxsize=None)
def reference(cid):
    """``(case, ref, env, info)`` of :func:`reference_of` for a case of the list, computed once."""
    case = build_case(cid)
    return (case,) + reference_of(case, cid in composite_ids())


@functools.lru_cache(maxsize=None)
def edge_reference(mesh, n_elems):
    """``(case, ref, env, info)`` of the first ``n_elems`` elements of ``mesh`` as a mesh of their own (``fx.sub_case``), at
    ``max|H| = 0.3`` of the whole mesh's field."""
    case = fx.sub_case(build_case((mesh, "strain", 0, 0.3)), n_elems)
    return (case,) + reference_of(case)


def check_fields(got, ref, env, key, factor, label, names=OUTPUTS, verbose=True):
    """``operator_extended.check`` of ``got`` (name -> array without the leading axis) against ``ref[key]``: ``(worst, bad)``."""
    got = {k: np.asarray(got[k])[None] for k in names}
    return ox.check(got, ref[key], env[key], factor, label, names=list(names), verbose=verbose)


def check(got, cid, key, factor, label=None, names=OUTPUTS, verbose=True):
    """:func:`check_fields` against the reference of the case ``cid``."""
    _, ref, env, _ = reference(cid)
    return check_fields(got, ref, env, key, factor, label or f"{case_name(cid)} {key[0]} {key[1]}", names, verbose)


def nominal(case):
    """``max|H|`` of the strain part of the case's displacement in longdouble: of ``u`` itself, less the rigid motion in the
    rotation family and the dilation in its own."""
    _, family, value, _ = case["id"]
    T = np.longdouble
    u = np.asarray(case["u"], dtype=T)
    if family == "rotation":
        u = u - fd.rigid_motion(case["points"], value)
    if family == "dilation":
        u = u - T(value) * np.asarray(case["points"], dtype=T).reshape(-1)
    fs = fd.FiniteStrain(case["points"], case["cells"], case["lmd"], case["mu"], ())
    return float(np.abs(fs.gradient(u)).max())


def with_copy(name, first=256, n_copy=32, hmax=0.3):
    """``(points, cells, u, part, centre)``: the mesh ``name`` followed by a disconnected copy of its first ``n_copy`` elements
    on nodes of their own (``operator_extended.sub_mesh``), translated clear of the mesh along y; the copy is elements ``ne``
    to ``ne + n_copy - 1``.  The mesh itself is cut behind its first ``first`` elements: the elements from ``first`` on get
    nodes of their own at the same coordinates (every element keeps its place and its geometry; the stress passes work
    element by element, so nothing they compute changes), because a part can only be reflected while its neighbours stay
    healthy if they share no node.  ``part (n,)`` is 0, 1 or 2 per node (the first ``first`` elements, the rest of the mesh,
    the copy) and ``centre (n, 3)`` the centroid of the node's part: ``u = -2 (X - centre)`` reflects a part through its
    centroid, ``F = -I`` and ``det F = -1`` at every point.  ``u (3 n,)`` is the seeded field at ``max|H| = hmax``."""
    points, cells, _ = fd.mesh(name)
    pieces = [ox.sub_mesh(points, cells, first)[1:], ox.sub_mesh(points, cells[first:], len(cells) - first)[1:],
              ox.sub_mesh(points, cells, n_copy)[1:]]
    span = points.max(axis=0) - points.min(axis=0)
    pieces[2] = (pieces[2][0] + np.array([0.0, 2.0 * span[1] + 1.0, 0.0]), pieces[2][1])
    all_points, all_cells, part, centre, n = [], [], [], [], 0
    for k, (p, c) in enumerate(pieces):
        all_points.append(p)
        all_cells.append(c + n)
        part.append(np.full(len(p), k))
        centre.append(np.broadcast_to(p.mean(axis=0), p.shape))
        n += len(p)
    all_points, all_cells = np.ascontiguousarray(np.concatenate(all_points)), np.concatenate(all_cells)
    lmd, mu = fd.lame(fd.E, fd.NU)
    fs = fd.FiniteStrain(all_points, all_cells, lmd, mu, ())
    field = fd.smooth_random_field(all_points, 4100 + len(name))
    u = field * (hmax / float(np.abs(fs.gradient(field)).max()))
    return all_points, all_cells, u, np.concatenate(part), np.concatenate(centre)


@functools.lru_cache(maxsize=None)
def copy_reference(name):
    """``(case, columns (3, 3 n), ref, env, n_inverted)`` of the workgroup test on :func:`with_copy` of ``name``: column 0 healthy
    everywhere, column 1 with the copy reflected, column 2 with the first 256 elements reflected and the rest healthy;
    ``ref[j][key][name]``, ``env[j][key][name]`` and ``n_inverted[j][key]`` per column as :func:`reference_of` gives them."""
    points, cells, u, part, centre = with_copy(name)
    lmd, mu = fd.lame(fd.E, fd.NU)
    flip = (-2.0 * (points - centre)).reshape(-1)
    on = lambda k: np.repeat(part == k, 3)  # noqa: E731
    columns = np.stack([u, np.where(on(2), flip, u), np.where(on(0), flip, u)])
    case = {"points": points, "cells": cells, "dd": np.zeros(0, dtype=np.int64), "lmd": lmd, "mu": mu}
    ref, env, count = [], [], []
    for col in columns:
        r, e, info = reference_of({**case, "u": col})
        ref.append(r)
        env.append(e)
        count.append(info["n_inverted"])
    return case, columns, ref, env, count
