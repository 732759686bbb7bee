"""Extended-precision reference of one step of the operator stepper (``csrc/saa_opstep.hip``: the lumped-mass kernels, the node
and finish passes with ``opstep_update_dof``, the energy partials and their final kernel), the cases that take it off the
unit beam, and the bar it is held to.  Shared by tests/test_stepper_extended.py (CPU) and tests/test_gpu_stepper_extended.py.
Lives under tests/: the product never imports it.

Arithmetic, meshes, families and the bar are those of tests/operator_extended.py (``ox``): ``err = max|y - r| / max|r| <= 1e-12
+ 8 env`` per output column, ``env`` the largest relative change of the reference over 8 draws in which every floating-point
input is multiplied by ``1 + d``, ``|d| <= 2^-53``.  A column whose reference is exactly 0 (``dD`` at ``alpha = 0``, the mass
terms of a rank that owns none of its nodes) is held to exact 0 instead.

Inputs of a stepper case, all float64 and all perturbed in the draws: the ``ox`` case (points, cells, ``lmd``, ``mu``, ``rho``); the
clamped dofs (every dof of the nodes on the face of smallest x of the vertex box; mid-edge nodes that the ``curved`` family
pushes out of that face are clamped too); ``mass`` and ``load``, which are the reference's own HRZ / row-sum mass and its
consistent load of the force density ``ox.FORCE`` rounded to float64 and handed to both sides as the stepper's vectors (the
kernels that form them are held to the bar on their own: ``mass`` here, ``load`` in tests/test_gpu_operator_extended.py); ``dt
= 0.9 * 2 / omega`` with ``omega`` the largest element frequency (``ox.element_omega`` at order 1, the same Irons-Treharne
bound from the element matrices and the HRZ element masses at order 2: an upper bound of ``omega_max(M_L^-1 K)``, clamped or
not); ``alpha``, ``tn = 0.37`` with the ramp on; and two states, the two columns of ``d0`` and ``dn``:

* column 0, *random*: both uniform noise of size 1e-3, clamped dofs included, so that ``dt^2 K d0`` is as large as ``m d0``;
* column 1, *smooth*: ``d0 = 1e-3 fd.smooth_random_field``, ``dn = d0 - dt v`` with ``v`` such a field scaled to ``max |dt v| = 1e-3
  max |d0|``: the near-cancelling ``2 d0 - dn`` of a real run.

The reference, in ``np.longdouble`` with ``ox.Extended``'s rules (elementwise loops over the small index, sums as explicit
loops; no ``einsum``, ``dot`` or ``bincount``): the masked ``s = K d0`` from ``Extended.apply_k`` (input and output times the free
mask) and one step of ``Dynamic_solver.py:12-20`` in increment form,

    d1 = d0 + (dt^2 (lambda f - s) + m (d0 - dn) (1 - alpha dt / 2)) / (m + alpha m dt / 2),        0 on a dof that is not live,

which is the update of ``opstep_update_dof`` with ``m d0`` taken out of numerator and denominator: ``d1 - d0`` and ``d1 - dn`` never
pass through the cancellation that the five energy numbers ``T_{n+1/2}, U_{n+1/2}, U_n, dW, dD`` (``include/saa_hip.h``) would
otherwise inherit.  The same code runs in ``np.float64`` (the stable restatement, with mutants that prove the bar can fail) and
in ``ox.MP`` (mpmath, on 4-element sub-cases).

On a partition (``fem_setup.build_layouts``) one synchronised step gives per rank the local ``d1``, the summed interface buffer
on the rank's free shared dofs (a clamped dof's slot holds the unmasked element sums, which nothing reads), the history row
and the energy share under lowest-holder ownership; one predicted step from a table row (the synchronised ``d1`` of the shared
dofs times ``1 + 1e-3`` plus noise, clamped dofs included) gives ``d1``, the history row and the share with ``U_{n+1/2}`` from the
partial ``s`` on every holder.

Qualification (tests/test_stepper_extended.py, every case): ``env <= 1e-6``, the float64 restatement within ``1e-12 + 2 env``,
and ``max|d1| <= 10 max(|d0|, |dn|)`` in the reference.  No state had to be changed for a case to qualify."""
from __future__ import annotations

import functools

import numpy as np

import operator_extended as ox
from operator_extended import Extended, _sum, conv, scalar, zeros

ALPHA, TN = 0.5, 0.37
STATES = ("random", "smooth")
ENERGY = ("T", "Uh", "Un", "dW", "dD")
VARIANTS = ("base", "alpha0", "alpha2dt", "noramp", "tn1.5")
PARTITIONS = ("slab2", "mod3")
PART_MESHES = ("structured2", "delaunay2", "curved288")
PART_FAMILIES = (("nu", 0.3), ("nu", 0.499999), ("shift", 20), ("sliver", 1e-6))
MUTANTS = ("ramp_late", "dD_half", "owner_ignored", "partial_half")


# ----------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------

def clamped_nodes(points, cells):
    """The nodes on the face of smallest x of the vertices' box (and any node below it)."""
    points = np.asarray(points, dtype=np.float64)
    x = points[:, 0]
    vx = x[np.unique(np.asarray(cells)[:, :4])]
    return np.nonzero(x <= vx.min() + 1e-9 * max(vx.max() - vx.min(), 1e-300))[0]


def omega_bound(points, cells, lmd, mu, rho):
    """An upper bound of ``omega_max(M_L^-1 K)``: the largest element frequency (Irons-Treharne)."""
    cells = np.asarray(cells)
    if cells.shape[1] == 4:
        return float(ox.element_omega(dict(points=points, cells=cells, lmd=lmd, mu=mu, rho=rho)).max())
    import p2_double as p2
    import p2_dynamics_double as dyn

    _, Ke, _ = p2.element_matrices(points, cells, lmd, mu, rho, (0.0, 0.0, 0.0))
    m = np.repeat(dyn.hrz_element_masses(points, cells, rho), 3, axis=1)       # (ne, 30), dof 3 a + i
    s = 1.0 / np.sqrt(m)
    A = Ke * s[:, :, None] * s[:, None, :]
    return float(np.sqrt(np.linalg.eigvalsh(0.5 * (A + np.swapaxes(A, 1, 2)))[:, -1].max()))


def lumped_mass(ext):
    """``(1, 3 n)``: HRZ from the 14-point rule at order 2, ``rho V / 4`` at order 1; one value on a node's three dofs."""
    T = ext.T
    if ext.order == 2:
        I, vol = zeros((ext.n_elems, 10), T), zeros(ext.n_elems, T)
        for q in range(len(ext.wm)):
            I = I + ext.wdm[:, q, None] * (ext.Nm[None, q, :] * ext.Nm[None, q, :])
            vol = vol + ext.wdm[:, q]
        total = zeros(ext.n_elems, T)
        for a in range(10):
            total = total + I[:, a]
        m = (ext.rho * vol / total)[:, None] * I
    else:
        m = (ext.rho * ext.wdk[:, 0] / 4)[:, None] + zeros((ext.n_elems, 4), T)
    return ext._scatter(m[None, :, :, None] + zeros((1, ext.n_elems, ext.na, 3), T))


def make_case(points, cells, lmd, mu, rho, seed, variant="base"):
    """The stepper case on a mesh and material (see the module docstring); ``variant`` one of ``VARIANTS``."""
    import finite_strain_double as fd

    points, cells = np.ascontiguousarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    n = len(points)
    nodes = clamped_nodes(points, cells)
    dirichlet = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    free = np.ones(3 * n)
    free[dirichlet] = 0.0
    ext = Extended(points, cells, lmd, mu, rho)
    assert ext.min_det() > 0
    r64 = lambda v: np.asarray(v, dtype=np.float64)
    mass = r64(lumped_mass(ext)[0])
    load = r64(ext.load(np.array(ox.FORCE))) * free
    dt = 0.9 * 2.0 / omega_bound(points, cells, lmd, mu, rho)
    alpha = {"alpha0": 0.0, "alpha2dt": 2.0 / dt}.get(variant, ALPHA)
    rng = np.random.default_rng(seed)
    d0, dn = np.empty((2, 3 * n)), np.empty((2, 3 * n))
    d0[0], dn[0] = rng.uniform(-0.5, 0.5, size=(2, 3 * n)) * 1e-3
    d0[1] = fd.smooth_random_field(points, seed + 1, 1e-3)
    dn[1] = d0[1] - fd.smooth_random_field(points, seed + 2, 1e-3 * np.abs(d0[1]).max())
    return {"points": points, "cells": cells, "lmd": float(lmd), "mu": float(mu), "rho": float(rho), "clamped": nodes,
            "dirichlet": dirichlet, "free": free, "mass": mass, "load": load, "dt": dt, "alpha": alpha,
            "tn": 1.5 if variant == "tn1.5" else TN, "ramp": variant != "noramp", "d0": d0, "dn": dn, "variant": variant}


def _seed(cid, extra=""):
    return 5000 + sum(ord(c) for c in ox.case_name(cid) + extra)


@functools.lru_cache(maxsize=None)
def build_case(cid, variant="base"):
    c = ox.build_case(cid)
    out = make_case(c["points"], c["cells"], c["lmd"], c["mu"], c["rho"], _seed(cid, variant), variant)
    out["id"] = (cid, variant)
    return out


def sub_case(cid, n_elems=4, variant="base", elements=None):
    """The stepper case on the first ``n_elems`` elements (or on ``elements``) of an ``ox`` case as a mesh of their own."""
    c = ox.build_case(cid)
    cells = c["cells"][:n_elems] if elements is None else c["cells"][np.asarray(elements)]
    _, points, cells = ox.sub_mesh(c["points"], cells, len(cells))
    return make_case(points, cells, c["lmd"], c["mu"], c["rho"], _seed(cid, variant) + len(cells), variant)


def elements_with_node_count(cells, target):
    """Element indices that use exactly ``target`` nodes: the longest prefix of the mesh from which taking every later
    element that still fits, in mesh order or in one of a few seeded orders, ends at the target."""
    cells = np.asarray(cells)
    sets = [set(c.tolist()) for c in cells]
    for prefix in range(len(cells), 0, -1):
        first = set().union(*sets[:prefix])
        if len(first) > target:
            continue
        for seed in range(8):
            rest = np.arange(prefix, len(cells))
            if seed:
                rest = np.random.default_rng(seed).permutation(rest)
            chosen, used = list(range(prefix)), set(first)
            for e in rest:
                if len(used) == target:
                    break
                if len(used | sets[e]) <= target:
                    chosen.append(int(e))
                    used |= sets[e]
            if len(used) == target:
                return np.array(sorted(chosen))
    raise AssertionError(f"no element set with {target} nodes")


def epart_of(name, points, cells):
    cells = np.asarray(cells)
    if name == "mod3":
        return np.arange(len(cells)) % 3, 3
    cx = np.asarray(points)[cells[:, :4], 0].mean(axis=1)
    return (cx > np.median(cx)).astype(np.int64), 2


def add_partition(case, layouts, n_global_shared, seed):
    """``case`` with ``layouts``, ``n_gs``, ``slot_free`` (slot -> one of the node's dofs is free) and the per-rank table rows
    ``tables[r] (2, 3 n_shared_r)`` of the predicted step."""
    out = dict(case)
    out["layouts"], out["n_gs"] = layouts, int(n_global_shared)
    out["slot_free"] = np.zeros(int(n_global_shared), dtype=bool)
    for lay in layouts:
        out["slot_free"][np.asarray(lay.shared_slots, dtype=np.int64)] = \
            case["free"][_global_shared_dofs(lay)].reshape(-1, 3).any(axis=1)
    out["tables"] = [np.zeros((2, 3 * len(lay.shared_local))) for lay in layouts]
    d1 = np.asarray(outputs(out, only="synced")["d1_unmasked"], dtype=np.float64)
    rng = np.random.default_rng(seed)
    row = d1 * (1.0 + 1e-3) + 1e-6 * rng.uniform(-1.0, 1.0, size=d1.shape)
    out["tables"] = [np.ascontiguousarray(row[:, _global_shared_dofs(lay)]) for lay in layouts]
    return out


def _global_shared_dofs(lay):
    g = np.asarray(lay.nodes, dtype=np.int64)[np.asarray(lay.shared_local, dtype=np.int64)]
    return (3 * g[:, None] + np.arange(3)[None, :]).ravel()


@functools.lru_cache(maxsize=None)
def build_partition_case(cid, part):
    from synchronization_avoiding_algorithms_amd import fem_setup as fs

    case = build_case(cid)
    epart, P = epart_of(part, case["points"], case["cells"])
    layouts, gs = fs.build_layouts(case["cells"], epart, P, len(case["points"]), case["clamped"])
    out = add_partition(case, layouts, len(gs), _seed(cid, part))
    out["id"] = (cid, part)
    return out


def fake_shared_case(case, n_shared, n_extra, seed=2):
    """The whole mesh as one rank in which ``n_shared`` nodes (clamped ones among them, in an order that is not node order)
    are declared shared, among ``n_shared + n_extra`` slots: ``n_extra`` are held by nobody."""
    from synchronization_avoiding_algorithms_amd.fem_setup import RankLayout, node_to_dof

    n = len(case["points"])
    rng = np.random.default_rng(seed + n_shared)
    lead = case["clamped"][:1] if n_shared > 1 else case["clamped"][:0]
    rest = np.setdiff1d(np.arange(n), case["clamped"])
    shared = np.concatenate([lead, rng.permutation(rest)[:n_shared - len(lead)]])
    shared = shared[rng.permutation(len(shared))]
    slots = np.sort(rng.permutation(n_shared + n_extra)[:n_shared])
    lay = RankLayout(rank=0, elements=np.arange(len(case["cells"])), nodes=np.arange(n),
                     cells_local=np.asarray(case["cells"], dtype=np.int32), shared_nodes=shared,
                     shared_local=shared.astype(np.int32), shared_slots=slots.astype(np.int32),
                     dirichlet_dofs=case["dirichlet"].astype(np.int32), loc_dof_shared=node_to_dof(shared))
    return add_partition(case, [lay], n_shared + n_extra, seed)


FLOAT_INPUTS = ("points", "lmd", "mu", "rho", "mass", "load", "dt", "alpha", "tn", "d0", "dn")


def perturbed(case, rng):
    """The case with every floating-point input times ``1 + d``, ``d`` uniform in ``+-2^-53``, held in longdouble."""
    def one(v):
        v = np.asarray(v, dtype=np.longdouble)
        d = np.asarray(rng.uniform(-1.0, 1.0, size=v.shape), dtype=np.longdouble) * np.longdouble(2.0) ** -53
        return v * (1 + d)

    out = dict(case)
    for k in FLOAT_INPUTS:
        out[k] = one(case[k])
    if "tables" in case:
        out["tables"] = [one(t) for t in case["tables"]]
    return out


def scaled_case(case, u):
    """Coordinates, ``d0``, ``dn``, table rows and ``dt`` times ``2^(40 u)``, ``lmd`` and ``mu`` times ``4^(10 u)``, ``rho`` times
    ``2^(20 u)``, ``alpha`` times ``2^(-40 u)``, the force density times ``2^(-20 u)`` (the load vector: ``2^(100 u)``; the mass
    vector: ``2^(140 u)``)."""
    L, S, R = 2.0 ** (40 * u), 4.0 ** (10 * u), 2.0 ** (20 * u)
    out = dict(case)
    for k in ("points", "d0", "dn", "dt"):
        out[k] = case[k] * L
    out["lmd"], out["mu"], out["rho"], out["alpha"] = case["lmd"] * S, case["mu"] * S, case["rho"] * R, case["alpha"] / L
    out["mass"], out["load"] = case["mass"] * 2.0 ** (140 * u), case["load"] * 2.0 ** (100 * u)
    if "tables" in case:
        out["tables"] = [t * L for t in case["tables"]]
    return out


def unit_exponent(name):
    """The exponent of 2 per unit ``u`` that an output picks up under :func:`scaled_case`."""
    leaf = name.split(".")[-1]
    return {"mass": 140, "d1": 40, "hist": 40, "iface": 100, "d1_unmasked": 40}.get(leaf, 140)


# ----------------------------------------------------------------------------------------------------------------------
# The reference
# ----------------------------------------------------------------------------------------------------------------------

def _update(s, mass, load, d0, dn, dt, alpha, lam, live):
    """``(d1, d1 - d0)`` of the increment form; ``live`` is 0 / 1 in the arithmetic of the rest."""
    half = alpha * dt / 2
    den = (mass + mass * half) * live + (1 - live)                    # a dof that is not live: never its 0 / 0
    inc = (dt * dt * (lam * load - s) + mass * (d0 - dn) * (1 - half)) / den
    return live * (d0 + inc), inc


def _five(T, mt, hm, nm, s_half, s_now, mass, load, d0, dn, d1, inc, dt, alpha, lam, mutant=None):
    """name -> ``(2, 1)``: the step's sums over the dofs that the 0 / 1 masks ``mt`` (terms with ``m`` or ``f``), ``hm`` (the
    cross form) and ``nm`` (``U_n``) keep."""
    v, w = inc / dt, inc + (d0 - dn)
    damp = alpha / ((2 if mutant == "dD_half" else 4) * dt)
    out = {"T": _sum(mt * mass * (v * v), T) / 2, "Uh": _sum(hm * d1 * s_half, T) / 2, "Un": _sum(nm * d0 * s_now, T) / 2,
           "dW": lam * _sum(mt * load * (w / 2), T), "dD": damp * _sum(mt * mass * (w * w), T)}
    return {k: a.reshape(-1, 1) for k, a in out.items()}


def _live(ext, free, T):
    has = np.zeros(ext.n_nodes)
    has[np.unique(ext.cells)] = 1.0
    return conv(np.repeat(has, 3) * np.asarray(free, dtype=np.float64), T)


def _masked_k(ext, free, d0):
    return free[None, :] * ext.apply_k(free[None, :] * d0)


def outputs(case, T=np.longdouble, mutant=None, only=None):
    """name -> array (columns first) of every output of the case in the arithmetic ``T``.  The whole mesh: ``mass (1, 3 n)``,
    ``d1 (2, 3 n)`` and the five energies ``(2, 1)``.  With layouts, per rank ``r<i>.``: ``d1``, ``iface`` (the summed buffer on
    the rank's free shared dofs), ``hist`` and the five shares of the synchronised step, and ``p.d1``, ``p.hist``, ``p.T`` ... of
    the predicted one."""
    sc = lambda k: scalar(case[k], T)
    dt, alpha, tn = sc("dt"), sc("alpha"), sc("tn")
    late = tn + dt if mutant == "ramp_late" else tn
    lam = (late if late < 1 else scalar(1.0, T)) if case["ramp"] else scalar(1.0, T)
    mass, load, d0, dn = (conv(case[k], T) for k in ("mass", "load", "d0", "dn"))
    free = conv(case["free"], T)
    out = {}
    if only != "synced":
        ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], T)
        live = _live(ext, case["free"], T)
        out["mass"] = lumped_mass(ext)
        s = _masked_k(ext, free, d0)
        d1, inc = _update(s, mass, load, d0, dn, dt, alpha, lam, live)
        out["d1"] = d1
        out.update(_five(T, live, live, live, s, s, mass, load, d0, dn, d1, inc, dt, alpha, lam, mutant))
    if "layouts" not in case:
        return out
    lays, n_gs = case["layouts"], case["n_gs"]
    points = conv(case["points"], T)
    owner = np.full(n_gs, len(lays), dtype=np.int64)
    holders = np.zeros(n_gs, dtype=np.int64)
    for lay in lays:
        slots = np.asarray(lay.shared_slots, dtype=np.int64)
        owner[slots] = np.minimum(owner[slots], int(lay.rank))
        holders[slots] += 1
    if mutant == "owner_ignored":                                      # one three-holder node counts on every holder
        owner[np.nonzero((holders == holders.max()) & case["slot_free"])[0][0]] = -1
    ranks, iface = [], zeros((2, 3 * n_gs), T)
    for lay in lays:
        nodes, dof = np.asarray(lay.nodes, dtype=np.int64), np.asarray(lay.local_dof, dtype=np.int64)
        ext = Extended(points[nodes], lay.cells_local, case["lmd"], case["mu"], case["rho"], T)
        live = _live(ext, case["free"][dof], T)
        loc = np.asarray(lay.loc_dof_shared, dtype=np.int64)
        slots = np.asarray(lay.shared_slots, dtype=np.int64)
        gd = (3 * slots[:, None] + np.arange(3)[None, :]).ravel()
        partial = _masked_k(ext, free[dof], d0[:, dof])
        iface[:, gd] = iface[:, gd] + partial[:, loc]
        own = np.ones(len(dof))
        own[loc] = np.repeat((owner[slots] == int(lay.rank)) | (owner[slots] < 0), 3)
        ranks.append((lay, dof, live, loc, gd, partial, conv(own, T)))
    unmasked = zeros(d0.shape, T)
    for i, (lay, dof, live, loc, gd, partial, own) in enumerate(ranks):
        m, f, x0, xn = mass[dof], load[dof], d0[:, dof], dn[:, dof]
        full = partial.copy()
        full[:, loc] = iface[:, gd]
        d1, inc = _update(full, m, f, x0, xn, dt, alpha, lam, live)
        unmasked[:, dof] = x0 + inc
        if only == "synced":
            continue
        p = f"r{i}."
        out[p + "d1"], out[p + "hist"], out[p + "iface"] = d1, d1[:, loc], iface[:, gd] * free[dof][None, loc]
        mine = live * own
        e = _five(T, mine, mine, live, partial if mutant == "partial_half" else full, partial, m, f, x0, xn, d1, inc, dt, alpha,
                  lam, mutant)
        out.update({p + k: v for k, v in e.items()})
        # predicted: the rank's own partial forces, the table row over the shared dofs, clamped ones included
        table = conv(case["tables"][i], T)
        d1, inc = _update(partial, m, f, x0, xn, dt, alpha, lam, live)
        d1[:, loc], inc[:, loc] = table, table - x0[:, loc]
        out[p + "p.d1"], out[p + "p.hist"] = d1, table
        e = _five(T, mine, live, live, partial, partial, m, f, x0, xn, d1, inc, dt, alpha, lam, mutant)
        out.update({p + "p." + k: v for k, v in e.items()})
    if only == "synced":
        return {"d1_unmasked": unmasked}
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Envelope, bar
# ----------------------------------------------------------------------------------------------------------------------

def envelope(case, seed=79):
    """``(ref, env)``: the longdouble outputs and per output ``env (columns,)`` (0 where the reference's column is 0)."""
    ref = outputs(case)
    rng = np.random.default_rng(seed)
    env = {k: np.zeros(len(v)) for k, v in ref.items()}
    for _ in range(ox.N_DRAWS):
        alt = outputs(perturbed(case, rng))
        for k in env:
            r, a = ox._columns(k, ref[k]), ox._columns(k, alt[k])
            top = np.abs(r).max(axis=1)
            rel = np.abs(a - r).max(axis=1) / np.where(top > 0, top, 1)
            env[k] = np.maximum(env[k], np.asarray(rel, dtype=np.float64))
    return ref, env


@functools.lru_cache(maxsize=None)
def reference(cid, variant="base"):
    """``(case, ref, env)`` of a whole-mesh case."""
    case = build_case(cid, variant)
    return (case,) + envelope(case)


@functools.lru_cache(maxsize=None)
def partition_reference(cid, part):
    case = build_partition_case(cid, part)
    return (case,) + envelope(case)


def check(got, ref, env, factor, label, names=None, verbose=True):
    """``ox.check`` on the columns whose reference is not 0; the others must be exactly 0.  Returns ``(worst, bad)``."""
    names = list(names or [k for k in ref if k in got])
    g2, r2, e2, bad = {}, {}, {}, []
    for name in names:
        r, g = ox._columns(name, ref[name]), ox._columns(name, np.asarray(got[name]))
        assert g.shape == r.shape, (label, name, g.shape, r.shape)
        live = np.asarray(np.abs(r).max(axis=1) > 0)
        if not (np.asarray(g[~live], dtype=np.float64) == 0).all():
            bad.append((name, "not exactly 0 where the reference is"))
        if live.any():
            g2[name], r2[name], e2[name] = g[live], r[live], np.asarray(env[name])[live]
    worst, more = ox.check(g2, r2, e2, factor, label, names=[n for n in names if n in g2], verbose=verbose)
    return worst, bad + more


EDGE_MESHES = ("curved288", "structured2")
EDGE_NODES = (0, 255, 256, 257)                                        # 0: one element
FAKE_SETS = ((1, 1), (1, 100), (85, 1), (85, 100), (86, 1), (86, 100))  # (shared nodes, slots that nobody holds)


@functools.lru_cache(maxsize=None)
def edge_reference(mesh, n_nodes):
    """``(case, ref, env)`` of the sub-mesh of ``(mesh, nu, 0.3)`` with ``n_nodes`` nodes (0: its first element)."""
    cid = (mesh, "nu", 0.3)
    if n_nodes == 0:
        case = sub_case(cid, 1)
    else:
        case = sub_case(cid, elements=elements_with_node_count(ox.build_case(cid)["cells"], n_nodes))
        assert len(case["points"]) == n_nodes
    return (case,) + envelope(case)


@functools.lru_cache(maxsize=None)
def fake_reference(mesh, n_shared, n_extra):
    case = fake_shared_case(build_case((mesh, "nu", 0.3)), n_shared, n_extra)
    assert len(case["layouts"][0].shared_local) == n_shared and case["n_gs"] == n_shared + n_extra
    return (case,) + envelope(case)


def whole_case_keys():
    """Every (cid, variant) of the whole-mesh bar families."""
    out = [(cid, "base") for cid in ox.case_ids()]
    out += [((m, "nu", 0.3), v) for m in ox.MESHES for v in VARIANTS[1:]]
    return out


def partition_keys():
    return [((m, fam, val), part) for m in PART_MESHES for fam, val in PART_FAMILIES for part in PARTITIONS]


def key_name(key):
    return f"{ox.case_name(key[0])}-{key[1]}"
