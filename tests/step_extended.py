"""Extended-precision reference of the production step kernels (``csrc/saa_kernels.hip``: ``fused_step_kernel`` plain and
``FORCE_ONLY``, ``persistent_steps_kernel`` = the resident kernel, ``det_items_kernel`` / ``det_nodes_kernel``,
``iface_finish_kernel``, ``halo_overwrite_kernel``) and of the set-up kernels (``csrc/saa_setup.hip``), the cases that take them
off the unit beam, and the bar they are held to.  Shared by tests/test_step_extended.py (CPU) and
tests/test_gpu_step_extended.py.  Lives under tests/: the product never imports it.

Cases, arithmetic and the bar are those of tests/operator_extended.py (``ox``) and tests/stepper_extended.py (``sx``): ``err =
max|y - r| / max|r| <= 1e-12 + 8 env`` per output column (here: per step and state), ``env`` the largest relative change of
the longdouble reference over 8 draws of ``sx.perturbed``.  The step kernels are order 1 only: the 20 ids of ``ox.case_ids()``
on ``ox.MESHES_P1``, and at ``nu = 0.3`` the variants of ``sx.VARIANTS`` plus ``cross1``, whose ``tn = 1 - 3.5 dt`` lets the load
ramp reach 1 after the fourth step of an 8-step resident launch (half a step away from the kink on either side).

A case is ``sx.build_case(cid, variant)`` with three changes, so that it is what ``HipExplicitSolver`` takes and still runs
resident:

* ``load`` is the reference's consistent load of the force density ``(0, -0.5, -0.5)`` rounded to float64, times ``free``.  Every
  x entry is ``+0`` and ``y == z`` bitwise on every node, and the mass is equal on a node's three dofs (asserted): the compact
  per-node forms of ``refresh_nodal_mass`` / ``refresh_nodal_load`` (``saa_api.cpp``) stay in force.
* ``d0`` and ``dn`` are multiplied by ``free``.  The production rule is ``d1[dirichlet] = 0`` with an UNMASKED ``K``
  (``oracle/fem_oracle.py: cd_update``); with the clamped dofs at zero it coincides with ``sx``'s masked increment form.
* ``cross1`` only: ``tn``.

The reference is ``n`` steps of ``sx.outputs(...)["d1"]`` (the masked ``K`` of ``Extended.apply_k``, ``sx._update``, built once per
trajectory instead of once per step: tests/test_step_extended.py asserts that step 1 IS ``sx.outputs(case)["d1"]``), rotating
``(d0, dn, tn)``, in ``np.longdouble`` and in ``ox.MP`` on 4-element sub-cases.  :func:`restatement` runs the same steps in
float64 with the production association ``(dt**2*(F*ramp - f) + 2*m*d0 - m*dn + dt/2*m*alpha*dn) / (m + 0.5*alpha*m*dt)`` on
the unmasked float64 ``K d0``, and carries the four mutants that prove the bar can fail:

* ``rcp32``: ``1 / detJ`` rounded to float32 (the reciprocal seed of ``tet_core`` without its Newton step);
* ``halo_stale``: one free dof read one step old in the force of step 4 of 8 (the middle free dof: which dofs are halo dofs
  depends on the plan, and every free dof is one under some plan);
* ``ramp_late``: the ramp read one step late;
* ``ramp_unclamped``: ``cross1`` with the ramp not clamped at 1.

Partitions (``sx.PART_FAMILIES`` x ``sx.PARTITIONS`` on both meshes): ``sx.build_partition_case``'s layouts around the case above,
the table rows made by ``sx.add_partition`` from it.  Of ``sx.outputs`` per rank the production solver has ``d1``, ``iface`` (the
summed buffer on the rank's free shared dofs), ``hist``, and of the predicted step ``p.d1``, ``p.hist``; it has no energies.  On a
clamped shared dof the production rule (``fem_oracle.explicit_step_synced`` / ``run_hybrid``) and ``sx.outputs`` agree in every
one of these: a synchronised step gives ``d1 = 0`` and history 0, the interface slot holds the unmasked element sums that
nothing reads (compared on free dofs only), and a predicted step writes the table row over every shared dof, clamped ones
included, into the state and the history.  They differ only in what they compute on the way (``K`` unmasked against masked),
which the clamped zeros of ``d0`` make the same numbers.

Set-up fields (``fem_setup.device_setup_fields``): ``sx.lumped_mass``, the consistent load of ``(0, -fz, -fz)`` and the shortest edge
(longdouble ``sqrt`` of the least squared edge), ``env`` from ``sx.perturbed`` and one more draw for ``fz``.

Plans: A ``block_nodes=0, threads=64`` (one wave per workgroup: the LDS adds run in program order, resident and fused kernels
must agree bitwise), B ``block_nodes=24, threads=0``.  Both are multi-block on every case, with halo nodes on every block,
paired and single items (:func:`plan_facts`, asserted on the CPU)."""
from __future__ import annotations

import functools

import numpy as np

import operator_extended as ox
import stepper_extended as sx
from operator_extended import Extended, conv, scalar, sqrt

N_STEPS = 8                                                            # kPersistMinSteps: the fewest steps that run resident
FZ = 0.5
VARIANTS = sx.VARIANTS + ("cross1",)
PLANS = {"A": dict(block_nodes=0, threads=64), "B": dict(block_nodes=24, threads=0)}
MUTANTS = ("rcp32", "halo_stale", "ramp_late", "ramp_unclamped")
STALE_STEP = 3                                                         # index of step 4 of 8
GROWTH_MAX = 16.0
RANK_OUTPUTS = ("d1", "iface", "hist", "p.d1", "p.hist")
# ``sx.scaled_case`` scales ``dt`` by 2^(40 u) and leaves ``tn`` and the ramp's 1 alone: the unit of time changes under a ramp that
# does not.  One step reads the ramp before the clock moves and commutes on ``base``; 8 steps commute where the ramp is off
# (``noramp``) or stays at 1 whatever ``dt`` is (``tn1.5``: 1.5 + 8 * 2^40 dt > 1, and 1.5 + 2^-40 dt rounds to 1.5)
UNIT_RUNS = (("base", 1), ("noramp", N_STEPS), ("tn1.5", N_STEPS))


# ----------------------------------------------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------------------------------------------

def case_ids():
    return [cid for cid in ox.case_ids() if cid[0] in ox.MESHES_P1]


def case_keys():
    """Every (cid, variant): the 20 ids at ``base`` and the variants at ``nu = 0.3``."""
    return [(cid, "base") for cid in case_ids()] + [((m, "nu", 0.3), v) for m in ox.MESHES_P1 for v in VARIANTS[1:]]


def partition_keys():
    return [((m, fam, val), part) for m in ox.MESHES_P1 for fam, val in sx.PART_FAMILIES for part in sx.PARTITIONS]


key_name = sx.key_name


def yz_load(points, cells, lmd, mu, rho, fz=FZ, T=np.longdouble):
    """The consistent load of the force density ``(0, -fz, -fz)`` in ``T``."""
    fz = scalar(fz, T)
    return Extended(points, cells, lmd, mu, rho, T).load(np.array([scalar(0.0, T), -fz, -fz]))


def compact_forms(case):
    """The predicates of ``refresh_nodal_load`` and ``refresh_nodal_mass``: x ``+0`` and ``y == z``; one mass per node."""
    f, m = case["load"].reshape(-1, 3), case["mass"].reshape(-1, 3)
    load = bool((f[:, 0] == 0).all() and not np.signbit(f[:, 0]).any() and np.array_equal(f[:, 1], f[:, 2]))
    return load, bool(np.array_equal(m[:, 0], m[:, 1]) and np.array_equal(m[:, 0], m[:, 2]))


def adapt(case, variant):
    """The three changes of the module docstring on a case of ``sx``."""
    out = dict(case)
    load = np.asarray(yz_load(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"]), dtype=np.float64)
    out["load"] = load * case["free"]
    out["d0"], out["dn"] = case["d0"] * case["free"][None, :], case["dn"] * case["free"][None, :]
    if variant == "cross1":
        out["tn"] = 1.0 - 3.5 * case["dt"]
    out["variant"] = variant
    assert compact_forms(out) == (True, True), compact_forms(out)
    return out


@functools.lru_cache(maxsize=None)
def build_case(cid, variant="base"):
    out = adapt(sx.build_case(cid, variant), variant)
    out["id"] = (cid, variant)
    return out


def sub_case(cid, variant="base", n_elems=4):
    return adapt(sx.sub_case(cid, n_elems, variant), variant)


@functools.lru_cache(maxsize=None)
def build_partition_case(cid, part):
    theirs = sx.build_partition_case(cid, part)
    out = sx.add_partition(build_case(cid), theirs["layouts"], theirs["n_gs"], sx._seed(cid, part))
    out["id"] = (cid, part)
    return out


def stale_dof(case):
    """The y dof of the first free corner of the element with the smallest ``detJ``: where one stale value weighs most."""
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], np.float64)
    for node in case["cells"][int(np.argmin(ext.detk[:, 0]))]:
        if case["free"][3 * int(node) + 1]:
            return 3 * int(node) + 1
    raise AssertionError("the smallest element is clamped at every corner")


def growth(case, ref):
    """``max|d|`` over the steps and both states by ``max(|d0|, |dn|)`` over both states."""
    return float(np.abs(ref).max() / max(np.abs(case["d0"]).max(), np.abs(case["dn"]).max()))


# mutant -> the cases (``key_name``) on which it stays under the bar, and why (tests/test_step_extended.py asserts the list
# both ways: every case named here is missed by nothing, every other case the mutant applies to misses)
_SMALL_DT = [f"{m}-{fam}-base" for m in ox.MESHES_P1 for fam in ("nu-0.499999", "needle-0.001", "sliver-1e-06")]
BLIND = {
    # structured_beam(2) off the slivers: every 1 / detJ is a float32 up to 2^-50 (1 / 64 000 on the needle; asserted)
    "rcp32": [key_name(k) for k in case_keys() if k[0][0] == "structured2" and k[0][1] != "sliver"],
    "halo_stale": [],
    # dt^2 * load * dt against m d: below the bar where dt is set by a bulk modulus, a needle or a sliver
    "ramp_late": _SMALL_DT + ["delaunay2-nu-0.4999-base"],
    "ramp_unclamped": [],
}


# ----------------------------------------------------------------------------------------------------------------------
# The reference, the restatement
# ----------------------------------------------------------------------------------------------------------------------

def trajectory(case, T=np.longdouble, n=N_STEPS):
    """``(d (n, 2, 3 n_nodes), tn after every step)``: ``n`` steps of ``sx.outputs(...)["d1"]`` in the arithmetic ``T``."""
    sc = lambda k: scalar(case[k], T)
    dt, alpha, tn, one = sc("dt"), sc("alpha"), sc("tn"), scalar(1.0, T)
    mass, load, d0, dn, free = (conv(case[k], T) for k in ("mass", "load", "d0", "dn", "free"))
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], T)
    live = sx._live(ext, case["free"], T)
    out, tns = [], []
    for _ in range(n):
        lam = (tn if tn < 1 else one) if case["ramp"] else one
        d1, _ = sx._update(sx._masked_k(ext, free, d0), mass, load, d0, dn, dt, alpha, lam, live)
        dn, d0, tn = d0, d1, tn + dt
        out.append(d1)
        tns.append(tn)
    return np.stack(out), tns


def restatement(case, n=N_STEPS, mutant=None):
    """The same steps in float64 as the production kernels state them: the unmasked ``K d0``, the reference's association of
    the update, ``d1[dirichlet] = 0``, ``tn`` the repeated sum.  ``mutant``: one of ``MUTANTS``."""
    dt, alpha, tn = float(case["dt"]), float(case["alpha"]), float(case["tn"])
    m, F = np.asarray(case["mass"])[None, :], np.asarray(case["load"])[None, :]
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], np.float64)
    if mutant == "rcp32":                                              # grad N = adj J * fl32(1 / detJ)
        r32 = np.asarray(np.asarray(1.0 / ext.detk, dtype=np.float32), dtype=np.float64)
        ext.grad = ext.grad * (ext.detk * r32)[:, :, None, None]
    d0, dn = np.array(case["d0"], dtype=np.float64), np.array(case["dn"], dtype=np.float64)
    out, tns = [], []
    for k in range(n):
        t = tn + dt if mutant == "ramp_late" else tn
        ramp = (t if (t <= 1 or mutant == "ramp_unclamped") else 1.0) if case["ramp"] else 1.0
        seen = d0
        if mutant == "halo_stale" and k == STALE_STEP:
            seen = d0.copy()
            seen[:, stale_dof(case)] = dn[:, stale_dof(case)]
        f = ext.apply_k(seen)
        d1 = (dt ** 2 * (F * ramp - f) + 2 * m * d0 - m * dn + dt / 2 * m * alpha * dn) / (m + 0.5 * alpha * m * dt)
        d1[:, case["dirichlet"]] = 0
        dn, d0, tn = d0, d1, tn + dt
        out.append(d1)
        tns.append(tn)
    return np.stack(out), tns


def _rel_change(alt, ref, axis):
    top = np.abs(ref).max(axis=axis)
    return np.asarray(np.abs(alt - ref).max(axis=axis) / np.where(top > 0, top, 1), dtype=np.float64)


def envelope(case, seed=83):
    """``(ref (n, 2, 3 n_nodes) longdouble, env (n, 2))``: per step and state."""
    ref, _ = trajectory(case)
    rng = np.random.default_rng(seed)
    env = np.zeros(ref.shape[:2])
    for _ in range(ox.N_DRAWS):
        env = np.maximum(env, _rel_change(trajectory(sx.perturbed(case, rng))[0], ref, 2))
    return ref, env


@functools.lru_cache(maxsize=None)
def reference(cid, variant="base"):
    case = build_case(cid, variant)
    return (case,) + envelope(case)


def errors(got, ref):
    """``err`` per column of ``got (..., 3 n)`` against a reference of the same shape, the difference in longdouble."""
    got = np.asarray(got, dtype=np.longdouble)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return _rel_change(got, ref, -1)


def hold(got, ref, env, factor, label, steps=None, verbose=True):
    """Hold ``got (..., 3 n)`` to ``1e-12 + factor env`` per column (a trajectory: per step and state; ``steps`` picks the steps
    of the reference that ``got`` holds).  Prints the worst column's ``err``, ``env`` and ``err / env`` (``verbose``); returns ``(its
    err, its env, its err / bar, the columns that miss)``, a column named by its index, first entry counted from 1."""
    if steps is not None:
        ref, env = ref[list(steps)], env[list(steps)]
    first = list(steps) if steps is not None else list(range(len(ref)))
    err, e = errors(got, ref), np.asarray(env)
    ratio = err / (ox.TOL + factor * e)
    at = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
    name = lambda idx: (first[idx[0]] + 1,) + tuple(int(i) for i in idx[1:])
    if verbose:
        print(f"{label:60s} worst at {str(name(at)):8s} err {err[at]:.2e}  env {e[at]:.2e}  err/env {err[at] / max(e[at], 1e-300):.2e}  "
              f"err/bar {ratio[at]:.3g}")
    bad = [name(idx) + (float(err[idx]), float(e[idx])) for idx in zip(*np.nonzero(~(ratio <= 1)))]
    return float(err[at]), float(e[at]), float(ratio[at]), bad


# ----------------------------------------------------------------------------------------------------------------------
# K X on the five columns of ``ox``; the set-up fields; partitions
# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def force_reference(cid):
    """``(ox case, K X (5, 3 n) longdouble, env (5,))``: the unmasked ``Extended.apply_k`` on the columns ``X`` of the ``ox`` case."""
    case = ox.build_case(cid)
    kx = lambda c: Extended(c["points"], c["cells"], c["lmd"], c["mu"], c["rho"]).apply_k(c["X"])
    ref = kx(case)
    rng = np.random.default_rng(84)
    env = np.zeros(len(ref))
    for _ in range(ox.N_DRAWS):
        env = np.maximum(env, _rel_change(kx(ox.perturbed(case, rng)), ref, 1))
    return case, ref, env


def setup_outputs(case, T=np.longdouble, fz=FZ):
    """name -> ``(1, .)``: what ``device_setup_fields`` returns, in the arithmetic ``T``."""
    ext = Extended(case["points"], case["cells"], case["lmd"], case["mu"], case["rho"], T)
    P = conv(case["points"], T)[ext.cells]
    least = None
    for a in range(4):
        for b in range(a):
            d = P[:, a] - P[:, b]
            sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).min()
            least = sq if least is None or sq < least else least
    edge = np.empty((1, 1), dtype=object if T is ox.MP else T)
    edge[0, 0] = sqrt(np.array([least]), T)[0]
    fz = scalar(fz, T)
    return {"mass": sx.lumped_mass(ext), "load": ext.load(np.array([scalar(0.0, T), -fz, -fz]))[None], "edge": edge}


@functools.lru_cache(maxsize=None)
def setup_reference(cid):
    case = build_case(cid)
    ref = setup_outputs(case)
    rng = np.random.default_rng(85)
    env = {k: np.zeros(1) for k in ref}
    for _ in range(ox.N_DRAWS):
        fz = np.longdouble(FZ) * (1 + np.longdouble(rng.uniform(-1.0, 1.0)) * np.longdouble(2.0) ** -53)
        alt = setup_outputs(sx.perturbed(case, rng), fz=fz)
        for k in env:
            env[k] = np.maximum(env[k], _rel_change(alt[k], ref[k], 1))
    return case, ref, env


def rank_names(case):
    return [f"r{i}.{k}" for i in range(len(case["layouts"])) for k in RANK_OUTPUTS]


@functools.lru_cache(maxsize=None)
def partition_reference(cid, part):
    """``(case, ref, env)`` of ``sx.envelope`` on the partition case, cut down to the outputs the production solver has."""
    case = build_partition_case(cid, part)
    ref, env = sx.envelope(case)
    names = rank_names(case)
    return case, {k: ref[k] for k in names}, {k: env[k] for k in names}


# ----------------------------------------------------------------------------------------------------------------------
# Plans
# ----------------------------------------------------------------------------------------------------------------------

def plan_facts(case, plan):
    """``plan_host_stats`` and ``plan_host_block_maxima`` of the case under a plan, with ``check`` = ``plan_host_check``.  No GPU."""
    from synchronization_avoiding_algorithms_amd.solver import plan_host_block_maxima, plan_host_check, plan_host_stats

    bn = PLANS[plan]["block_nodes"]
    out = dict(plan_host_stats(case["points"], case["cells"], bn))
    out.update(plan_host_block_maxima(case["points"], case["cells"], bn))
    out["check"] = plan_host_check(case["points"], case["cells"], bn)
    return out


def plan_is_rich(facts):
    """More than one block, a halo on every block, paired items and single items, a sound plan."""
    return (facts["n_blocks"] > 1 and facts["min_halo"] > 0 and facts["n_pairs"] > 0 and facts["n_items"] > facts["n_pairs"]
            and facts["check"] == 0)
