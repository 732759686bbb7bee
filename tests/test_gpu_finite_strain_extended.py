"""The finite-strain element passes of ``csrc/saa_opfs.hip`` off the moderate-strain unit beam, against the longdouble
reference of tests/finite_strain_double.py on the cases of tests/finite_strain_extended.py.

Families (tests/finite_strain_extended.py builds them, tests/test_finite_strain_extended.py qualifies every one on the CPU):
``max|H|`` from 1e-2 down to 1e-8; ``nu`` up to 0.499999 and -0.3; ``min det F`` down to 1e-3; a rigid rotation of 0.5 rad
plus a strain of 1e-4 and 1e-6; a dilation that keeps ``J^2 - 1`` between 1/16 and 1/4; coordinates shifted by 2^10 and 2^20,
needles, slivers and strongly curved elements at ``max|H|`` 0.3 and 1e-6; on the four meshes of
``finite_strain_double.MESHES`` (<= 288 elements, three of them cross a 256-lane block edge), for ``svk`` and ``neo_hookean``.

The bar, per output (``f`` with and without the energy - the latter is the kernel the stepper launches -, ``energy_elem``):
``err = max|y - r| / max|r| <= 1e-12 + 8 env``, as tests/test_gpu_operator_extended.py.  Each test prints ``err``, ``env`` and
``err / env``.  Units: no bar, bitwise.  The neo-Hooke pass as it was first written (``P = mu F + ((lam ln J - mu)/J) cof F``
from ``F = I + H``) fails this file at every ``max|H| <= 1e-4`` in ``energy_elem`` and at ``<= 1e-6`` in ``f``.

Also here: an order-2 element inverted at some of its Gauss points only, a NaN displacement, and the stepper at the default
load of the drivers, where the strain is 1e-4 and less."""
import numpy as np
import pytest

from conftest import rel_l2

import finite_strain_double as fd
import finite_strain_extended as fx
import operator_extended as ox

pytestmark = pytest.mark.gpu

LMD, MU = fd.lame(fd.E, fd.NU)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(t):
    return t.cpu().numpy()


def _operator(case):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(case["points"], case["cells"].astype(np.int32), case["dd"].astype(np.int32), case["lmd"], case["mu"],
                         fd.RHO)


def gpu_outputs(case, material):
    """``({"f", "energy_elem", "f_plain"}, n_inverted)``: with the energy, and ``f`` of the ``ENERGY = false`` kernel."""
    with _operator(case) as op:
        u = _dev(case["u"])
        f, en, n_inv = op.internal_force(u, material, energy=True)
        plain = op.internal_force(u, material)
        return {"f": _host(f), "energy_elem": _host(en), "f_plain": _host(plain)}, n_inv


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", fx.case_ids(), ids=fx.case_name)
def test_force_and_energy_are_within_the_bar(cid, material):
    case, ref, env, info = fx.reference(cid)
    assert not info["inverted"][material].any()
    got, n_inv = gpu_outputs(case, material)
    assert n_inv == 0                                                 # (neo-Hooke: nothing is inverted; svk never counts)
    label = f"{fx.case_name(cid)} {material}"
    _, bad = fx.check(got, cid, material, ox.KERNEL_FACTOR, label)
    _, bad_plain = fx.check({"f": got["f_plain"]}, cid, material, ox.KERNEL_FACTOR, label + " plain", names=("f",))
    assert not bad and not bad_plain, (bad, bad_plain)
    assert not got["f"][case["dd"]].any() and not got["f_plain"][case["dd"]].any()


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", fx.unit_cases(), ids=fx.case_name)
def test_power_of_two_units_commute_bitwise(cid, material, u):
    import torch

    case = fx.build_case(cid)
    scaled = fx.scaled_case(case, u)
    ref = fx.outputs(scaled, material)[0]                             # no overflow or underflow in the reference first
    for name, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        assert np.isfinite(r).all() and (np.abs(r[r != 0]) > 1e-290).all() and np.abs(r).max() < 1e290, name
    (base, n0), (got, n1) = gpu_outputs(case, material), gpu_outputs(scaled, material)
    assert n0 == 0 and n1 == 0
    differ = []
    for name in ("f", "energy_elem", "f_plain"):
        want = torch.from_numpy(base[name]) * 2.0 ** (u * fx.UNIT_EXPONENT[name.split("_plain")[0]])
        if not torch.equal(torch.from_numpy(got[name]), want):
            differ.append((name, int((got[name] != want.numpy()).sum())))
    print(fx.case_name(cid), material, u, "outputs that differ:", differ)
    assert not differ, differ


# ---- an element inverted at some of its points only ---------------------------------------------------------------------------

def test_an_element_inverted_at_some_points_only_is_dropped_whole_and_counted_once():
    """``curved288``, one vertex moved alone on a gentle background: in the double six elements have ``det F > 0`` at three
    Gauss points and ``< 0`` at the fourth (``|det F| >= 1e-3`` everywhere, so no rounding decides a sign).  The kernel counts
    each once, gives it the energy 0, and ``f`` is the double's with those elements dropped, to the bar; one such element as a
    mesh of its own (30 dofs, ``f`` IS its 30 contributions) gives 30 zeros."""
    import torch

    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    pts, cells, dd = fd.mesh("curved288")
    fs = fd.FiniteStrain(pts, cells, LMD, MU, dd)
    u, partial = fx.partial_inversion_state(fs, pts, 0.02 * fd.smooth_random_field(pts, 3))
    want_f, want_e, inv = fs.evaluate(u, "neo_hookean")
    det = np.asarray(fs.det_f(u), dtype=np.float64)
    assert len(partial) >= 1 and inv[partial].all() and (det[partial] > 0).any(axis=1).all() and (det[partial] <= 0).any(axis=1).all()
    assert 0 < inv.sum() < len(cells) and float(np.abs(want_f).max()) > 1.0
    case = {"points": pts, "cells": cells, "dd": dd, "lmd": LMD, "mu": MU, "u": u}
    rng = np.random.default_rng(77)
    env = {"f": np.zeros(1), "energy_elem": np.zeros(1)}
    ref = {"f": want_f[None], "energy_elem": want_e[None]}
    for _ in range(ox.N_DRAWS):
        alt, alt_inv, _ = fx.outputs(fx.perturbed(case, rng), "neo_hookean")
        assert (alt_inv == inv).all()
        for k in env:
            env[k] = np.maximum(env[k], float(np.abs(alt[k] - ref[k]).max() / np.abs(ref[k]).max()))
    got, n_inv = gpu_outputs(case, "neo_hookean")
    print("partially inverted", list(partial), "inverted in all", int(inv.sum()), "n_inverted", n_inv)
    assert n_inv == int(inv.sum())                                    # once per element, not once per point
    assert not got["energy_elem"][inv].any() and np.isfinite(got["f"]).all() and np.isfinite(got["energy_elem"]).all()
    _, bad = ox.check({k: got[k][None] for k in env}, ref, env, ox.KERNEL_FACTOR, "curved288 partial inversion", names=list(env))
    _, bad_plain = ox.check({"f": got["f_plain"][None]}, ref, env, ox.KERNEL_FACTOR, "curved288 partial inversion plain", names=["f"])
    assert not bad and not bad_plain, (bad, bad_plain)
    e = int(partial[0])                                               # the element alone: its ten nodes, no Dirichlet dofs
    nodes = cells[e]
    dof = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    with ModalOperator(pts[nodes], np.arange(10, dtype=np.int32)[None], np.zeros(0, dtype=np.int32), LMD, MU, fd.RHO) as op:
        for energy in (True, False):
            out = op.internal_force(_dev(u[dof]), "neo_hookean", energy=energy)
            f = out[0] if energy else out
            assert f.numel() == 30 and not bool(f.any().item()), f    # every one of the 30 contributions is 0
            if energy:
                assert float(out[1][0]) == 0.0 and out[2] == 1
        f_svk = op.internal_force(_dev(u[dof]), "svk")                # St. Venant-Kirchhoff does not look at J
        assert bool(torch.isfinite(f_svk).all()) and float(f_svk.abs().max()) > 0.0


# ---- NaN ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_a_nan_displacement_drops_the_elements_around_the_node_under_neo_hooke(name):
    """The "NaN included" clause of the inversion rule: one free vertex's displacement is NaN.  Every element that holds the
    node is dropped and counted, ``f`` and ``energy_elem`` are finite everywhere and are the double's with those elements
    removed, to the bar (the envelope of the elements that are left).  St. Venant-Kirchhoff has no such rule: its NaNs
    propagate by design and it is only asserted to return."""
    pts, cells, dd = fd.mesh(name)
    fs = fd.FiniteStrain(pts, cells, LMD, MU, dd)
    node = next(int(v) for v in np.unique(cells[:, :4])[::-1] if fs.free[3 * v:3 * v + 3].all())
    star = (cells == node).any(axis=1)
    u = 0.05 * fd.smooth_random_field(pts, 11)
    u[3 * node:3 * node + 3] = np.nan
    want_f, want_e, inv = fs.evaluate(u, "neo_hookean")
    assert (inv == star).all() and 0 < star.sum() < len(cells)
    assert np.isfinite(np.asarray(want_f, dtype=np.float64)).all() and np.isfinite(np.asarray(want_e, dtype=np.float64)).all()
    keep = np.nonzero(~star)[0]                                       # the envelope: the mesh without the star, NaN set to 0
    u0 = np.where(np.isnan(u), 0.0, u)
    rest = {"points": pts, "cells": cells[keep], "dd": dd, "lmd": LMD, "mu": MU, "u": u0}
    base = fx.outputs(rest, "neo_hookean")[0]
    assert float(np.abs(base["f"][0] - want_f).max()) <= 1e-17 * float(np.abs(want_f).max())
    rng = np.random.default_rng(77)
    env = {"f": np.zeros(1), "energy_elem": np.zeros(1)}
    for _ in range(ox.N_DRAWS):
        alt = fx.outputs(fx.perturbed(rest, rng), "neo_hookean")[0]
        for k in env:
            env[k] = np.maximum(env[k], float(np.abs(alt[k] - base[k]).max() / np.abs(base[k]).max()))
    case = {"points": pts, "cells": cells, "dd": dd, "lmd": LMD, "mu": MU, "u": u}
    got, n_inv = gpu_outputs(case, "neo_hookean")
    print(name, "node", node, "elements around it", int(star.sum()), "n_inverted", n_inv)
    assert n_inv == int(star.sum())
    for k in ("f", "energy_elem", "f_plain"):
        assert np.isfinite(got[k]).all(), k
    assert not got["energy_elem"][star].any()
    ref = {"f": want_f[None], "energy_elem": want_e[None]}
    _, bad = ox.check({k: got[k][None] for k in env}, ref, env, ox.KERNEL_FACTOR, f"{name} NaN", names=list(env))
    _, bad_plain = ox.check({"f": got["f_plain"][None]}, ref, env, ox.KERNEL_FACTOR, f"{name} NaN plain", names=["f"])
    assert not bad and not bad_plain, (bad, bad_plain)
    svk, n_svk = gpu_outputs(case, "svk")
    assert n_svk == 0 and svk["f"].shape == want_f.shape


# ---- the stepper at the default load: a strain of 1e-4 and less ---------------------------------------------------------------

# rel-L2 between the neo-Hooke and the linear run after 200 steps over max|H| of the final state, measured with the double's two
# float64 loops on the CPU (exact omega_max of the linear operator): 0.52 at order 1 (max|H| 1.4e-4, difference 7.5e-5) and
# 0.32 at order 2 (max|H| 3.3e-5, difference 1.1e-5); the test allows 4 times that
NONLINEAR_OVER_STRAIN = {1: 4 * 0.52, 2: 4 * 0.32}


@pytest.mark.parametrize("order,name", ((1, "structured288"), (2, "curved288")))
def test_small_strain_stepper_against_the_double(order, name):
    """``neo_hookean`` under the reference load ``(0, -fz, -fz)``, ``fz = 0.5``, the default of the drivers: from rest, ramp off,
    ``alpha = 0.5``, 200 steps at ``dt = 0.9 * 2/omega_max``, against the double's float64 loop on the stable force: rel-L2 <
    1e-11, the project's short-run bar.  The strain stays at 1e-4 and less, where the first kernel's force carried an error of
    ``eps/|H|``.  And the material hardly matters there: the linear stepper ends within ``NONLINEAR_OVER_STRAIN`` times
    ``max|H|`` of the final state (measured on the CPU: 0.52 and 0.32 times, see above)."""
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    pts, cells, dd = fd.mesh(name)
    f64 = fd.FiniteStrain(pts, cells, LMD, MU, dd, T=np.float64)
    live = f64.free.copy()
    live[np.repeat(np.bincount(cells.ravel(), minlength=len(pts)) == 0, 3)] = False
    runs = {}
    with ModalOperator(pts, cells.astype(np.int32), dd.astype(np.int32), LMD, MU, fd.RHO) as op:
        mass, load = op.lumped_mass(), op.load((0.0, -0.5, -0.5))
        dt = stable_time_step_operator(op, mass, 0.9)["dt"]
        for material in ("neo_hookean", "linear"):
            with OperatorStepper(op, mass, load, dt, 0.5, ramp=False, material=material) as st:
                st.step(200)
                d0, dn, _ = st.state()
                runs[material] = (_host(d0), _host(dn), st.inverted())
        mass, load = _host(mass), _host(load)
    want = fd.run(lambda x: f64.force(x, "neo_hookean"), mass, load, live, dt, 0.5, False, 200)
    d0, dn, inverted = runs["neo_hookean"]
    e0, en = rel_l2(d0, want[0]), rel_l2(dn, want[1])
    hmax = float(np.abs(f64.gradient(d0)).max())
    apart = rel_l2(runs["linear"][0], d0)
    print(f"order {order} neo_hookean at fz = 0.5: 200 steps from rest, d0 {e0:.2e} dn {en:.2e}; max|H| {hmax:.2e}, the linear "
          f"stepper differs by {apart:.2e} = {apart / hmax:.2f} max|H|; inverted {inverted}")
    assert inverted == (0, -1) and 1e-6 < hmax < 1e-3
    assert e0 < 1e-11 and en < 1e-11
    assert apart <= NONLINEAR_OVER_STRAIN[order] * hmax
