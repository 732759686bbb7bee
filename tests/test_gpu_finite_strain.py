"""Finite-strain materials on the operator handle on the GPU: ``saa_operator_internal_force``,
``saa_operator_stepper_set_material`` / ``_inverted`` and everything above them, against the NumPy double of
tests/finite_strain_double.py (longdouble for forces and energies, float64 for the time loop).

Shapes: ``structured_beam(2, length=6.0)`` (288 tets = 256 + 32, 117 nodes) and ``delaunay_beam(2)`` at order 1, the 36-tet
beam (one block) and the curved 288-tet / 625-node fixture at order 2: the smallest that cross a block edge of the 256-lane
passes.  Bars: 1e-12 of the largest entry for one evaluation against the longdouble double (the project's bar for operator
outputs), rel-L2 < 1e-11 for states after 200 steps (the project's short-run bar), bitwise wherever the same kernels run on
the same data."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel_l2

import finite_strain_double as fd

pytestmark = pytest.mark.gpu

LMD, MU = fd.lame(fd.E, fd.NU)
ORDER_MESH = {1: "structured288", 2: "curved288"}
TOL = 1e-12


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _np(t):
    return t.cpu().numpy()


def _err(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - want).max() / np.abs(want).max())


def _op(pts, cells, dd):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(pts, cells.astype(np.int32), np.asarray(dd, dtype=np.int32), LMD, MU, fd.RHO)


@pytest.fixture(scope="module")
def meshes():
    """name -> dict(pts, cells, dd, fs: the clamped longdouble double, free: the same without Dirichlet dofs)."""
    out = {}
    for name in fd.MESHES:
        pts, cells, dd = fd.mesh(name)
        out[name] = {"pts": pts, "cells": cells, "dd": dd, "fs": fd.FiniteStrain(pts, cells, LMD, MU, dd),
                     "free": fd.FiniteStrain(pts, cells, LMD, MU, ())}
    return out


# ---- 1. one evaluation against the double ---------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("k,name", list(enumerate(fd.MESHES)))
def test_internal_force_against_the_double(meshes, k, name, material):
    """A seeded smooth-plus-random field scaled to ``max|H| = 0.3`` (``min det F`` 0.55 .. 0.71).  Measured on the MI355X, of
    the largest entry: ``f`` 1.7e-16 .. 1.8e-15 (svk), 2.3e-16 .. 1.6e-15 (neo_hookean), the same with and without the energy;
    ``energy_elem`` 2.6e-16 .. 1.8e-15 (svk), 6.2e-16 .. 9.2e-16 (neo_hookean)."""
    import torch

    m = meshes[name]
    u, det, hmax = fd.scale_to_strain(m["fs"], fd.smooth_random_field(m["pts"], 40 + k))
    assert det >= 0.2 and hmax >= 0.1, (det, hmax)
    want_f, want_e, inv = m["fs"].evaluate(u, material)
    assert not inv.any()
    with _op(m["pts"], m["cells"], m["dd"]) as op:
        f, en, n_inv = op.internal_force(_dev(u), material, energy=True)
        plain = op.internal_force(_dev(u), material)                  # ENERGY = false: the kernel the stepper launches
    ef, ee, ep = _err(_np(f), want_f), _err(_np(en), want_e), _err(_np(plain), want_f)
    print(name, material, f"min det F {det:.3f} max|H| {hmax:.3f}: f {ef:.2e} (without energy {ep:.2e}) energy_elem {ee:.2e}",
          "n_inverted", n_inv)
    assert n_inv == 0
    assert ef <= TOL and ep <= TOL and ee <= TOL
    assert not _np(f)[m["dd"]].any() and bool(torch.isfinite(f).all())


# ---- 2. rigid motion --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_rigid_motion_gives_no_force_where_the_linear_operator_gives_a_load(meshes, name, material):
    """The test that cannot pass without the feature: ``u = (R - I) X + c``, 0.5 rad.  Measured on the MI355X:
    ``max|f_fs| / max|K u|`` 4.7e-15 .. 3.3e-14 over the four meshes and both materials, with ``max|K u|`` 1.9e4 .. 8.2e4."""
    m = meshes[name]
    u = _dev(np.asarray(fd.rigid_motion(m["pts"], 0.5), dtype=np.float64))
    with _op(m["pts"], m["cells"], ()) as op:
        ku = float(op.apply(u)[0].abs().max())
        f = float(op.internal_force(u, material).abs().max())
    print(name, material, "max|f_fs| / max|K u| =", f / ku, "max|K u| =", ku)
    assert ku > 1e3                                                   # the linear operator answers a rigid rotation with a real load
    assert f <= TOL * ku


# ---- 3. the linear material is the block apply ------------------------------------------------------------------------------

@pytest.mark.parametrize("order", (1, 2))
def test_linear_material_is_the_apply(meshes, order):
    """Bit-equal, not only to 1e-14: material 0 launches the element pass of ``saa_operator_apply`` with ``m = 1`` and the
    same node sum."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    m = meshes[ORDER_MESH[order]]
    u = _dev(0.1 * fd.smooth_random_field(m["pts"], 9))
    with _op(m["pts"], m["cells"], m["dd"]) as op:
        want = op.apply(u)[0]
        got = op.internal_force(u, "linear")
        assert _err(_np(got), _np(want)) <= 1e-14 and torch.equal(got, want)
        with pytest.raises(_lib.SaaError) as exc:
            op.internal_force(u, "linear", energy=True)
        assert exc.value.code == _lib.SAA_E_ARG and "energy_elem_dev" in str(exc.value)


# ---- 4. the stepper against the double's loop -------------------------------------------------------------------------------

class Dynamic:
    """A clamped beam of one order on the GPU: handle, lumped mass, load, ``dt = 0.9 * 2/omega_max`` of the LINEAR operator,
    the bent state ``u0`` (tip rotation 0.3 rad) and a float64 double for the loop."""

    def __init__(self, m):
        from synchronization_avoiding_algorithms_amd.modal import stable_time_step_operator

        self.m = m
        self.op = _op(m["pts"], m["cells"], m["dd"])
        self.mass, self.load = self.op.lumped_mass(), self.op.load((0.0, -0.5, -0.5))
        self.dt = stable_time_step_operator(self.op, self.mass, 0.9)["dt"]
        self.u0 = fd.bend(m["pts"], 0.3, m["dd"])
        self.f64 = fd.FiniteStrain(m["pts"], m["cells"], LMD, MU, m["dd"], T=np.float64)
        self.live = self.f64.free.copy()
        self.live[np.repeat(np.bincount(m["cells"].ravel(), minlength=len(m["pts"])) == 0, 3)] = False
        self._runs = {}

    def stepper(self, material="linear", ramp=False):
        from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

        st = OperatorStepper(self.op, self.mass, self.load, self.dt, 0.5, ramp=ramp, material=material)
        st.set_state(_dev(self.u0), _dev(self.u0))
        return st

    def run(self, material, n=200):
        """``(d0, dn)`` after ``n`` steps in one call, computed once."""
        if (material, n) not in self._runs:
            with self.stepper(material) as st:
                st.step(n)
                d0, dn, _ = st.state()
                self._runs[material, n] = (d0, dn, st.inverted())
        return self._runs[material, n]


@pytest.fixture(scope="module")
def dynamic(meshes):
    out = {order: Dynamic(meshes[name]) for order, name in ORDER_MESH.items()}
    yield out
    for d in out.values():
        d.op.close()


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("order", (1, 2))
def test_stepper_against_the_double(dynamic, order, material):
    """200 steps, ``ramp=False``, ``alpha = 0.5``, ``dt = 0.9 * 2/omega_max``, from ``d0 = dn = u0``, the circular bend with
    the tip rotated by 0.3 rad.  Measured on the MI355X, rel-L2 of ``d0``: order 1 9.4e-15 (svk), 4.0e-14 (neo_hookean);
    order 2 7.4e-15, 7.4e-15.  The linear stepper from the same state ends 1.0e-1 (order 1) and 5.9e-2 (order 2) away."""
    c = dynamic[order]
    d0, dn, inverted = c.run(material)
    force = (lambda x: c.f64.force(x, material))
    want = fd.run(force, _np(c.mass), _np(c.load), c.live, c.dt, 0.5, False, 200, c.u0, c.u0)
    lin = c.run("linear")[0]
    e0, en = rel_l2(_np(d0), want[0]), rel_l2(_np(dn), want[1])
    guard = rel_l2(_np(lin), _np(d0))
    print(f"order {order} {material}: 200 steps from the bend, d0 {e0:.2e} dn {en:.2e}; linear stepper differs by {guard:.2e};",
          "max|d|", float(d0.abs().max()), "max|u0|", np.abs(c.u0).max(), "inverted", inverted)
    assert guard > 1e-3                                               # the material matters: 1e-11 means something
    assert float(d0.abs().max()) < 2.0 * np.abs(c.u0).max()           # the run stays bounded
    assert inverted == (0, -1)
    assert e0 < 1e-11 and en < 1e-11


# ---- 5. repeatability -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("order", (1, 2))
def test_runs_are_bitwise_repeatable_however_they_are_split(dynamic, order, material):
    import torch

    c = dynamic[order]
    d0, dn, _ = c.run(material)
    with c.stepper(material) as st:
        st.step(200)
        a0, an, _ = st.state()
    assert torch.equal(a0, d0) and torch.equal(an, dn)
    with c.stepper(material) as st:
        traj = st.record(200)
        marks = {}
        for k in range(200):
            st.step(1)
            if k % 50 == 49:
                marks[k] = st.state()[0]
        b0, bn, _ = st.state()
        assert torch.equal(b0, d0) and torch.equal(bn, dn)
        for k, s in marks.items():                                    # the recorder's column k is d^(k+1), the state after step k
            assert torch.equal(traj[:, k], s)
        assert torch.equal(traj[:, 198], dn) and torch.equal(traj[:, 199], d0)


# ---- 6. the partition -------------------------------------------------------------------------------------------------------

def _partition_against_whole(pts, cells, dnodes, dd, epart, P, label):
    """200 synchronised steps of ``OperatorPartition(material="svk")`` from the bend against the whole-mesh stepper, every
    holder's copy of a node bit-equal, then 50 predicted steps from the tables a synchronised run recorded."""
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorPartition, OperatorStepper

    u0 = _dev(fd.bend(pts, 0.3, dd))
    with OperatorPartition(pts, cells.astype(np.int32), dnodes, epart, P, rho=fd.RHO, fz=0.5, alpha=0.5, lame=(LMD, MU),
                           material="svk") as part:
        assert part.material == "svk" and all(r.stepper.material == "svk" for r in part.ranks)
        for r in part.ranks:
            r.stepper.set_state(u0[r.global_dof], u0[r.global_dof])
        with _op(pts, cells, dd) as op:
            with OperatorStepper(op, op.lumped_mass(), op.load((0.0, -0.5, -0.5)), part.dt, 0.5, material="svk") as st:
                st.set_state(u0, u0)
                st.step(200)
                w200 = st.state()
                st.step(50)
                w250 = st.state()
            with OperatorStepper(op, op.lumped_mass(), op.load((0.0, -0.5, -0.5)), part.dt, 0.5) as st:
                st.set_state(u0, u0)
                st.step(200)
                guard = rel_l2(_np(st.state()[0]), _np(w200[0]))
        part.step_synced(200)
        d0 = part.gather("d0")
        e200 = rel_l2(_np(d0), _np(w200[0]))
        for r in part.ranks:                                          # every holder's copy of a shared node, bit for bit
            assert torch.equal(r.get_state()[0], d0[r.global_dof])
        saved = [r.get_state() for r in part.ranks]
        hists = [torch.zeros((50, r.input_size), dtype=torch.float64, device="cuda") for r in part.ranks]
        part.step_synced(50, hists, 0)
        s250 = part.gather("d0")
        e250 = rel_l2(_np(s250), _np(w250[0]))
        for r, (a, b, tn) in zip(part.ranks, saved):
            r.stepper.set_state(a, b, tn)
        part.step_predicted(50, hists)
        p250 = part.gather("d0")
        ep = rel_l2(_np(p250), _np(s250))
        inverted = part.inverted()
    print(label, f"svk: 200 synchronised steps against the whole mesh {e200:.2e}, 250 {e250:.2e}; 50 predicted steps from the "
          f"recorded tables against the synchronised run {ep:.2e}; the linear stepper differs by {guard:.2e}; inverted", inverted)
    assert guard > 1e-3
    assert inverted == (0, -1)
    assert e200 < 1e-11 and e250 < 1e-11 and ep < 1e-11


@pytest.mark.parametrize("split", ("slab2", "mod3"))
def test_partition_order_two(meshes, split):
    """Measured on the MI355X: 200 / 250 synchronised steps against the whole mesh 8.4e-15 / 8.7e-15 (2 slabs), 6.6e-15 /
    1.5e-14 (3 interleaved parts); the 50 predicted steps reproduce the synchronised run bit for bit."""
    from synchronization_avoiding_algorithms_amd.mesh import slab_partition, structured_beam

    m = meshes["curved288"]
    epart, P = (slab_partition(structured_beam(2, length=6.0), 2), 2) if split == "slab2" else (np.arange(288) % 3, 3)
    _partition_against_whole(m["pts"], m["cells"], np.unique(m["dd"] // 3), m["dd"], epart, P, "curved288 " + split)


def test_partition_order_one():
    """Measured on the MI355X: 1.35e-14 / 1.38e-14 after 200 / 250 synchronised steps, predicted steps bit-equal; the
    linear stepper ends 1.6e-1 away."""
    from synchronization_avoiding_algorithms_amd.fem_setup import node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, slab_partition, structured_beam

    mesh = structured_beam(2)
    dnodes = plane_nodes(mesh.points)
    _partition_against_whole(mesh.points, np.asarray(mesh.tets, dtype=np.int64), dnodes, node_to_dof(dnodes),
                             slab_partition(mesh, 2), 2, "structured_beam(2) slab2")


# ---- 7. inversion -----------------------------------------------------------------------------------------------------------

def test_inverted_elements_contribute_nothing_and_are_counted(meshes):
    """Vertex 5 of the 36-tet beam (and the mid-edge nodes of its edges by half as much) pushed through the opposite faces
    of its four elements, on a gentle background field so that the other elements carry a force.  Measured on the MI355X:
    4 inverted, ``f`` 8.2e-16 and ``energy_elem`` 1.1e-15 of the largest entry against the double with them dropped."""
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    m = meshes["beam36"]
    fs = m["fs"]
    node, u, star = fd.inversion_state(fs, m["pts"], 0.02 * fd.smooth_random_field(m["pts"], 3))
    want_f, want_e, inv = fs.evaluate(u, "neo_hookean")
    assert list(np.nonzero(inv)[0]) == list(star) and len(star) > 0   # exactly the elements around the node, in the double
    with _op(m["pts"], m["cells"], m["dd"]) as op:
        f, en, n_inv = op.internal_force(_dev(u), "neo_hookean", energy=True)
        ef, ee = _err(_np(f), want_f), _err(_np(en), want_e)
        print("node", node, "elements", list(star), "n_inverted", n_inv, f"f {ef:.2e} energy_elem {ee:.2e}")
        assert n_inv == len(star)
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(en).all()) and not _np(en)[star].any()
        assert ef <= TOL and ee <= TOL
        assert op.internal_force(_dev(u), "svk", energy=True)[2] == 0  # St. Venant-Kirchhoff does not look at J
        mass, load = op.lumped_mass(), op.load((0.0, -0.5, -0.5))
        with OperatorStepper(op, mass, load, 1e-5, 0.5, ramp=False, material="neo_hookean") as st:
            assert st.inverted() == (0, -1)
            st.set_state(_dev(u), _dev(u))
            st.step(1)
            assert st.inverted() == (len(star), 0)
            assert bool(torch.isfinite(st.state()[0]).all())
            st.set_state(_dev(u), _dev(u))
            assert st.inverted() == (0, -1)
            st.step(2)                                                # the step index runs on: steps 1 and 2
            count, first = st.inverted()
            assert first == 1 and count >= len(star)
            st.set_material("neo_hookean")
            assert st.inverted() == (0, -1)


# ---- 8. state rules ---------------------------------------------------------------------------------------------------------

def test_state_rules(dynamic):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    c = dynamic[2]
    with c.stepper("svk") as st:
        with pytest.raises(_lib.SaaError) as exc:
            st.record_energy(4)
        assert exc.value.code == _lib.SAA_E_STATE and "nonlinear material" in str(exc.value)
        st.step_begin()                                               # without a shared set begin + finish is the plain step
        with pytest.raises(_lib.SaaError) as exc:
            st.set_material("linear")
        assert exc.value.code == _lib.SAA_E_STATE and "in flight" in str(exc.value)
        st.step_finish()
        st.set_material("linear")
        st.record_energy(4)
        with pytest.raises(_lib.SaaError) as exc:
            st.set_material("neo_hookean")
        assert exc.value.code == _lib.SAA_E_STATE and "energy balance" in str(exc.value)
        st.record_energy(0)
        st.set_state(_dev(c.u0), _dev(c.u0))
        st.step(50)
        got = st.state()
    with c.stepper() as ref:                                          # a stepper that never had a material
        ref.step(50)
        want = ref.state()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------

def test_driver_dynamics_with_a_material(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "dynamics", "--synthetic", "2", "--order", "2",
            "--material", "svk", "--fz", "50", "--steps", "200", "--out", str(tmp_path)]
    out = subprocess.run(base, cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["material"] == "svk" and res["inverted"] == 0 and res["first_inverted_step"] == -1
    assert res["order"] == 2 and res["steps"] == 200 and res["max_abs_d"] > 0 and np.isfinite(res["tip_deflection"])
    bad = subprocess.run(base + ["--energy"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300, env=env)
    assert bad.returncode != 0
    assert "the energy balance is defined for the linear material only" in bad.stderr and "Traceback" not in bad.stderr
