"""Explicit dynamics on the operator handle on the GPU: ``saa_operator_lumped_mass`` and the ``saa_operator_stepper`` of
either order against the NumPy double (tests/p2_dynamics_double.py: dense ``K`` from tests/p2_double.py), the production
step kernel (order 1), the steady solution (physics) and the driver.

Shapes: the smallest that cross a block edge of the 256-lane passes - 36 tets / 117 nodes sit inside one block; 288 tets =
256 + 32 and 625 nodes = 2 x 256 + 113 run a partial last block in both passes.  Both element passes of order 2
(``stored_geometry`` 0 and 1) run every parity case.

Bars: 1e-13 / 1e-14 for the lumped masses (sums of at most a few dozen positive terms); rel-L2 < 1e-11 for states after a
few hundred steps, the project's short-run bar (two independent NumPy formulations of the 500-step run differ by 2.5e-13);
1e-8 for ``omega_max`` (tests/test_gpu_modal.py); 1e-9 for the settled state against the steady solve (the steady bar of
tests/test_steady.py; the double of tests/p2_dynamics_double.py reaches 1.7e-12 against a dense solve)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden, rel_l2

import p2_double as p2
import p2_dynamics_double as dyn

pytestmark = pytest.mark.gpu

E, NU, RHO, FZ = 1e6, 0.3, 1.0, 0.5
OMEGA_MAX = {1: 8893.974037, 2: 17548.990195}        # dense eigh, tests/test_p2_dynamics.py
STORED = (0, 1)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _op(points, cells, dirichlet, lmd, mu, rho):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(points, cells, dirichlet, lmd, mu, rho)


def _stepper(op, mass, load, dt, alpha, ramp=True, stored=0):
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    st = OperatorStepper(op, mass, load, dt, alpha, ramp=ramp)
    st.set_option("stored_geometry", stored)
    return st


class Case:
    """A clamped order-2 beam with its dense double: K, HRZ mass, load, dt = 0.9 dt_crit."""

    def __init__(self, points, cells10, dirichlet, lmd, mu, rho, fz):
        self.pts, self.c10, self.dd = points, cells10, np.asarray(dirichlet, dtype=np.int64)
        self.lmd, self.mu, self.rho = lmd, mu, rho
        self.K, _ = p2.assemble(points, cells10, self.dd, lmd, mu, rho)
        self.mass = dyn.hrz_mass(points, cells10, rho)
        self.load = p2.load(points, cells10, self.dd, (0.0, -fz, -fz))
        self.omega_min, self.omega_max = dyn.omega_extremes(self.K, self.mass, self.dd)
        self.dt = 0.9 * 2.0 / self.omega_max

    def op(self):
        return _op(self.pts, self.c10, self.dd, self.lmd, self.mu, self.rho)

    def run(self, nsteps, alpha=0.5, ramp=True, **kw):
        return dyn.run(self.K, self.mass, self.load, self.dd, self.dt, alpha, ramp, nsteps, **kw)


@pytest.fixture(scope="module")
def beam36():
    """to_quadratic(structured_beam(1, length=6.0)) with every mid-edge node moved by a seeded +-0.025."""
    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

    quad = to_quadratic(structured_beam(1, length=6.0))
    nv = len(structured_beam(1, length=6.0).points)
    pts = quad.points.copy()
    pts[nv:] += np.random.default_rng(11).uniform(-0.025, 0.025, size=(len(pts) - nv, 3))
    assert quad.tets10.shape == (36, 10) and len(pts) == 117
    return Case(pts, quad.tets10, node_to_dof(plane_nodes(quad.points)), *lame(E, NU), RHO, FZ)


@pytest.fixture(scope="module")
def straight36():
    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

    quad = to_quadratic(structured_beam(1, length=6.0))
    return Case(quad.points, quad.tets10, node_to_dof(plane_nodes(quad.points)), *lame(E, NU), RHO, FZ)


@pytest.fixture(scope="module")
def gold():
    g = load_golden("p2_beam.npz")
    g["mat"] = tuple(float(g[k]) for k in ("lmd", "mu", "rho", "fz"))
    return g


@pytest.fixture(scope="module")
def curved288(gold):
    lmd, mu, rho, fz = gold["mat"]
    assert gold["cells10"].shape == (288, 10) and len(gold["points_curved"]) == 625
    return Case(gold["points_curved"], gold["cells10"], gold["dirichlet_dofs"], lmd, mu, rho, fz)


# ---- lumped mass -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("straight", "curved"))
def test_lumped_mass_order_two_matches_the_double(gold, name):
    pts, c10, dd = gold[f"points_{name}"], gold["cells10"], gold["dirichlet_dofs"]
    lmd, mu, rho, _ = gold["mat"]
    with _op(pts, c10, dd, lmd, mu, rho) as op:
        got = op.lumped_mass().cpu().numpy()
        again = op.lumped_mass().cpu().numpy()
    want = dyn.hrz_mass(pts, c10, rho)
    err = rel_l2(got, want)
    print(name, "HRZ mass rel-L2", err, "min", got.min(), "sum / (rho V) - 1", got[0::3].sum() / (rho * 6.0) - 1.0)
    assert err < 1e-13 and (got > 0).all() and np.array_equal(got, again)
    assert (got[dd] > 0).all()                                       # the Dirichlet mask is not applied
    assert np.array_equal(got[0::3], got[1::3]) and np.array_equal(got[0::3], got[2::3])


def test_lumped_mass_order_one_matches_the_setup_kernels():
    from synchronization_avoiding_algorithms_amd.fem_setup import device_setup_fields, lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam

    mesh = structured_beam(2)
    lmd, mu = lame(E, NU)
    rho = 1.3
    want, _, _ = device_setup_fields(mesh.points, mesh.tets, rho, FZ, 0)
    with _op(mesh.points, mesh.tets, node_to_dof(plane_nodes(mesh.points)), lmd, mu, rho) as op:
        assert op.order == 1
        got = op.lumped_mass().cpu().numpy()
    err = rel_l2(got, want)
    print("order 1 lumped mass against saa_setup_fields", err)
    assert err < 1e-14


# ---- parity with the double -----------------------------------------------------------------------------------------------

def _compare(st, want, label):
    d0, dn, tn = st.state()
    e0, en = rel_l2(d0.cpu().numpy(), want[0]), rel_l2(dn.cpu().numpy(), want[1])
    print(label, "rel-L2 d0", e0, "dn", en, "tn", tn, want[2])
    assert e0 < 1e-11 and en < 1e-11 and abs(tn - want[2]) <= 1e-14 * abs(want[2])
    return d0.cpu().numpy(), dn.cpu().numpy()


@pytest.mark.parametrize("stored", STORED)
def test_500_steps_on_the_36_tet_beam(beam36, stored):
    c = beam36
    want = c.run(500)
    with c.op() as op:
        mass = op.lumped_mass()
        assert rel_l2(mass.cpu().numpy(), c.mass) < 1e-13
        with _stepper(op, mass, op.load((0.0, -FZ, -FZ)), c.dt, 0.5, stored=stored) as st:
            st.step(500)
            d0, dn = _compare(st, want, f"36 tets, 500 steps, stored_geometry={stored}:")
    assert not d0[c.dd].any() and not dn[c.dd].any()                 # exactly 0
    assert np.abs(d0).max() > 0


@pytest.mark.parametrize("stored", STORED)
def test_200_steps_on_the_curved_288_tet_beam(curved288, stored):
    c = curved288
    want = c.run(200)
    with c.op() as op:
        with _stepper(op, op.lumped_mass(), _dev(c.load), c.dt, 0.5, stored=stored) as st:
            st.step(200)
            d0, dn = _compare(st, want, f"288 curved tets, 200 steps, stored_geometry={stored}:")
    assert not d0[c.dd].any() and not dn[c.dd].any()


@pytest.mark.parametrize("stored", STORED)
def test_launch_splits_and_buffer_parity_are_bitwise_equal(curved288, stored):
    import torch

    c = curved288
    with c.op() as op:
        mass, load = op.lumped_mass(), _dev(c.load)

        def run(chunks):
            with _stepper(op, mass, load, c.dt, 0.5, stored=stored) as st:
                for n in chunks:
                    st.step(n)
                return st.state()

        ref = run([7])
        for chunks in ([1] * 7, [3, 4], [7], [0, 7, 0]):
            got = run(chunks)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2] == ref[2], chunks
        # an odd count leaves d0 in the second buffer: get_state must hand back that one, and dn the step before
        want = c.run(7)
        assert rel_l2(ref[0].cpu().numpy(), want[0]) < 1e-11 and rel_l2(ref[1].cpu().numpy(), want[1]) < 1e-11
        six = run([6])
        assert torch.equal(six[0], ref[1])
        # nsteps = 0 changes nothing
        with _stepper(op, mass, load, c.dt, 0.5, stored=stored) as st:
            st.step(3)
            a = st.state()
            st.step(0)
            b = st.state()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("ramp", (True, False))
def test_ramp_clamp(beam36, ramp):
    """tn crosses 1 between the fourth and the fifth of 8 steps: min(tn, 1) on both sides of the clamp."""
    c = beam36
    rng = np.random.default_rng(3)
    d0 = rng.uniform(-1e-4, 1e-4, size=len(c.mass))
    dn = d0 + rng.uniform(-1e-6, 1e-6, size=len(c.mass))
    d0[c.dd] = dn[c.dd] = 0.0
    t0 = 1.0 - 3.5 * c.dt
    want = c.run(8, ramp=ramp, d0=d0, dn=dn, tn=t0)
    other = c.run(8, ramp=not ramp, d0=d0, dn=dn, tn=t0)
    assert rel_l2(other[0], want[0]) > 1e-9                          # the case tells the two apart
    with c.op() as op:
        with _stepper(op, c.mass, c.load, c.dt, 0.5, ramp=ramp) as st:
            st.set_state(d0, dn, t0)
            st.step(8)
            _compare(st, want, f"ramp={ramp}, tn from 1 - 3.5 dt:")


# ---- recorder ---------------------------------------------------------------------------------------------------------------

def test_recorder_columns_guard_and_continuation(beam36):
    import torch

    c = beam36
    n = len(c.mass)
    cols = {}
    c.run(10, record=lambda i, d1: cols.__setitem__(i, d1.copy()))
    with c.op() as op:
        mass, load = op.lumped_mass(), op.load((0.0, -FZ, -FZ))
        with _stepper(op, mass, load, c.dt, 0.5) as st:
            traj = st.record(4, save_every=3)
            st.step(10)
            got = traj.cpu().numpy()
        for k, i in enumerate((0, 3, 6, 9)):
            assert rel_l2(got[:, k], cols[i]) < 1e-11, (k, i)
        assert not got[:, 0].any() and got[:, 3].any()               # step 0 starts from rest under a ramped load
        # three columns: step 9 has no column; nothing lands past the end (nor in column 0 of the next row)
        guard = torch.full((3 * n + n,), -7.0, dtype=torch.float64, device="cuda")
        with _stepper(op, mass, load, c.dt, 0.5) as st:
            t3 = st.record(3, save_every=3, out=guard)
            st.step(10)
            got3 = t3.cpu().numpy()
        assert np.array_equal(got3, got[:, :3]) and bool((guard[3 * n:] == -7.0).all())
        # a non-zero next_step_index continues a run: steps 5..9 of the same trajectory fill columns 2 and 3 only
        with _stepper(op, mass, load, c.dt, 0.5) as st:
            st.step(5)
            cont = st.record(4, save_every=3, next_step_index=5, out=torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda"))
            st.step(5)
            gc = cont.cpu().numpy()
            st.record(0)
            st.step(1)                                               # recorder off: no write
            assert np.array_equal(cont.cpu().numpy(), gc)
        assert (gc[:, :2] == -7.0).all() and np.array_equal(gc[:, 2:], got[:, 2:])


# ---- orphan node ---------------------------------------------------------------------------------------------------------

def test_a_node_without_elements_stays_at_zero(beam36):
    c = beam36
    pts = np.vstack([c.pts, [[9.0, 9.0, 9.0]]])
    mass = np.concatenate([c.mass, np.zeros(3)])
    load = np.concatenate([c.load, [1.0, 1.0, 1.0]])
    with c.op() as op:
        with _stepper(op, c.mass, c.load, c.dt, 0.5) as st:
            st.step(20)
            ref = st.state()[0].cpu().numpy()
    with _op(pts, c.c10, c.dd, c.lmd, c.mu, c.rho) as op:
        got_mass = op.lumped_mass().cpu().numpy()
        assert not got_mass[-3:].any() and np.array_equal(got_mass[:-3] > 0, np.ones(len(c.mass), dtype=bool))
        with _stepper(op, mass, load, c.dt, 0.5) as st:
            st.step(20)
            d0, dn, _ = st.state()
    d0, dn = d0.cpu().numpy(), dn.cpu().numpy()
    assert np.isfinite(d0).all() and np.isfinite(dn).all()
    assert not d0[-3:].any() and not dn[-3:].any()
    assert np.array_equal(d0[:-3], ref)


def test_create_refuses_a_non_positive_mass_at_a_node_with_elements(beam36):
    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    c = beam36
    with c.op() as op:
        for bad in (0.0, -1.0, float("nan")):
            mass = c.mass.copy()
            mass[3 * 50 + 1] = bad
            with pytest.raises(_lib.SaaError, match="mass is not > 0") as ei:
                OperatorStepper(op, mass, c.load, c.dt, 0.5)
            assert ei.value.code == _lib.SAA_E_ARG


# ---- order 1 against the production kernel --------------------------------------------------------------------------------

def test_order_one_against_the_production_step_kernel():
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes, structured_beam
    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver

    mesh = structured_beam(2)
    lmd, mu = fs.lame(E, NU)
    lumped, fpre, min_edge = fs.device_setup_fields(mesh.points, mesh.tets, RHO, FZ, 0)
    dd = fs.node_to_dof(clamp_nodes(mesh))
    dt = fs.dt_from_min_edge(min_edge, E, NU, RHO, 0.9)
    with HipExplicitSolver(mesh.points, mesh.tets, lumped, fpre, dd, lmd, mu, dt, 0.5, device=0) as sol:
        sol.step(200)
        w0, wn, wt = sol.get_state()
    with _op(mesh.points, mesh.tets, dd, lmd, mu, RHO) as op:
        with _stepper(op, lumped, fpre, dt, 0.5) as st:
            st.step(200)
            d0, dn, tn = st.state()
    e0, en = rel_l2(d0.cpu().numpy(), w0), rel_l2(dn.cpu().numpy(), wn)
    print("order 1, 1200 tets, 200 steps against HipExplicitSolver: d0", e0, "dn", en, "tn", tn, wt)
    assert e0 < 1e-11 and en < 1e-11 and abs(tn - wt) <= 1e-14 * wt
    assert not d0.cpu().numpy()[dd].any()


# ---- time step ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 2))
def test_stable_time_step_operator_reproduces_the_dense_omega_max(n):
    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import stable_time_step_operator

    quad = to_quadratic(structured_beam(n, length=6.0))
    lmd, mu = lame(E, NU)
    with _op(quad.points, quad.tets10, node_to_dof(plane_nodes(quad.points)), lmd, mu, RHO) as op:
        r = stable_time_step_operator(op, op.lumped_mass(), gamma=0.9)
    print(n, r)
    assert set(r) == {"omega_max", "dt_crit", "dt"}
    assert abs(r["omega_max"] / OMEGA_MAX[n] - 1.0) < 1e-8
    assert r["dt_crit"] == 2.0 / r["omega_max"] and r["dt"] == 0.9 * r["dt_crit"]


# ---- physics ------------------------------------------------------------------------------------------------------------

def test_critically_damped_run_settles_on_the_steady_solution(straight36):
    """alpha = 2 omega_1 damps the first mode critically (and every other one more than that relative to its period):
    after t = 2.0 = 56 / omega_1 with the load constant since t = 1 the state is the steady one."""
    from synchronization_avoiding_algorithms_amd.steady import steady_solve_operator

    c = straight36
    assert abs(c.omega_min / 28.17398 - 1.0) < 1e-6 and abs(c.omega_max / OMEGA_MAX[1] - 1.0) < 1e-9
    nsteps = 9882
    assert abs(nsteps * c.dt - 2.0) < c.dt
    with c.op() as op:
        load = op.load((0.0, -FZ, -FZ))
        want, _, rel = steady_solve_operator(op, load, tol=1e-13)
        with _stepper(op, op.lumped_mass(), load, c.dt, 2.0 * c.omega_min) as st:
            st.step(nsteps)
            d0, dn, tn = st.state()
    err = rel_l2(d0.cpu().numpy(), want)
    print("t =", tn, "rel-L2 to the steady solution", err, "steady residual", rel, "last increment",
          rel_l2(d0.cpu().numpy(), dn.cpu().numpy()))
    assert err < 1e-9


# ---- driver ---------------------------------------------------------------------------------------------------------------

def test_driver_dynamics(tmp_path):
    from synchronization_avoiding_algorithms_amd.results_io import load_displacement

    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "dynamics", "--synthetic", "1",
                          "--order", "2", "--steps", "50", "--out", str(tmp_path)], cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["order"] == 2 and res["n_elems"] == 150 and res["steps"] == 50
    assert res["dt"] < res["dt_crit"] < res["dt_reference_rule"]
    assert res["ratio"] == pytest.approx(res["dt_reference_rule"] / res["dt_crit"]) and res["tn"] == pytest.approx(50 * res["dt"])
    assert res["max_abs_d"] > 0 and np.isfinite(res["tip_deflection"])
    data = load_displacement(str(tmp_path / "Results" / "Dynamics" / "Displacement_order2.hdf5"))
    assert data.shape == (3 * res["n_nodes"], 50) and np.isfinite(data).all() and data[:, -1].any()
    assert np.abs(data[:, -1]).max() == pytest.approx(res["max_abs_d"])    # the last column is the final state
