"""Following the time step at finite strain on the MI355X (``csrc/saa_opdt.hip``): ``saa_operator_tangent_bound`` and
``saa_operator_stepper_set_dt`` against the double of tests/dt_follow_double.py (tests/test_dt_follow.py qualifies it on the
CPU), ``OperatorStepper.follow_time_step`` on the release scenario, and ``drivers dynamics --dt-follow``.

The bound is held to the bar of tests/test_gpu_tangent.py, ``err = max|omega_e - r| / max|r| <= 1e-12 + 8 env`` with ``r`` the
longdouble double and ``env`` its largest change under eight ``+-2^-53`` perturbations of the inputs.  The meshes are the four of
``finite_strain_double.MESHES`` (288 tets: two workgroups, one partial; the Delaunay beam; 36 and 288 quadratic tets), except the
driver's, which it builds itself."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dt_follow_double as dd
import finite_strain_double as fd

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = fd.lame(fd.E, fd.NU)
ALL = ("linear", "svk", "neo_hookean")
ALPHA = 0.5


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _operator(pts, cells, dofs):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(pts, np.asarray(cells).astype(np.int32), np.asarray(dofs).astype(np.int32), LMD, MU, fd.RHO)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return fd.mesh(name)


@functools.lru_cache(maxsize=None)
def _reference(name, material, st):
    """``(u, omega_e longdouble-built, env)``, computed once per case."""
    pts, cells, dofs = _mesh(name)
    fs = dd.Bound(pts, cells, LMD, MU, fd.RHO, dofs)
    u = dd.state(st, pts, dd.Bound(pts, cells, LMD, MU, fd.RHO, dofs, T=np.float64))
    ref = fs.omega_e(u, material)
    assert not ref["inverted"].any() and np.isfinite(ref["omega_e"]).all()
    return u, ref["omega_e"], dd.envelope(pts, cells, dofs, u, material, ref["omega_e"])


@pytest.mark.parametrize("material", ALL)
@pytest.mark.parametrize("name", fd.MESHES)
def test_the_bound_against_the_double(name, material):
    pts, cells, dofs = _mesh(name)
    with _operator(pts, cells, dofs) as op:
        for st in (("zero",) if material == "linear" else dd.STATES):
            u, ref, env = _reference(name, material, st)
            bar = 1e-12 + 8 * env
            b = op.tangent_bound(None if material == "linear" else _dev(u), material, return_omega=True)
            got = b["omega_e"].cpu().numpy()
            err = float(np.abs(got - ref).max() / ref.max())
            ties = int((got == got.max()).sum())
            print(f"{name:14s} {material:12s} {st:7s} err {err:.2e}  env {env:.2e}  bar {bar:.2e}  argmax {b['element']} ({ties} tied)")
            assert err <= bar
            assert (b["n_nonpositive"], b["n_inverted"], b["n_nonfinite"], b["certified"]) == (0, 0, 0, True)
            # the maximum is an entry of omega_e, bit for bit, its element the lowest index that holds it, and it is the
            # reference's maximum up to the bar
            assert b["omega_max"] == got.max() and b["element"] == int(np.argmax(got))
            assert ref[b["element"]] >= ref.max() * (1 - bar) and abs(b["omega_max"] - ref.max()) <= bar * ref.max()
            # omega_e_dev = NULL, counts = NULL; a second call
            again = op.tangent_bound(None if material == "linear" else _dev(u), material)
            assert "omega_e" not in again and again == {k: v for k, v in b.items() if k != "omega_e"}
            w, arg = C.c_double(), C.c_int32()
            ptr = None if material == "linear" else C.c_void_p(_dev(u).data_ptr())
            from synchronization_avoiding_algorithms_amd import _lib

            _lib.check(op._lib.saa_operator_tangent_bound(op._h, _lib.material_id(material), ptr, None, C.byref(w), C.byref(arg), None))
            assert (w.value, arg.value) == (b["omega_max"], b["element"])
            assert np.array_equal(op.tangent_bound(None if material == "linear" else _dev(u), material, True)["omega_e"].cpu().numpy(), got)
        if material == "linear":                                       # u is ignored: a state changes nothing
            u = _reference(name, "svk", "strain")[0]
            assert np.array_equal(op.tangent_bound(_dev(u), "linear", True)["omega_e"].cpu().numpy(), got)


def test_on_the_structured_beam_at_rest_many_elements_tie_and_the_lowest_wins():
    """The six tetrahedra of a cell repeat along the beam: the double finds the maximum on element 0 and many elements within
    round-off of it; the GPU's element is the lowest index among the entries equal to ITS maximum."""
    pts, cells, dofs = _mesh("structured288")
    u, ref, env = _reference("structured288", "svk", "zero")
    near = np.nonzero(ref >= ref.max() * (1 - 1e-12))[0]
    assert len(near) > 1
    with _operator(pts, cells, dofs) as op:
        for material in ALL:
            b = op.tangent_bound(_dev(u), material, return_omega=True)
            got = b["omega_e"].cpu().numpy()
            assert b["element"] in near and b["element"] == int(np.nonzero(got == b["omega_max"])[0][0])


@pytest.mark.parametrize("name", ("structured288", "beam36"))
def test_the_counts(name):
    pts, cells, dofs = _mesh(name)
    fs = dd.Bound(pts, cells, LMD, MU, fd.RHO, dofs, T=np.float64)
    # a flipped element: two vertices exchanged (order 2: and the mid-edge nodes that go with them)
    flipped = cells.copy()
    flipped[5] = cells[5][[1, 0, 2, 3] if cells.shape[1] == 4 else [1, 0, 2, 3, 4, 6, 5, 8, 7, 9]]
    u = dd.state("strain", pts, fs)
    with _operator(pts, flipped, dofs) as op:
        for material in ALL:
            b = op.tangent_bound(_dev(u), material)
            assert b["n_nonpositive"] == 1 and not b["certified"], (material, b)
    # one vertex pushed through its star: neo-Hooke drops exactly those elements, SVK none
    node, ui, star = fd.inversion_state(fs, pts, background=0.1 * u)
    want = fs.bound(ui, "neo_hookean")
    assert want["n_inverted"] == len(star) > 0
    with _operator(pts, cells, dofs) as op:
        b = op.tangent_bound(_dev(ui), "neo_hookean", return_omega=True)
        got = b["omega_e"].cpu().numpy()
        assert b["n_inverted"] == len(star) and (got[star] == 0.0).all() and b["n_nonfinite"] == 0
        rest = np.setdiff1d(np.arange(len(cells)), star)
        assert b["element"] in rest and b["omega_max"] == got[rest].max()
        assert abs(b["omega_max"] - want["omega_max"]) <= 1e-10 * want["omega_max"]
        s = op.tangent_bound(_dev(ui), "svk")
        assert s["n_inverted"] == 0 and s["n_nonfinite"] == 0 and s["omega_max"] > 0
        # a NaN in u: its elements are not finite, counted, and left out of the maximum
        bad = u.copy()
        free_node = int(np.nonzero(fs.free.reshape(-1, 3).all(axis=1))[0][-1])
        bad[3 * free_node] = np.nan
        touched = np.nonzero((cells == free_node).any(axis=1))[0]
        b = op.tangent_bound(_dev(bad), "svk", return_omega=True)
        got = b["omega_e"].cpu().numpy()
        assert b["n_nonfinite"] == len(touched) > 0 and not np.isfinite(got[touched]).any()
        clean = np.setdiff1d(np.arange(len(cells)), touched)
        assert np.isfinite(b["omega_max"]) and b["omega_max"] == got[clean].max() and b["element"] in clean
        assert np.array_equal(got[clean], op.tangent_bound(_dev(u), "svk", True)["omega_e"].cpu().numpy()[clean])


def _stepper(op, material, dt, load=None):
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    mass = op.lumped_mass()
    return OperatorStepper(op, mass, _dev(np.zeros(op.n_dof)) if load is None else _dev(load), dt, ALPHA, ramp=True,
                           material=material), mass.cpu().numpy()


@pytest.mark.parametrize("name,material", (("structured288", "neo_hookean"), ("beam36", "svk"), ("curved288", "linear")))
def test_set_dt_against_the_double(name, material):
    from synchronization_avoiding_algorithms_amd import _lib

    fs, live, mass64, _, u, dt, _ = dd.release_problem(name, "svk" if material == "linear" else material, strain=0.1)
    pts, cells, dofs = _mesh(name)
    load = 1e-3 * mass64
    small = 1e-3 * fd.smooth_random_field(pts, 5) * live
    tn = 0.3
    force = (lambda d: np.asarray(fs.linear_force(d), dtype=np.float64)) if material == "linear" else \
        (lambda d: np.asarray(fs.force(d, material), dtype=np.float64))
    with _operator(pts, cells, dofs) as op:
        st, mass = _stepper(op, material, dt, load)
        with st:
            assert np.abs(mass - mass64).max() <= 1e-13 * mass64.max()
            st.set_state(_dev(u), _dev(u - small), tn)
            traj = st.record(3)
            # the same dt: nothing is launched, both buffers bit-equal
            st.set_dt(dt)
            d0, dn, t = st.state()
            assert np.array_equal(d0.cpu().numpy(), u) and np.array_equal(dn.cpu().numpy(), u - small) and t == tn
            new = 0.6 * dt
            st.set_dt(new)
            d0, dn, t = st.state()
            want = dd.set_dt(force(u), mass, load, live, u, u - small, dt, new, ALPHA, min(tn, 1.0))
            err = float(np.abs(dn.cpu().numpy() - want).max() / np.abs(u).max())
            print(f"{name} {material}: dn' against the double, {err:.2e} of max|d|")
            assert err <= 1e-12
            assert np.array_equal(d0.cpu().numpy(), u) and t == tn and st.dt == new and st.inverted() == (0, -1)
            assert (dn.cpu().numpy()[~live] == 0.0).all()
            # the recorder's column index did not move: the next step fills column 0, and it is the step of the new dt
            st.step(1)
            d1, _, t1 = st.state()
            assert t1 == tn + new and np.array_equal(traj[:, 0].cpu().numpy(), d1.cpu().numpy()) and not traj[:, 1:].any()
            ref = fd.run(force, mass, load, live, new, ALPHA, True, 1, u, want, tn)[0]
            assert np.abs(d1.cpu().numpy() - ref).max() <= 1e-12 * np.abs(u).max()
            # refusals
            for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0 / ALPHA):
                with pytest.raises(_lib.SaaError, match="dt_new") as exc:
                    st.set_dt(bad)
                assert exc.value.code == _lib.SAA_E_ARG and st.dt == new
            st.step_begin()
            with pytest.raises(_lib.SaaError, match="in flight") as exc:
                st.set_dt(dt)
            assert exc.value.code == _lib.SAA_E_STATE
            st.step_finish()
            st.set_shared([0], [0], 1)
            with pytest.raises(_lib.SaaError, match="shared set") as exc:
                st.set_dt(dt)
            assert exc.value.code == _lib.SAA_E_STATE
            st.set_shared([], [], 0)
            st.set_option("passes", 1)
            with pytest.raises(_lib.SaaError, match="passes") as exc:
                st.set_dt(dt)
            assert exc.value.code == _lib.SAA_E_STATE
            st.set_option("passes", 3)
            if material == "linear":
                st.record_energy(4)
                with pytest.raises(_lib.SaaError, match="energy balance") as exc:
                    st.set_dt(dt)
                assert exc.value.code == _lib.SAA_E_STATE
                st.record_energy(0)
            st.set_dt(dt)                                              # and after all that it works again
            assert st.dt == dt


@pytest.mark.parametrize("mode", ("certified", "anchored"))
@pytest.mark.parametrize("name,material", (("structured288", "neo_hookean"), ("beam36", "svk")))
def test_the_released_beam_is_followed(name, material, mode):
    """The release at rest from the 0.3-strain state with the linear operator's ``dt``: above the limit as created, below it after
    the first check and at every later one, nothing inverts, and the state is that of the velocity form of the scheme fed with the
    ``(step, dt)`` list of this run, to the short-run bar rel-L2 1e-11."""
    from conftest import rel_l2

    fs, live, mass64, load, u, dt, omega_l = dd.release_problem(name, material)
    pts, cells, dofs = _mesh(name)
    n_steps, every = 40, 5
    with _operator(pts, cells, dofs) as op:
        st, mass = _stepper(op, material, dt)
        with st:
            st.set_state(_dev(u), _dev(u), 0.0)
            first = st.stable_time_step()
            assert abs(first["dt"] - dt) == 0.0 and 1.0 < first["dt_over_dt_crit"] < 1.4, first
            records, ratios = [], []
            for done in range(0, n_steps, every):
                records.append(st.follow_time_step(mode, 0.9))
                ratios.append(st.stable_time_step()["dt_over_dt_crit"])
                st.step(every)
            d0 = st.state()[0].cpu().numpy()
            print(f"{name} {material} {mode}: dt/dt_crit created {first['dt_over_dt_crit']:.3f}, followed {max(ratios):.3f} at worst; "
                  f"dt {[f'{r[3]:.3e}' for r in records]}")
            assert [r[0] for r in records] == list(range(0, n_steps, every)) and max(ratios) <= 1.0
            assert all(r[3] <= dt for r in records) and records[-1][3] == st.dt
            assert st.inverted() == (0, -1)
    force = lambda d: np.asarray(fs.force(d, material), dtype=np.float64)  # noqa: E731
    dts = dd.per_step([(r[0], r[3]) for r in records], n_steps)
    want = dd.run_variable(dts, force, mass, load, live, ALPHA, True, u, u, dt)[0]
    err = rel_l2(d0, want)
    print(f"{name} {material} {mode}: state against the velocity form, rel-L2 {err:.2e}; max|d| {np.abs(d0).max():.3f}")
    assert np.abs(d0).max() < 1.0 and err <= 1e-11


def _driver(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=str(cwd),
                          capture_output=True, text=True, timeout=300, env=env)


# what `drivers dynamics --material svk` printed before the flag existed
PLAIN_KEYS = {"order", "n_nodes", "n_elems", "n_free_dofs", "dt", "dt_crit", "dt_reference_rule", "ratio", "omega_max", "steps", "tn",
              "max_abs_d", "tip_deflection", "material", "inverted", "first_inverted_step", "path"}


def test_driver_dynamics_follows_the_time_step_and_leaves_the_plain_run_alone(tmp_path):
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    base = ["dynamics", "--synthetic", "2", "--order", "2", "--material", "svk", "--fz", "50", "--steps", "40", "--save-every", "2"]
    runs = {}
    for tag, extra in (("followed", ["--dt-follow", "anchored", "--dt-follow-every", "10", "--dt-check-every", "20"]), ("plain", [])):
        where = tmp_path / tag
        where.mkdir()
        out = _driver(base + extra + ["--out", str(where)], where)
        assert out.returncode == 0, out.stderr[-3000:]
        runs[tag] = json.loads(out.stdout.strip().splitlines()[-1])
    follow = runs["followed"]["dt_follow"]
    print(follow)
    assert set(follow) == {"mode", "every", "n_checks", "n_changes", "dt_first", "dt_min", "dt_last", "omega_bound_0", "omega_bound_max",
                           "bound_over_lanczos_0"}
    assert follow["mode"] == "anchored" and follow["every"] == 10 and follow["n_checks"] == 4
    assert follow["dt_min"] <= follow["dt_first"] <= runs["plain"]["dt"] and follow["omega_bound_max"] >= follow["omega_bound_0"] > 0
    assert 1.0 < follow["bound_over_lanczos_0"] < 4.0
    assert runs["followed"]["dt_check"]["n_checks"] == 2 and runs["followed"]["dt_check"]["dt_over_dt_crit_max"] <= 1.0
    traj = rio.load_displacement(runs["followed"]["path"])
    with np.load(runs["followed"]["time_path"]) as z:
        t, step, dts = z["t"], z["step"], z["dt"]
    assert traj.shape[1] == 20 and len(t) == traj.shape[1] and (np.diff(t) > 0).all() and len(step) == len(dts) >= 1 and step[0] == 0
    assert abs(t[-1] - dd.per_step(list(zip(step, dts)), 40)[:39].sum()) <= 1e-12 and abs(runs["followed"]["tn"] - t[-1] - dts[-1]) < 1e-12
    # without the flag: the keys of old, no time file, and the trajectory of a stepper that is simply stepped
    assert set(runs["plain"]) == PLAIN_KEYS and not os.path.exists(os.path.join(str(tmp_path / "plain"), "Results", "Dynamics", "Time_order2.npz"))
    mesh = to_quadratic(structured_beam(2))
    with ModalOperator(mesh.points, np.asarray(mesh.tets10, dtype=np.int32), fs.node_to_dof(plane_nodes(mesh.points)), LMD, MU, fd.RHO) as op:
        mass = op.lumped_mass()
        ts = stable_time_step_operator(op, mass, 0.9)
        with OperatorStepper(op, mass, op.load((0.0, -50.0, -50.0)), ts["dt"], ALPHA, ramp=True, material="svk") as st:
            want = st.record(20, 2)
            st.step(40)
            want = want.cpu().numpy()
    assert ts["dt"] == runs["plain"]["dt"] and np.array_equal(rio.load_displacement(runs["plain"]["path"]), want)
