"""Following the time step at finite strain, on the CPU: the double of tests/dt_follow_double.py is qualified here - its bound
against the dense ``omega_max`` of ``M_L^-1 K_T`` and against the host formula of ``saa_operator_element_bound``, its change of
step against the velocity form of the variable-step scheme, the scenario that motivates the feature - and the pieces of the
product that need no GPU: the two signatures and the driver's refusals."""
import ctypes as C

import numpy as np
import pytest

import dt_follow_double as dd
import finite_strain_double as fd

MATERIALS = ("svk", "neo_hookean")


@pytest.mark.parametrize("name", fd.MESHES)
def test_the_bound_is_a_bound(name):
    pts, cells, dofs, fs = dd.problem(name)
    for st in dd.STATES:
        u = dd.state(st, pts, fs)
        for material in MATERIALS:
            b = fs.bound(u, material)
            dense = fs.omega_dense(u, material)
            print(f"{name:14s} {st:7s} {material:12s} bound / dense {b['omega_max'] / dense:.4f}")
            assert b["n_nonpositive"] == 0 and b["n_inverted"] == 0 and b["n_nonfinite"] == 0
            assert b["omega_max"] >= dense, (name, st, material, b["omega_max"], dense)


@pytest.mark.parametrize("name", ("structured288", "delaunay2"))
def test_at_order_1_and_rest_it_is_the_element_bound(name):
    from synchronization_avoiding_algorithms_amd import modal

    pts, cells, dofs, fs = dd.problem(name)
    want = modal.element_omega(pts, cells, *fd.lame(fd.E, fd.NU), fd.RHO)[0]
    for material in ("linear",) + MATERIALS:
        got = fs.omega_e(np.zeros(3 * len(pts)), material)["omega_e"]
        assert np.abs(got - want).max() <= 1e-12 * want.max(), (name, material)


@pytest.mark.parametrize("name,material", (("structured288", "neo_hookean"), ("beam36", "svk")))
def test_the_replaced_dn_continues_the_variable_step_scheme(name, material):
    """Three changes of step: constant-step updates with ``dn'`` in the place of ``dn`` against ``run_variable``, which never forms
    it, to 1e-13 of ``max|d|``."""
    fs, live, mass, load, u, dt, _ = dd.release_problem(name, material, strain=0.1)
    alpha = 0.5
    load = 1e-3 * mass                                                 # some load, so that the ramp factor matters
    force = lambda d: np.asarray(fs.force(d, material), dtype=np.float64)  # noqa: E731
    plan = [(0.5 * dt, 4), (0.8 * dt, 3), (0.45 * dt, 5), (0.6 * dt, 4)]   # the first entry is the step the state was made with
    small = 1e-3 * fd.smooth_random_field(fs.points64, 5) * live
    d0, dn, tn, now = u.copy(), u - small, 0.3, plan[0][0]
    a0, an = d0.copy(), dn.copy()
    dts = []
    for dt_k, n in plan:
        if dt_k != now:
            dn = dd.set_dt(force(d0), mass, load, live, d0, dn, now, dt_k, alpha, min(tn, 1.0))
            now = dt_k
        d0, dn, tn = fd.run(force, mass, load, live, now, alpha, True, n, d0, dn, tn)
        dts += [dt_k] * n
    want, _, tw = dd.run_variable(dts, force, mass, load, live, alpha, True, a0, an, plan[0][0], 0.3)
    err = float(np.abs(d0 - want).max() / np.abs(want).max())
    print(f"{name} {material}: dn' route against the velocity form, {err:.2e}")
    assert abs(tn - tw) < 1e-15 and err <= 1e-13


@pytest.mark.parametrize("name", ("structured288", "beam36"))
@pytest.mark.parametrize("material", MATERIALS)
def test_the_fixed_step_blows_up_and_the_followed_step_does_not(name, material):
    """The release at rest from the 0.3-strain state with ``dt = 0.9 * 2/omega_max`` of the linear operator, 40 steps."""
    fs, live, mass, load, u, dt, omega_l = dd.release_problem(name, material)
    assert np.abs(u).max() < 0.4
    top = dd.followed_run(fs, material, live, mass, load, u, dt, omega_l, "anchored", fixed=True)[4]
    print(f"{name} {material}: fixed dt, max|d| {top:.3g}")
    assert not top < 1.0
    for mode in ("anchored", "certified"):
        _, changes, worst, inverted, top = dd.followed_run(fs, material, live, mass, load, u, dt, omega_l, mode)
        print(f"{name} {material} {mode}: worst dt/dt_crit {worst:.3f}, max|d| {top:.3f}, {len(changes)} values of dt")
        assert worst <= 1.0 and inverted == 0 and top < 1.0
        if mode == "anchored":                                         # never above the linear operator's step
            assert all(c[1] <= dt for c in changes)


def test_the_binding_has_both_entries():
    from synchronization_avoiding_algorithms_amd import _lib, dynamics, modal

    sig = _lib.SIGNATURES
    assert sig["saa_operator_tangent_bound"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                           C.POINTER(C.c_int32), C.POINTER(C.c_int64)])
    assert sig["saa_operator_stepper_set_dt"] == (C.c_int, [C.c_void_p, C.c_double])
    assert hasattr(modal.ModalOperator, "tangent_bound")
    assert all(hasattr(dynamics.OperatorStepper, m) for m in ("set_dt", "follow_time_step"))


def test_the_entries_check_their_arguments_before_the_device():
    from synchronization_avoiding_algorithms_amd import _lib

    lib = _lib.load()
    fake = C.c_void_p(8)
    w, arg = C.c_double(), C.c_int32()
    for material in (-1, 3):
        assert lib.saa_operator_tangent_bound(fake, material, fake, None, C.byref(w), C.byref(arg), None) == _lib.SAA_E_ARG
        assert b"material" in lib.saa_last_error()
    assert lib.saa_operator_tangent_bound(None, 1, fake, None, C.byref(w), C.byref(arg), None) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error()
    assert lib.saa_operator_stepper_set_dt(None, 1.0) == _lib.SAA_E_ARG and b"null handle" in lib.saa_last_error()


@pytest.mark.parametrize("extra,message", ((["--material", "linear"], "following the step is for --material svk or neo-hookean"),
                                           (["--material", "svk", "--parts", "2"], "only its share of the internal force"),
                                           (["--material", "svk", "--energy"], "energy balance")))
def test_driver_refuses_to_follow(capsys, extra, message):
    from synchronization_avoiding_algorithms_amd import drivers

    with pytest.raises(SystemExit) as exc:
        drivers.main(["dynamics", "--synthetic", "1", "--dt-follow", "anchored", *extra])
    assert exc.value.code != 0
    err = capsys.readouterr().err
    assert message in err and "Traceback" not in err
    assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_run_dynamics_refuses_to_follow_too():
    from synchronization_avoiding_algorithms_amd.dynamics import run_dynamics

    pts, cells, dofs = fd.mesh("structured288")
    nodes = np.unique(dofs // 3)
    for kw, message in (({"material": "linear"}, "nonlinear material"), ({"material": "svk", "epart": np.zeros(len(cells), int)}, "partition"),
                        ({"material": "svk", "dt_follow": "sharp"}, "certified"), ({"material": "svk", "dt_follow_every": 0}, ">= 1")):
        with pytest.raises(ValueError, match=message):
            run_dynamics(pts, cells, nodes, 10, **{"dt_follow": "anchored", **kw})
