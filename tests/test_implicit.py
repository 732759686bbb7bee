"""The implicit stepper without a GPU: the NumPy double of tests/implicit_double.py is qualified against closed forms and
against the explicit double, the nonlinear case of the GPU tests is shown to be nonlinear and insensitive to the Newton
tolerance, and the C ABI, the bindings and the driver's refusals are checked.

Measured with the double on the CPU (``structured288`` / ``beam36``, 351 dofs each, ``dt_crit`` 2.86e-4 / 2.25e-4, first period
0.175 / 0.223):

* exact discrete frequency, 40 steps, of ``max|phi| = 1``: lowest mode at ``50 dt_crit`` 3.7e-11 / 6.0e-13, middle mode at ``5
  dt_crit`` 5.3e-14 / 1.3e-13, highest mode at ``3 dt_crit`` 4.5e-14 / 5.9e-14;
* energy, 50 steps at ``20 dt_crit``: ``max|B_n - B_0| / max U`` 3.4e-13 / 6.4e-13;
* second order against the explicit double on ``structured288`` (200 explicit steps of 0.876 ``dt_crit`` to ``t = 0.05``): 1.02e-5,
  3.81e-5, 1.30e-4, 4.16e-4 of ``max|d|`` at 1, 2, 4, 8 times the explicit step, ratios 3.74, 3.41, 3.20.  On ``beam36`` the
  differences are 1.76e-5, 2.67e-5, 6.01e-5, 2.07e-4: the explicit double's own error, which the first entry mostly is, is not
  small against the implicit one's at 1 and 2 there, so the ratios say nothing and the mesh is not used;
* the nonlinear case (bend of 0.5 rad, ``fz = 200``, ``alpha = 0.5``, ``5 dt_crit``, 12 steps), svk / neo-Hooke: ``max|H|`` 0.429 /
  0.432 and 0.451 / 0.452 during the run, ``min det F`` 0.919 / 0.932 and 0.951 / 0.956, 3 to 6 Newton iterations per step at ``tol =
  1e-10`` (4 to 7 at 1e-13); of ``max|d|``, ``tol = 1e-10`` against 1e-13 at most 4.2e-12 and ``tol = 1e-8`` against 1e-13 at most
  3.7e-10."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import finite_strain_double as fd
import implicit_double as imp

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_double_has_the_exact_discrete_frequency(name):
    """Linear, undamped, unloaded, from ``d = phi_j``, ``v = 0``: the trapezoidal rule turns the mode by ``theta = 2 atan(omega_j dt /
    2)`` per step, exactly.  The bar is that of the GPU test with the direct solve's ``eps`` for the tolerance: ``10 N eps kappa``."""
    p = imp.problem(name)
    for j, factor in imp.modal_cases(p):
        dt = factor * p.dt_crit
        nm = imp.Newmark(p, p.mass, np.zeros(p.n), dt, 0.0, ramp=False)
        nm.set_state(p.mode(j))
        assert nm.step(imp.MODAL_STEPS)["converged"]
        err = float(np.abs(nm.d - imp.modal_exact(p, j, dt, imp.MODAL_STEPS)).max())
        bar = 10 * imp.MODAL_STEPS * EPS * imp.modal_kappa(p, dt)
        print(f"{name} mode {j} at {factor} dt_crit: error {err:.2e} of max|phi|, bar {bar:.2e}")
        assert err <= bar


@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_double_conserves_the_energy_of_a_loaded_linear_run(name):
    """Constant load ``fz = 0.5``, undamped, ``dt = 20 dt_crit``, 50 steps from rest: ``T + U - f . d`` is constant for the trapezoidal
    rule.  Bar: 50 steps, each solved to ``eps kappa``, times the 20 the GPU test allows."""
    p = imp.problem(name)
    dt = 20.0 * p.dt_crit
    nm = imp.Newmark(p, p.mass, p.load(0.5), dt, 0.0, ramp=False)
    nm.set_state()
    b, u = [nm.energy()], [0.0]
    for _ in range(50):
        nm.step(1)
        b.append(nm.energy())
        u.append(0.5 * float(nm.d @ (p.K @ nm.d)))
    drift = float(np.abs(np.array(b) - b[0]).max() / max(u))
    bar = 50 * 20 * EPS * imp.modal_kappa(p, dt)
    print(f"{name}: energy drift {drift:.2e} of the largest U, bar {bar:.2e}")
    assert max(u) > 0 and drift <= bar


def test_double_is_second_order_against_the_explicit_double():
    p = imp.problem("structured288")
    load, dt, n = imp.second_order_case(p)
    want = imp.explicit_run(p, load, dt, n)
    diffs = []
    for f in imp.SECOND_ORDER_FACTORS:
        nm = imp.Newmark(p, p.mass, load, f * dt, 0.5, ramp=True)
        nm.set_state()
        assert nm.step(n // f)["converged"] and abs(nm.t - imp.SECOND_ORDER_END) < 1e-12
        diffs.append(float(np.abs(nm.d - want).max() / np.abs(want).max()))
    print("implicit - explicit of max|d| at 1, 2, 4, 8 explicit steps:", diffs, "ratios", [b / a for a, b in zip(diffs, diffs[1:])])
    for a, b in zip(diffs, diffs[1:]):
        assert 3.0 <= b / a <= 4.5


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_nonlinear_case_is_nonlinear_and_insensitive_to_the_tolerance(name, material):
    p = imp.problem(name)
    seen = {"h": 0.0, "det": np.inf}

    def watch(x):
        seen["h"] = max(seen["h"], float(np.abs(p.fs.gradient(x)).max()))
        seen["det"] = min(seen["det"], float(p.fs.det_f(x).min()))

    ref = imp.nonlinear_run(p, material, 1e-13, watch=watch)
    assert np.array_equal(ref.d, imp.nonlinear_reference(name, material))
    fine, coarse = imp.nonlinear_run(p, material, 1e-10), imp.nonlinear_run(p, material, 1e-8)
    scale = float(np.abs(ref.d).max())
    s10, s8 = float(np.abs(fine.d - ref.d).max()) / scale, float(np.abs(coarse.d - ref.d).max()) / scale
    print(f"{name} {material}: max|H| {seen['h']:.3f} min det F {seen['det']:.3f} Newton per step {fine.newton_per_step}; "
          f"tol 1e-10 vs 1e-13 {s10:.2e}, 1e-8 vs 1e-13 {s8:.2e}")
    assert seen["h"] >= 0.3 and seen["det"] > 0.5
    assert s10 <= 4 * 2.2e-11 and s8 <= 4 * 5.2e-9


def test_double_refuses_a_step_and_keeps_the_state():
    p = imp.problem("structured288")
    nm = imp.Newmark(p, p.mass, p.load(200.0), 5.0 * p.dt_crit, 0.5, ramp=False, material="svk", max_newton=1)
    nm.set_state(imp.nonlinear_start(p))
    before = (nm.d.copy(), nm.v.copy(), nm.a.copy(), nm.t)
    info = nm.step(3)
    assert (info["reason"], info["steps_done"], info["converged"]) == (1, 0, False)
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], (nm.d, nm.v, nm.a))) and nm.t == before[3]


# ---- the C ABI and the bindings -----------------------------------------------------------------------------------------------

NAMES = ("saa_operator_shifted_apply", "saa_operator_implicit_create", "saa_operator_implicit_destroy",
         "saa_operator_implicit_set_state", "saa_operator_implicit_get_state", "saa_operator_implicit_set_recorder",
         "saa_operator_implicit_set_option", "saa_operator_implicit_set_dt", "saa_operator_implicit_step")


def test_entry_points_are_declared_bound_and_exported():
    from synchronization_avoiding_algorithms_amd import _lib

    header = open(os.path.join(REPO, "include", "saa_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
        decl = re.search(r"\bint " + name + r"\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "saa_opimp.hip" in _lib.SOURCES and _lib.ABI_VERSION == lib.saa_abi_version()
    assert C.sizeof(_lib.ImplicitInfo) == 40
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    for m in ("step", "state", "set_state", "record", "set_dt", "set_option", "__enter__", "__exit__"):
        assert callable(getattr(ImplicitStepper, m))
    assert callable(ModalOperator.shifted_apply)


def test_arguments_are_refused_before_the_device_is_touched():
    from synchronization_avoiding_algorithms_amd import _lib

    lib = _lib.load()
    h, info, n_inv = C.c_void_p(), _lib.ImplicitInfo(), C.c_int64()
    one = C.c_void_p(8)                                               # never dereferenced: the checks come first

    def refused(rc, text):
        assert rc == _lib.SAA_E_ARG and text in lib.saa_last_error().decode(), (rc, lib.saa_last_error())

    refused(lib.saa_operator_shifted_apply(None, 7, None, one, None, one, None, C.byref(n_inv)), "material 7")
    refused(lib.saa_operator_shifted_apply(None, 1, one, one, None, one, None, None), "null handle")
    refused(lib.saa_operator_implicit_create(None, one, one, 0.0, 0.5, 1, 0, C.byref(h)), "dt must be finite and > 0")
    refused(lib.saa_operator_implicit_create(None, one, one, 1e-3, -1.0, 1, 0, C.byref(h)), "alpha must be finite and >= 0")
    refused(lib.saa_operator_implicit_create(None, one, one, 1e-3, 0.5, 1, 3, C.byref(h)), "material 3")
    refused(lib.saa_operator_implicit_create(None, one, one, 1e-3, 0.5, 1, 0, C.byref(h)), "null handle")
    refused(lib.saa_operator_implicit_create(None, one, one, 1e-3, 0.5, 1, 0, None), "null output")
    assert not h.value
    refused(lib.saa_operator_implicit_step(None, 1, C.byref(info)), "null handle")
    refused(lib.saa_operator_implicit_set_state(None, None, None, 0.0), "null handle")
    refused(lib.saa_operator_implicit_get_state(None, None, None, None, None), "null handle")
    refused(lib.saa_operator_implicit_set_recorder(None, None, 0, 1, 0), "null handle")
    refused(lib.saa_operator_implicit_set_option(None, b"tol", 1e-8), "null handle")
    refused(lib.saa_operator_implicit_set_dt(None, 1e-3), "null handle")
    assert lib.saa_operator_implicit_destroy(None) == _lib.SAA_OK


# ---- the driver ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", (["--parts", "2"], ["--energy"], ["--material", "svk", "--dt-follow", "certified"],
                                   ["--material", "svk", "--dt-check-every", "5"]))
def test_driver_refuses_what_the_implicit_run_does_not_provide(flags, tmp_path):
    cmd = [sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "dynamics", "--scheme", "newmark",
           "--synthetic", "2", "--steps", "4", "--out", str(tmp_path), *flags]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--scheme newmark " + flags[-2 if len(flags) > 1 else -1] in out.stderr, out.stderr[-400:]
    assert not os.listdir(tmp_path)


def test_driver_function_refuses_the_same_combinations():
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(1)
    for kw in ({"parts": 2}, {"energy_every": 1}, {"dt_follow": "certified", "material": "svk"},
               {"dt_check_every": 5, "material": "svk"}):
        with pytest.raises(ValueError, match="newmark"):
            drivers.dynamics(mesh, 4, scheme="newmark", **kw)
    with pytest.raises(ValueError, match="scheme"):
        drivers.dynamics(mesh, 4, scheme="hht")
