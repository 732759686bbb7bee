"""The finite-strain tangent without a GPU: the NumPy double of tests/tangent_double.py checked against itself (derivative of
the force, symmetry, the handle's K at u = 0, mpmath), every case of tests/test_gpu_tangent.py qualified, the new entry point
and the drivers' refusals, and the static problem of the Newton tests.

Bars.  ``K_T(u) v`` against the central difference of ``f_int`` in longdouble at ``h = 1e-6`` along ``v`` (``max|v| = 1``): the
statement of ``test_force_is_the_gradient_of_the_energy`` (tests/test_finite_strain.py) one derivative lower, with its step,
its norm (``max|.| / max|K_T v|``) and its bar 1e-8; measured 1.4e-11 .. 1.6e-10.  At ``h`` = 4e-3, 2e-3, 1e-3 the truncation
``h^2 f'''/6`` dominates and the discrepancy falls by 4 per halving (each ratio in [3.5, 4.5]).  Symmetry and the zero state hold
to 2^-58 in longdouble (eps 2^-63 and sums of a few hundred terms), the figure the reference is held to against mpmath."""
import ctypes as C

import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import operator_extended as ox
import tangent_double as td
from synchronization_avoiding_algorithms_amd import _lib

LMD, MU = fd.lame(fd.E, fd.NU)

SIGNATURE = (
    (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "int saa_operator_tangent_apply(saa_operator *op, int32_t material, const double *u_dev, const double *v_dev, "
    "double *kv_dev, int64_t *n_inverted /* host, or NULL */)")

MP_CASES = [("structured288", "strain", 0, 1e-8), ("curved288", "strain", 0, 0.3), ("delaunay2", "nu", 0.499999, 1e-6),
            ("beam36", "mindet", 1e-2, 0), ("structured288", "rotation", 0.5, 0.3), ("curved288", "shift", 20, 0.3),
            ("structured288", "sliver", 1e-6, 0.3), ("beam36", "curved", 0.2, 0.3)]


@pytest.fixture(scope="module")
def doubles():
    """name -> (Tangent clamped, u at max|H| = 0.3 with min det F >= 0.2, two directions with max|v| = 1)."""
    out = {}
    for k, name in enumerate(fd.MESHES):
        pts, cells, dd = fd.mesh(name)
        fs = td.Tangent(pts, cells, LMD, MU, dd)
        u, det, hmax = fd.scale_to_strain(fs, fd.smooth_random_field(pts, 40 + k), 0.3, 0.2)
        assert det >= 0.2 and abs(hmax - 0.3) < 1e-9, (name, det, hmax)
        rng = np.random.default_rng(70 + k)
        out[name] = (fs, u, rng.uniform(-1.0, 1.0, size=u.size), rng.uniform(-1.0, 1.0, size=u.size))
    return out


def _difference(fs, u, v, material, h):
    ul, vl, h = np.asarray(u, dtype=np.longdouble), np.asarray(v, dtype=np.longdouble), np.longdouble(h)
    return (fs.force(ul + h * vl, material) - fs.force(ul - h * vl, material)) / (2 * h)


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_tangent_is_the_derivative_of_the_force(doubles, name, material):
    fs, u, v, _ = doubles[name]
    kv = fs.tangent(u, v, material)
    top = np.abs(kv).max()
    worst = float(np.abs(_difference(fs, u, v, material, 1e-6) - kv).max() / top)
    coarse = [float(np.abs(_difference(fs, u, v, material, h) - kv).max() / top) for h in (4e-3, 2e-3, 1e-3)]
    print(name, material, "max |df/ds - K_T v| / max|K_T v| =", worst, "at h = 4e-3, 2e-3, 1e-3:", coarse,
          "ratios", coarse[0] / coarse[1], coarse[1] / coarse[2])
    assert worst <= 1e-8
    assert 3.5 <= coarse[0] / coarse[1] <= 4.5 and 3.5 <= coarse[1] / coarse[2] <= 4.5


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_tangent_is_symmetric_and_is_the_handles_operator_at_zero(doubles, name, material):
    fs, u, v, w = doubles[name]
    vm, wm = np.where(fs.free, v, 0.0), np.where(fs.free, w, 0.0)
    kv, kw = fs.tangent(u, v, material), fs.tangent(u, w, material)
    asym = float(abs((vm * kw).sum() - (wm * kv).sum()))
    scale = float(np.sqrt((vm * vm).sum()) * np.sqrt((kw * kw).sum()))
    zero = fs.tangent(np.zeros_like(u), v, material)
    lin = fs.linear_force(v)
    at_zero = float(np.abs(zero - lin).max() / np.abs(lin).max())
    print(name, material, "|v.Kw - w.Kv| / (|v| |Kw|) =", asym / scale, " max|K_T(0) v - K v| / max|K v| =", at_zero)
    assert asym <= 2.0 ** -58 * scale
    assert at_zero <= 2.0 ** -58


@pytest.mark.parametrize("cid", MP_CASES, ids=fx.case_name)
def test_longdouble_matches_mpmath_at_50_digits(cid):
    """Section 10's check for the tangent: four elements of every family, both materials and directions, to 2^-58 (the
    rotation family with ``max|H| = 0.3`` next to the rotation, as there)."""
    import mpmath

    case = td.sub_case(td.build_case(cid), 4)
    worst = {}
    with mpmath.workdps(50):
        for material in fd.MATERIALS:
            want, winv, _ = td.outputs(case, material, ox.MP)
            got, ginv, _ = td.outputs(case, material, np.longdouble)
            assert (winv == ginv).all()
            for name, w in want.items():
                worst[material, name] = float(np.abs(ox.conv(got[name], ox.MP) - w).max() / np.abs(w).max())
    print(fx.case_name(cid), {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= 2.0 ** -58, worst


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", td.case_ids(), ids=fx.case_name)
def test_the_bar_is_meaningful_on_this_case(cid, material):
    """The rule of tests/test_finite_strain_extended.py: the stable float64 restatement within ``1e-12 + 2 env``, ``env <= 1e-6``."""
    case, ref, env = td.reference(cid)
    got = td.outputs(case, material, np.float64)[0]
    _, bad = td.check({k: v[0] for k, v in got.items()}, cid, material, ox.STABLE_FACTOR)
    assert not bad, bad
    top = {k: float(v.max()) for k, v in env[material].items()}
    assert max(top.values()) <= ox.ENV_MAX, top


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("cid", td.unit_cases(), ids=fx.case_name)
def test_power_of_two_units_commute_bitwise_in_float64(cid, u):
    case = td.build_case(cid)
    scaled = td.scaled_case(case, u)
    for material in fd.MATERIALS:
        base, got = td.outputs(case, material, np.float64)[0], td.outputs(scaled, material, np.float64)[0]
        for name in td.DIRECTIONS:
            assert np.isfinite(got[name]).all() and np.abs(got[name]).max() < 1e290
            assert np.array_equal(got[name], base[name] * 2.0 ** (u * td.KV_UNIT_EXPONENT)), (material, name)


def test_inverted_elements_are_dropped_from_the_tangent():
    pts, cells, dd = fd.mesh("curved288")
    fs = td.Tangent(pts, cells, LMD, MU, dd)
    u, partial = fx.partial_inversion_state(fs, pts, 0.02 * fd.smooth_random_field(pts, 3))
    v = np.random.default_rng(5).uniform(-1.0, 1.0, size=u.size)
    kv, inv = fs.tangent_full(u, v, "neo_hookean")
    assert inv[partial].all() and (inv == fs.evaluate(u, "neo_hookean")[2]).all() and 0 < inv.sum() < len(cells)
    assert np.isfinite(np.asarray(kv, dtype=np.float64)).all()
    keep = np.nonzero(~inv)[0]
    rest = td.Tangent(pts, cells[keep], LMD, MU, dd)
    assert float(np.abs(rest.tangent(u, v, "neo_hookean") - kv).max()) <= 1e-17 * float(np.abs(kv).max())
    assert not fs.tangent_full(u, v, "svk")[1].any()


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", td.NEWTON_MESHES)
def test_the_load_of_the_newton_tests_has_a_solution_far_from_inversion(name, material):
    """The load of tests/test_gpu_tangent.py - the linear tip deflection is 0.25 of the beam length - in the double: its float64
    Newton with the dense tangent converges there with ``min det F > 0.5``, and the solution is not the linear one.  Measured:
    ``fz`` = 1773.0 (order 1) and 793.0 (order 2), ``min det F`` 0.87 .. 0.96, 17 .. 18 % from the linear solution in L2."""
    pts, cells, dd, fz, b, d_lin, _ = td.newton_problem(name)
    assert abs(td.tip_deflection(pts, cells, d_lin) / (pts[:, 0].max() - pts[:, 0].min()) - td.TIP_OVER_LENGTH) < 1e-12
    fs = td.Tangent(pts, cells, LMD, MU, dd, T=np.float64)
    u, res, its = td.newton(fs, b, material, tol=1e-11)
    det = float(fs.det_f(u).min())
    apart = float(np.linalg.norm(u - d_lin) / np.linalg.norm(d_lin))
    print(name, material, f"fz {fz:.6g} residual {res:.2e} after {its} iterations, min det F {det:.3f}, {apart:.3f} from the linear one")
    assert res <= 1e-10 and det > 0.5 and apart > 0.05


def test_library_exports_the_entry_point():
    lib = _lib.load()
    header = open(_lib.HEADER).read()
    name, (sig, text) = "saa_operator_tangent_apply", SIGNATURE
    assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert _lib.SIGNATURES[name] == sig
    decl = header[header.index("int " + name + "("):]
    assert " ".join(decl[:decl.index(";")].split()) == text
    assert _lib.SOURCES.index("saa_opfs.hip") < _lib.SOURCES.index("saa_optan.hip") < _lib.SOURCES.index("saa_api.cpp")
    from synchronization_avoiding_algorithms_amd import dynamics, modal, steady

    assert hasattr(modal.ModalOperator, "tangent_apply") and hasattr(steady, "newton_solve_operator")
    assert hasattr(dynamics.OperatorStepper, "stable_time_step")


def test_argument_checks_need_no_device():
    lib = _lib.load()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is looked at
    n = C.c_int64(0)
    for material in (-1, 3, 99):
        assert lib.saa_operator_tangent_apply(fake, material, fake, fake, fake, C.byref(n)) == _lib.SAA_E_ARG
        assert b"material" in lib.saa_last_error() and b"none of" in lib.saa_last_error()
    empty = C.c_void_p(0)
    for handle in (None, C.byref(empty)):
        assert lib.saa_operator_tangent_apply(handle, 1, fake, fake, fake, None) == _lib.SAA_E_ARG
        assert b"null handle" in lib.saa_last_error()


def test_newton_solve_refuses_the_linear_material():
    from synchronization_avoiding_algorithms_amd.steady import newton_solve_operator

    with pytest.raises(ValueError, match="steady_solve_operator"):
        newton_solve_operator(None, np.zeros(3), "linear")


@pytest.mark.parametrize("extra,message", ((["--material", "linear"], "the check is for --material svk or neo-hookean"),
                                           (["--material", "svk", "--parts", "2"], "only its share of the tangent")))
def test_driver_refuses_the_time_step_check(capsys, extra, message):
    from synchronization_avoiding_algorithms_amd import drivers

    with pytest.raises(SystemExit) as exc:
        drivers.main(["dynamics", "--synthetic", "1", "--dt-check-every", "5", *extra])
    assert exc.value.code != 0
    err = capsys.readouterr().err
    assert message in err and "Traceback" not in err


def test_run_dynamics_refuses_the_time_step_check_too():
    from synchronization_avoiding_algorithms_amd.dynamics import run_dynamics

    with pytest.raises(ValueError, match="nonlinear material"):
        run_dynamics(np.zeros((4, 3)), np.zeros((1, 4), dtype=np.int32), [], 10, dt_check_every=5)
    with pytest.raises(ValueError, match="partition"):
        run_dynamics(np.zeros((4, 3)), np.zeros((1, 4), dtype=np.int32), [], 10, material="svk", epart=np.zeros(1), dt_check_every=5)


def test_driver_steady_state_takes_a_material(monkeypatch, capsys):
    import json

    from synchronization_avoiding_algorithms_amd import drivers

    seen = {}

    def fake(mesh, out_dir, **kw):
        seen.update(kw, n_elems=len(mesh.tets))
        return "somewhere.vtk", None, {"converged": True}

    monkeypatch.setattr(drivers, "steady_state_nonlinear", fake)
    drivers.main(["steady_state", "--synthetic", "1", "--order", "2", "--material", "svk", "--fz", "12.5", "--load-steps", "3"])
    assert seen["material"] == "svk" and seen["order"] == 2 and seen["fz"] == 12.5 and seen["load_steps"] == 3
    assert json.loads(capsys.readouterr().out) == {"converged": True, "path": "somewhere.vtk"}

    def failing(mesh, out_dir, **kw):
        raise drivers.NotConverged("Newton stopped", {"converged": False})

    monkeypatch.setattr(drivers, "steady_state_nonlinear", failing)
    with pytest.raises(SystemExit) as exc:
        drivers.main(["steady_state", "--synthetic", "1", "--material", "neo-hookean"])
    assert exc.value.code not in (0, None) and "Newton stopped" in str(exc.value.code)
