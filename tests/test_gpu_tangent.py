"""The matrix-free finite-strain tangent ``saa_operator_tangent_apply`` (``csrc/saa_optan.hip``) and what is built on it - the
Newton-PCG static solve, the stable time step at a state - on the MI355X, against the double of tests/tangent_double.py.

Parity: the cases of ``tangent_double.case_ids`` (tests/test_tangent.py qualifies every one on the CPU), two directions each,
both materials, to the bar of tests/test_gpu_finite_strain_extended.py: ``err = max|y - r| / max|r| <= 1e-12 + 8 env``.  Units:
bitwise.  The meshes have at most 288 elements, except those of the two driver runs, which the drivers build themselves."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import operator_extended as ox
import tangent_double as td

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = fd.lame(fd.E, fd.NU)
TOL = 1e-10                                                            # newton_solve_operator's default
# fz at which the LINEAR tip deflection of `--synthetic 2 --order 2` (the 50 x 2 x 2 beam of length 25) is 0.25 of its length:
# 0.25 * 25 / (tip deflection per unit fz, 0.5833673364, which `steady_state --material` prints as linear.tip_deflection / fz)
DRIVER_FZ = 10.71366120409606


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(t):
    return t.cpu().numpy()


def _operator(case):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(case["points"], np.asarray(case["cells"]).astype(np.int32), np.asarray(case["dd"]).astype(np.int32),
                         case["lmd"], case["mu"], fd.RHO)


def gpu_outputs(case, material):
    """``({direction: kv}, n_inverted)``."""
    with _operator(case) as op:
        u = _dev(case["u"])
        out, n_inv = {}, 0
        for d in td.DIRECTIONS:
            kv, n = op.tangent_apply(u, _dev(case["v_" + d]), material, count=True)
            out[d], n_inv = _host(kv), max(n_inv, n)
        return out, n_inv


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", td.case_ids(), ids=fx.case_name)
def test_tangent_is_within_the_bar(cid, material):
    case, _, _ = td.reference(cid)
    got, n_inv = gpu_outputs(case, material)
    assert n_inv == 0
    _, bad = td.check(got, cid, material, ox.KERNEL_FACTOR)
    assert not bad, bad
    for d in td.DIRECTIONS:
        assert not got[d][case["dd"]].any()


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", td.unit_cases(), ids=fx.case_name)
def test_power_of_two_units_commute_bitwise(cid, material, u):
    case = td.build_case(cid)
    scaled = td.scaled_case(case, u)
    ref = td.outputs(scaled, material)[0]                             # no overflow or underflow in the reference first
    for name, r in ref.items():
        r = np.asarray(r, dtype=np.float64)
        assert np.isfinite(r).all() and (np.abs(r[r != 0]) > 1e-290).all() and np.abs(r).max() < 1e290, name
    (base, n0), (got, n1) = gpu_outputs(case, material), gpu_outputs(scaled, material)
    assert n0 == 0 and n1 == 0
    for d in td.DIRECTIONS:
        assert np.array_equal(got[d], base[d] * 2.0 ** (u * td.KV_UNIT_EXPONENT)), (d, int((got[d] != base[d] * 2.0 ** (u * td.KV_UNIT_EXPONENT)).sum()))


# ---- launch edges -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_elems", (1, 255, 256, 257))
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_launch_edges_and_the_canary_after_kv(name, n_elems):
    """The first ``n_elems`` elements of the 288-element fixtures as meshes of their own: one element, and one below, at and one
    above the 256 lanes of the element pass's workgroup.  Same bar; 64 doubles after ``kv`` keep their sentinel."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    case = td.sub_case(td.build_case((name, "strain", 0, 0.3)), n_elems)
    assert len(case["cells"]) == n_elems
    sentinel = -7.25e300
    for material in fd.MATERIALS:
        ref, inv, _ = td.outputs(case, material)
        assert not inv.any()
        env = td.envelope(case, ref, lambda c: td.outputs(c, material)[0])
        with _operator(case) as op:
            got = {}
            for d in td.DIRECTIONS:
                buf = torch.full((op.n_dof + 64,), sentinel, dtype=torch.float64, device="cuda")
                u, v = _dev(case["u"]), _dev(case["v_" + d])
                _lib.check(op._lib.saa_operator_tangent_apply(op._h, _lib.material_id(material), C.c_void_p(u.data_ptr()),
                                                              C.c_void_p(v.data_ptr()), C.c_void_p(buf.data_ptr()), None))
                torch.cuda.synchronize()
                assert bool((buf[op.n_dof:] == sentinel).all()), (material, d)
                got[d] = _host(buf[:op.n_dof])[None]
        _, bad = ox.check(got, ref, env, ox.KERNEL_FACTOR, f"{name}[:{n_elems}] {material}", names=list(td.DIRECTIONS))
        assert not bad, bad


# ---- linear material, symmetry, repeatability ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fd.MESHES)
def test_linear_material_is_the_apply_bit_for_bit(name):
    import torch

    case = td.build_case((name, "strain", 0, 0.3))
    with _operator(case) as op:
        v = _dev(case["v_random"])
        want = op.apply(v)[0]
        assert torch.equal(op.tangent_apply(None, v, "linear"), want)
        kv, n = op.tangent_apply(_dev(case["u"]), v, "linear", count=True)
        assert torch.equal(kv, want) and n == 0
        with pytest.raises(ValueError):
            op.tangent_apply(None, v, "svk")


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_tangent_is_symmetric_and_repeatable_on_the_device(name, material):
    import torch

    cid = (name, "strain", 0, 0.3)
    case, _, env = td.reference(cid)
    bar = ox.TOL + ox.KERNEL_FACTOR * float(max(e.max() for e in env[material].values()))
    with _operator(case) as op:
        u, v, w = _dev(case["u"]), _dev(case["v_random"]) * op.free, _dev(case["v_smooth"]) * op.free
        kv, kw = op.tangent_apply(u, v, material), op.tangent_apply(u, w, material)
        assert torch.equal(kv, op.tangent_apply(u, v, material)) and torch.equal(kw, op.tangent_apply(u, w, material))
        asym = abs(float(torch.dot(v, kw)) - float(torch.dot(w, kv)))
        scale = float(torch.linalg.vector_norm(v) * torch.linalg.vector_norm(kw))
    print(name, material, f"|v.Kw - w.Kv| / (|v| |Kw|) = {asym / scale:.2e}, allowed {2 * bar:.2e}")
    assert asym <= 2.0 * bar * scale


# ---- inversion ----------------------------------------------------------------------------------------------------------------

def test_inverted_elements_are_dropped_and_counted():
    pts, cells, dd = fd.mesh("curved288")
    fs = td.Tangent(pts, cells, LMD, MU, dd)
    u, partial = fx.partial_inversion_state(fs, pts, 0.02 * fd.smooth_random_field(pts, 3))
    case = {"points": pts, "cells": cells, "dd": dd, "lmd": LMD, "mu": MU, "u": u,
            "v_random": np.random.default_rng(5).uniform(-1.0, 1.0, size=u.size), "v_smooth": fd.smooth_random_field(pts, 6)}
    ref, inv, _ = td.outputs(case, "neo_hookean")
    assert inv[partial].all() and 0 < inv.sum() < len(cells)

    def outputs_of(c):
        out, alt_inv, _ = td.outputs(c, "neo_hookean")
        assert (alt_inv == inv).all()
        return out

    env = td.envelope(case, ref, outputs_of)
    got, n_inv = gpu_outputs(case, "neo_hookean")
    print("partially inverted", list(partial), "inverted in all", int(inv.sum()), "n_inverted", n_inv)
    assert n_inv == int(inv.sum())
    for d in td.DIRECTIONS:
        assert np.isfinite(got[d]).all()
    _, bad = ox.check({d: got[d][None] for d in td.DIRECTIONS}, ref, env, ox.KERNEL_FACTOR, "curved288 partial inversion",
                      names=list(td.DIRECTIONS))
    assert not bad, bad
    svk, n_svk = gpu_outputs(case, "svk")
    assert n_svk == 0 and np.isfinite(svk["random"]).all()


# ---- the stable time step at a state ------------------------------------------------------------------------------------------

def _dense_omega(fs64, u, material, mass):
    free = np.nonzero(fs64.free & (mass > 0))[0]
    s = 1.0 / np.sqrt(mass[free])
    A = fs64.tangent_matrix(u, material)[np.ix_(free, free)] * s[:, None] * s[None, :]
    return float(np.sqrt(np.linalg.eigvalsh(0.5 * (A + A.T))[-1]))


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", td.NEWTON_MESHES)
def test_stable_time_step_at_a_state(name, material):
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    pts, cells, dd = fd.mesh(name)
    fs64 = td.Tangent(pts, cells, LMD, MU, dd, T=np.float64)
    stretched = td.stretched_state(pts, fs64)
    with ModalOperator(pts, cells.astype(np.int32), dd.astype(np.int32), LMD, MU, fd.RHO) as op:
        mass = op.lumped_mass()
        linear = stable_time_step_operator(op, mass)
        assert set(linear) == {"omega_max", "dt_crit", "dt"}
        zero = stable_time_step_operator(op, mass, material=material, state=torch.zeros(op.n_dof, dtype=torch.float64, device="cuda"))
        there = stable_time_step_operator(op, mass, material=material, state=_dev(stretched))
        assert set(there) == {"omega_max", "dt_crit", "dt", "material", "n_inverted", "lanczos_residual"}
        assert there["material"] == material and there["n_inverted"] == 0 and zero["n_inverted"] == 0
        with OperatorStepper(op, mass, op.load((0.0, -0.5, -0.5)), linear["dt"], 0.5, material=material) as st:
            st.set_state(_dev(stretched), _dev(stretched))
            from_stepper = st.stable_time_step()
        m = _host(mass)
    dense_zero, dense_there = _dense_omega(fs64, np.zeros_like(stretched), material, m), _dense_omega(fs64, stretched, material, m)
    print(name, material, f"omega_max linear {linear['omega_max']:.10g} at 0 {zero['omega_max']:.10g} (dense {dense_zero:.10g}) "
          f"stretched {there['omega_max']:.10g} (dense {dense_there:.10g}), ratio {there['omega_max'] / linear['omega_max']:.6f}")
    assert abs(zero["omega_max"] / dense_zero - 1.0) <= 1e-8 and abs(there["omega_max"] / dense_there - 1.0) <= 1e-8
    assert abs(zero["omega_max"] / linear["omega_max"] - 1.0) <= 1e-8
    assert abs(dense_there / dense_zero - 1.0) > 1e-3                 # the state moves the limit ...
    assert abs((there["omega_max"] / linear["omega_max"]) / (dense_there / dense_zero) - 1.0) <= 2e-8   # ... by the dense ratio
    assert there["dt_crit"] == 2.0 / there["omega_max"] and there["dt"] == 0.9 * there["dt_crit"]
    assert from_stepper["omega_max"] == there["omega_max"] and from_stepper["dt"] == linear["dt"]
    assert from_stepper["dt_over_dt_crit"] == linear["dt"] / there["dt_crit"]


# ---- the Newton solve ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", td.NEWTON_MESHES)
def test_newton_solve(name, material):
    """The load of ``tangent_double.newton_problem`` (linear tip deflection 0.25 of the length; tests/test_tangent.py shows that
    the double's Newton converges there with ``min det F > 0.5``)."""
    import torch

    from synchronization_avoiding_algorithms_amd.modal import ModalOperator
    from synchronization_avoiding_algorithms_amd.steady import newton_solve_operator, steady_solve_operator

    pts, cells, dd, fz, _, d_lin_double, _ = td.newton_problem(name)
    f64 = td.Tangent(pts, cells, LMD, MU, dd, T=np.float64)
    with ModalOperator(pts, cells.astype(np.int32), dd.astype(np.int32), LMD, MU, fd.RHO) as op:
        load = op.load((0.0, -fz, -fz))
        b = _host(load)
        bn = float(np.linalg.norm(b))
        d_lin, _, _ = steady_solve_operator(op, load)
        u, info = newton_solve_operator(op, load, material)
        u4, info4 = newton_solve_operator(op, load, material, load_steps=4)
        print(name, material, f"fz {fz:.6g}: {info['newton_iterations']} Newton / {info['cg_iterations']} CG iterations, residual "
              f"{info['residual']:.2e}; in 4 load steps {info4['newton_iterations']} / {info4['cg_iterations']}, {info4['residual']:.2e}")
        assert info["converged"] and info4["converged"] and info["n_inverted"] == 0 and info["load_steps"] == 1
        assert len(info["residual_history"]) == info["newton_iterations"]

        def look(x):
            f, en, n_inv = op.internal_force(_dev(x), material, energy=True)
            return float(torch.linalg.vector_norm((load - f) * op.free)) / bn, float(en.sum()) - float(b @ x), n_inv

        res, phi, n_inv = look(u)
        res4 = look(u4)[0]
        assert res <= TOL and res4 <= TOL and n_inv == 0
        assert phi < look(d_lin)[1]                                   # lower than the linear solution in Pi(u) - b.u
    assert float(np.linalg.norm(d_lin - d_lin_double) / np.linalg.norm(d_lin_double)) < 1e-6   # (the load is the double's)
    independent = float(np.linalg.norm(np.where(f64.free, b - np.asarray(f64.force(u, material), dtype=np.float64), 0.0))) / bn
    apart = float(np.linalg.norm(u - d_lin) / np.linalg.norm(d_lin))
    free = np.nonzero(f64.free)[0]
    cond = float(np.linalg.cond(f64.tangent_matrix(u, material)[np.ix_(free, free)]))
    same = float(np.linalg.norm(u - u4) / np.linalg.norm(u))
    print(name, material, f"residual in the double's float64 force {independent:.2e}; {apart:.3f} from the linear solution; one "
          f"load step against four {same:.2e}, cond(K_T) {cond:.3g}, allowed {2 * TOL * cond:.2e}; min det F {float(f64.det_f(u).min()):.3f}")
    assert independent <= 2 * TOL
    assert apart > 100 * TOL
    assert same <= 2 * TOL * cond


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", td.NEWTON_MESHES)
def test_newton_solution_approaches_the_linear_one_at_small_loads(name, material):
    """The project's linearisation check: at two loads that strain the beam by about 1e-4 and half that, ``|u_nl - u_lin| /
    |u_lin|`` halves.  Newton to 1e-11: what it leaves in ``u`` (at most that times cond(K) = 1e5) is 1 % of the difference."""
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator
    from synchronization_avoiding_algorithms_amd.steady import newton_solve_operator, steady_solve_operator

    pts, cells, dd, fz, _, d_lin_double, _ = td.newton_problem(name)
    f64 = td.Tangent(pts, cells, LMD, MU, dd, T=np.float64)
    small = 1e-4 / float(np.abs(f64.gradient(d_lin_double)).max())
    rel = []
    with ModalOperator(pts, cells.astype(np.int32), dd.astype(np.int32), LMD, MU, fd.RHO) as op:
        for factor in (small, 0.5 * small):
            load = op.load((0.0, -fz * factor, -fz * factor))
            d_lin, _, _ = steady_solve_operator(op, load)
            u, info = newton_solve_operator(op, load, material, tol=1e-11)
            assert info["converged"], info
            rel.append(float(np.linalg.norm(u - d_lin) / np.linalg.norm(d_lin)))
    print(name, material, "relative differences", rel, "ratio", rel[0] / rel[1])
    assert 1.9 <= rel[0] / rel[1] <= 2.1


# ---- the drivers, one subprocess each -----------------------------------------------------------------------------------------

def _driver(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=str(cwd),
                          capture_output=True, text=True, timeout=300, env=env)


def test_driver_steady_state_with_a_material(tmp_path):
    out = _driver(["steady_state", "--synthetic", "2", "--order", "2", "--material", "svk", "--fz", repr(DRIVER_FZ), "--out",
                   str(tmp_path)], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["converged"] is True and res["order"] == 2 and res["material"] == "svk" and res["residual"] <= 1e-8   # (the driver's tolerance)
    assert abs(res["linear"]["tip_deflection"] / 25.0 - 0.25) < 0.01   # DRIVER_FZ is that load
    assert 0 < res["tip_deflection"] < res["linear"]["tip_deflection"]
    text = open(os.path.join(str(tmp_path), "Results", "Static", "steady_distributed.vtk")).read()
    types = text[text.index("CELL_TYPES"):text.index("POINT_DATA")].split()[2:]
    assert len(types) == res["n_elems"] and set(types) == {"24"}


def test_driver_dynamics_checks_the_time_step_and_leaves_the_run_alone(tmp_path):
    from synchronization_avoiding_algorithms_amd import results_io as rio

    base = ["dynamics", "--synthetic", "2", "--order", "2", "--material", "svk", "--fz", "50", "--steps", "40"]
    runs = {}
    for tag, extra in (("checked", ["--dt-check-every", "20"]), ("plain", [])):
        where = tmp_path / tag
        where.mkdir()
        out = _driver(base + extra + ["--out", str(where)], where)
        assert out.returncode == 0, out.stderr[-3000:]
        runs[tag] = json.loads(out.stdout.strip().splitlines()[-1])
    check = runs["checked"]["dt_check"]
    print(check)
    assert "dt_check" not in runs["plain"]
    assert set(check) == {"every", "n_checks", "dt_crit_min", "dt_crit_min_step", "dt_over_dt_crit_max", "first_exceeded_step"}
    assert check["every"] == 20 and check["n_checks"] == 2 and check["dt_crit_min_step"] in (20, 40)
    assert np.isfinite(check["dt_over_dt_crit_max"]) and check["dt_over_dt_crit_max"] > 0
    a, b = rio.load_displacement(runs["checked"]["path"]), rio.load_displacement(runs["plain"]["path"])
    assert a.shape == b.shape and a.shape[1] == 40 and np.array_equal(a, b)
    assert {k: v for k, v in runs["checked"].items() if k not in ("dt_check", "path")} == \
        {k: v for k, v in runs["plain"].items() if k != "path"}
