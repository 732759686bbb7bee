"""Implicit Newmark dynamics on the operator handle on the MI355X (``csrc/saa_opimp.hip``): ``saa_operator_shifted_apply``,
``saa_operator_implicit_*``, ``dynamics.ImplicitStepper`` and ``drivers dynamics --scheme newmark``, against the NumPy double of
tests/implicit_double.py (which tests/test_implicit.py qualifies on the CPU).

Meshes: those of ``finite_strain_double.mesh`` (at most 288 elements / 625 nodes; 288 = 256 + 32 crosses a block edge of the
256-lane passes), except the two driver runs, which build their own.  Bars: see each test; none comes from what the GPU gave."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import implicit_double as imp
import operator_extended as ox
import tangent_double as td

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_MATERIALS = ("linear",) + tuple(fd.MATERIALS)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(t):
    return t.cpu().numpy()


def _operator(pts, cells, dd, lmd=imp.LMD, mu=imp.MU):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(pts, np.asarray(cells).astype(np.int32), np.asarray(dd).astype(np.int32), lmd, mu, fd.RHO)


class Bench:
    """A mesh of the double on the GPU: the handle and its lumped mass."""

    def __init__(self, name):
        self.p = imp.problem(name)
        self.op = _operator(self.p.pts, self.p.cells, self.p.dd)
        self.mass = self.op.lumped_mass()

    def stepper(self, load, dt, alpha, ramp, material="linear", **options):
        from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper

        st = ImplicitStepper(self.op, self.mass, _dev(load), dt, alpha, ramp=ramp, material=material)
        for k, v in options.items():
            st.set_option(k, v)
        return st

    def nonlinear(self, material, **options):
        """The stepper of ``implicit_double.nonlinear_run`` at its start."""
        st = self.stepper(self.p.load(200.0), 5.0 * self.p.dt_crit, 0.5, False, material, **options)
        st.set_state(_dev(imp.nonlinear_start(self.p)))
        return st


@pytest.fixture(scope="module")
def benches():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Bench(name)
        return made[name]

    yield get
    for b in made.values():
        b.op.close()


# ---- 1. the shifted apply -----------------------------------------------------------------------------------------------------

def _shift_of(case, ref_d, v):
    """A positive diagonal of the size that makes ``s v`` comparable with ``K_T v``: ``(0.5 .. 1.5) max|K_T v| / max|v|``."""
    rng = np.random.default_rng(4242 + len(case["points"]))
    return rng.uniform(0.5, 1.5, size=v.shape) * float(np.abs(np.asarray(ref_d, dtype=np.float64)).max() / np.abs(v).max())


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", td.case_ids(), ids=fx.case_name)
def test_shifted_apply_is_within_the_bar_of_the_tangent(cid, material):
    """``K_T(u) v + s v`` against the longdouble ``tangent + s v`` on the cases and directions of ``tangent_double.case_ids``, to the
    bar of tests/test_gpu_tangent.py, ``err <= 1e-12 + 8 env``.  ``env`` of the sum: the envelope of ``K_T v`` carried over to the new
    largest entry, plus ``2^-52 max|s v|`` - what the same ``+-2^-53`` perturbation of ``s`` and ``v`` does to their product."""
    case, ref, env = td.reference(cid)
    free = np.ones(3 * len(case["points"]), dtype=bool)
    free[np.asarray(case["dd"], dtype=np.int64)] = False
    got, want, env_sum = {}, {}, {}
    with _operator(case["points"], case["cells"], case["dd"], case["lmd"], case["mu"]) as op:
        u = _dev(case["u"])
        for d in td.DIRECTIONS:
            v = case["v_" + d]
            r = np.asarray(ref[material][d][0], dtype=np.longdouble)
            s = _shift_of(case, r, v)
            sv = np.where(free, np.asarray(s, dtype=np.longdouble) * np.asarray(v, dtype=np.longdouble), np.longdouble(0))
            want[d] = (r + sv)[None]
            top = float(np.abs(want[d]).max())
            env_sum[d] = (env[material][d] * float(np.abs(r).max()) + 2.0 ** -52 * float(np.abs(sv).max())) / top
            out = op.shifted_apply(u, _dev(v), _dev(s), material)
            got[d] = _host(out)[None]
            assert not got[d][0][case["dd"]].any()
    _, bad = ox.check(got, want, env_sum, ox.KERNEL_FACTOR, f"{fx.case_name(cid)} {material} shifted", names=list(td.DIRECTIONS))
    assert not bad, bad


@pytest.mark.parametrize("material", ALL_MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_shifted_apply_without_shift_is_the_tangent_apply_and_its_dot_is_the_dot(name, material):
    """``shift = None`` is ``tangent_apply`` bit for bit; with a shift two calls are bit-equal, Dirichlet rows are exactly 0 and
    ``dot`` is within ``64 eps sum|v_i out_i|`` of the longdouble dot of the same two vectors."""
    import torch

    case = td.build_case((name, "strain", 0, 0.3))
    eps = float(np.finfo(np.float64).eps)
    with _operator(case["points"], case["cells"], case["dd"], case["lmd"], case["mu"]) as op:
        u, v = _dev(case["u"]), _dev(case["v_random"])
        want = op.tangent_apply(None if material == "linear" else u, v, material)
        plain, dot0 = op.shifted_apply(None if material == "linear" else u, v, None, material, dot=True)
        assert torch.equal(plain, want) and torch.equal(op.shifted_apply(u, v, None, material), want)
        s = _dev(_shift_of(case, _host(want), case["v_random"]))
        a, da = op.shifted_apply(u, v, s, material, dot=True)
        b, db = op.shifted_apply(u, v, s, material, dot=True)
        assert torch.equal(a, b) and torch.equal(da, db) and not torch.equal(a, want)
        assert not _host(a)[case["dd"]].any() and bool(torch.isfinite(a).all())
        for out, dot in ((plain, dot0), (a, da)):
            vl, ol = np.asarray(_host(v), dtype=np.longdouble), np.asarray(_host(out), dtype=np.longdouble)
            exact, size = (vl * ol).sum(), float(np.abs(vl * ol).sum())
            err = abs(float(np.longdouble(float(dot)) - exact))
            print(f"{name} {material}: dot error {err:.2e}, bar {64 * eps * size:.2e}")
            assert err <= 64 * eps * size


# ---- 2. the linear material: exact discrete frequency, energy -------------------------------------------------------------------

@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_linear_modes_turn_by_the_exact_discrete_angle(benches, name):
    """From ``d = phi_j``, ``v = 0``, no load, no damping, 40 steps at ``tol = 1e-12``: ``d = phi_j cos(40 theta)``, ``theta = 2 atan(omega_j dt /
    2)``.  Bar ``10 N tol kappa`` of ``max|phi| = 1``, ``kappa = (1 + (omega_max dt/2)^2) / (1 + (omega_1 dt/2)^2)`` the condition number
    of ``J`` in the mass norm (a residual of ``tol`` is an error of at most ``tol kappa``), 10 for the change of norm.
    Measured on the MI355X (``structured288`` / ``beam36``): lowest mode 5.3e-11 / 1.7e-13 (bar 9.4e-7 / 9.8e-7), middle 3.8e-11 /
    2.4e-11 (bar 1.0e-8), highest 5.0e-11 / 2.2e-11 (bar 4.0e-9); 36 .. 147 PCG iterations per step."""
    b = benches(name)
    p = b.p
    for j, factor in imp.modal_cases(p):
        dt = factor * p.dt_crit
        with b.stepper(np.zeros(p.n), dt, 0.0, False, tol=1e-12) as st:
            st.set_state(_dev(p.mode(j)))
            info = st.step(imp.MODAL_STEPS)
            d = _host(st.state()[0])
        err = float(np.abs(d - imp.modal_exact(p, j, dt, imp.MODAL_STEPS)).max())
        bar = 10 * imp.MODAL_STEPS * 1e-12 * imp.modal_kappa(p, dt)
        print(f"{name} mode {j} at {factor} dt_crit: error {err:.2e} bar {bar:.2e}", info)
        assert info["converged"] and info["steps_done"] == imp.MODAL_STEPS
        assert err <= bar


@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_linear_run_conserves_the_energy(benches, name):
    """Constant ``fz = 0.5``, undamped, ``dt = 20 dt_crit``, 50 steps at ``tol = 1e-12``: ``T + U - f . d`` drifts by at most 1e-9 of the
    largest ``U`` - 50 steps times ``tol``, times 20 for the inexact solves; the scheme itself conserves exactly.  The stepper is
    used as created: its initial acceleration is that of the balance at rest, ``f / m``.  Measured on the MI355X: 6.4e-13 / 1.1e-12."""
    b = benches(name)
    p = b.p
    load, mass = p.load(0.5), _host(b.mass)
    bal, u = [], []
    with b.stepper(load, 20.0 * p.dt_crit, 0.0, False, tol=1e-12) as st:
        for k in range(51):
            if k:
                assert st.step(1)["converged"]
            d, v, _, _ = (_host(x) if hasattr(x, "cpu") else x for x in st.state())
            u.append(0.5 * float(d @ (p.K @ d)))
            bal.append(0.5 * float(mass @ (v * v)) + u[-1] - float(load @ d))
    drift = float(np.abs(np.array(bal) - bal[0]).max() / max(u))
    print(f"{name}: energy drift {drift:.2e} of the largest U = {max(u):.3e}")
    assert max(u) > 0 and drift <= 1e-9


# ---- 3. the nonlinear materials against the double ----------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_nonlinear_run_against_the_double(benches, name, material):
    """``d`` after the 12 steps of ``implicit_double.nonlinear_run`` at ``tol = 1e-10`` against the double at ``tol = 1e-13``: 1e-8 of
    ``max|d|``, the double's own sensitivity at a hundred times looser tolerance.  ``v`` and ``a`` of every step satisfy the Newmark
    identities with the states before, to 1e-12 of their largest entry.  Measured on the MI355X: 2.1e-13 .. 4.0e-12 over the four
    meshes and both materials, 4 .. 5 Newton and 52 .. 70 PCG iterations per step."""
    b = benches(name)
    want = imp.nonlinear_reference(name, material)
    with b.nonlinear(material) as st:
        dt = st.dt
        states = [tuple(_host(x) for x in st.state()[:3])]
        total = {"newton_iterations": 0, "cg_iterations": 0}
        for _ in range(imp.NONLINEAR_STEPS):
            info = st.step(1)
            assert info["converged"] and info["steps_done"] == 1, info
            for k in total:
                total[k] += info[k]
            states.append(tuple(_host(x) for x in st.state()[:3]))
        t_end = st.state()[3]
    err = float(np.abs(states[-1][0] - want).max() / np.abs(want).max())
    print(f"{name} {material}: d after 12 steps {err:.2e} of max|d|;", total)
    assert abs(t_end - imp.NONLINEAR_STEPS * dt) <= 1e-12 * t_end
    assert err <= 1e-8
    for (d0, v0, a0), (d1, v1, a1) in zip(states, states[1:]):
        ev = np.abs(v1 - (2.0 / dt * (d1 - d0) - v0)).max() / np.abs(v1).max()
        ea = np.abs(a1 - (4.0 / (dt * dt) * (d1 - d0 - dt * v0) - a0)).max() / np.abs(a1).max()
        assert ev <= 1e-12 and ea <= 1e-12, (ev, ea)


@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_implicit_and_explicit_kernels_agree_at_equal_dt(benches, name):
    """The second-order case (ramped ``fz = 0.5``, ``alpha = 0.5``, to ``t = 0.05``) at the explicit step on both GPU steppers: they
    differ by the two schemes' truncation errors, which the two doubles show; within twice the doubles' own difference."""
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    b = benches(name)
    p = b.p
    load, dt, n = imp.second_order_case(p)
    nm = imp.Newmark(p, p.mass, load, dt, 0.5, ramp=True)
    nm.set_state()
    nm.step(n)
    ex = imp.explicit_run(p, load, dt, n)
    own = float(np.abs(nm.d - ex).max() / np.abs(ex).max())
    with b.stepper(load, dt, 0.5, True) as st:
        assert st.step(n)["converged"]
        di = _host(st.state()[0])
    with OperatorStepper(b.op, b.mass, _dev(load), dt, 0.5, ramp=True) as st:
        st.step(n)
        de = _host(st.state()[0])
    got = float(np.abs(di - de).max() / np.abs(de).max())
    print(f"{name}: implicit - explicit on the GPU {got:.3e}, of the doubles {own:.3e}")
    assert own > 1e-7 and got <= 2.0 * own


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_runs_are_bitwise_repeatable_however_they_are_split(benches, name, material):
    import torch

    b = benches(name)
    n = imp.NONLINEAR_STEPS
    with b.nonlinear(material) as st:
        traj = st.record(n)
        whole = st.step(n)
        one = st.state()
        cols = traj.clone()
    assert whole["converged"] and whole["steps_done"] == n
    assert torch.equal(cols[:, n - 1], one[0])                        # the column of step index i is the d after that step
    with b.nonlinear(material) as st:
        traj = st.record(n)
        first = st.step(5)
        mid = st.state()
        assert st.step(0) == {"steps_done": 0, "converged": True, "reason": 0, "reason_name": "ok", "newton_iterations": 0,
                              "cg_iterations": 0, "residual": 0.0}
        again = st.state()
        assert all(torch.equal(x, y) for x, y in zip(mid[:3], again[:3])) and mid[3] == again[3]
        assert torch.equal(traj[:, 4], mid[0]) and not traj[:, 5:].any()
        second = st.step(7)
        two = st.state()
        assert torch.equal(traj, cols)
    assert all(torch.equal(x, y) for x, y in zip(one[:3], two[:3])) and one[3] == two[3]
    for k in ("newton_iterations", "cg_iterations"):
        assert first[k] + second[k] == whole[k]
    with b.nonlinear(material) as st:                                 # and a third run that records every other step
        half = st.record(n // 2, save_every=2)
        st.step(n)
        three = st.state()
        assert torch.equal(half, cols[:, 0::2])
    assert all(torch.equal(x, y) for x, y in zip(one[:3], three[:3]))


@pytest.mark.parametrize("name", ("structured288", "beam36"))
def test_state_round_trip_and_initial_acceleration(benches, name):
    """``set_state`` masks ``d`` and ``v`` and sets ``a = (scale(t) f - f_int(d) - alpha m v) / m``; ``get_state`` hands back what was
    set.  Against the double's float64 ``a`` at 1e-12 of its largest entry (one force evaluation, the project's bar)."""
    b = benches(name)
    p = b.p
    d = 0.2 * fd.bend(p.pts, 0.5, p.dd)
    v = np.where(p.live, fd.smooth_random_field(p.pts, 5), 0.0)
    raw_d, raw_v = d.copy(), v.copy()
    raw_d[p.dd], raw_v[p.dd] = 3.0, -2.0                              # the mask takes these out
    for material in ALL_MATERIALS:
        nm = imp.Newmark(p, p.mass, p.load(200.0), 1e-3, 0.5, ramp=True, material=material)
        nm.set_state(d, v, 0.25)
        with b.stepper(p.load(200.0), 1e-3, 0.5, True, material) as st:
            st.set_state(_dev(raw_d), _dev(raw_v), 0.25)
            gd, gv, ga, t = st.state()
        assert t == 0.25 and np.array_equal(_host(gd), d) and np.array_equal(_host(gv), v)
        err = float(np.abs(_host(ga) - nm.a).max() / np.abs(nm.a).max())
        print(f"{name} {material}: initial acceleration {err:.2e}")
        assert err <= 1e-12 and not _host(ga)[p.dd].any()


def test_a_step_that_is_not_accepted_leaves_the_state_alone(benches):
    import torch

    b = benches("structured288")
    p = b.p
    with b.nonlinear("svk", max_newton=1) as st:                      # 3 to 6 iterations are needed
        before = st.state()
        info = st.step(3)
        after = st.state()
    assert (info["reason"], info["reason_name"], info["steps_done"], info["converged"]) == (1, "max_newton", 0, False)
    assert info["newton_iterations"] == 1 and info["residual"] > 1e-10
    assert all(torch.equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3]
    # neo-Hooke from a state with inverted elements: the first trial already holds them
    fs = fd.FiniteStrain(p.pts, p.cells, imp.LMD, imp.MU, p.dd)
    _, u, elements = fd.inversion_state(fs, p.pts)
    with b.stepper(p.load(0.5), 5.0 * p.dt_crit, 0.5, False, "neo_hookean") as st:
        st.set_state(_dev(u))
        before = st.state()
        info = st.step(2)
        after = st.state()
        assert (info["reason"], info["reason_name"], info["steps_done"], info["converged"]) == (3, "inverted", 0, False)
        assert all(torch.equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3]
        st.set_state(_dev(imp.nonlinear_start(p)))                    # and the stepper is usable afterwards
        assert st.step(1)["converged"]
    with b.stepper(p.load(0.5), 5.0 * p.dt_crit, 0.5, False, "svk") as st:   # svk has no inversion rule: it goes on
        st.set_state(_dev(0.1 * imp.nonlinear_start(p)))
        st.set_dt(2.0 * p.dt_crit)
        assert st.dt == 2.0 * p.dt_crit and st.step(2)["converged"] and abs(st.state()[3] - 4.0 * p.dt_crit) < 1e-15


def test_arguments_are_refused(benches):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper

    b = benches("structured288")
    p = b.p
    bad_mass = b.mass.clone()
    bad_mass[3 * int(p.cells[0, 0])] = 0.0
    with pytest.raises(_lib.SaaError) as exc:
        ImplicitStepper(b.op, bad_mass, _dev(p.load(0.5)), 1e-3, 0.5)
    assert exc.value.code == _lib.SAA_E_ARG and "mass is not > 0 at 1 node" in str(exc.value)
    with pytest.raises(ValueError):
        ImplicitStepper(b.op, b.mass, _dev(p.load(0.5)), 1e-3, 0.5, material="rubber")
    with b.stepper(p.load(0.5), 1e-3, 0.5, True) as st:
        for name, value in (("tol", 0.0), ("tol", 1.0), ("max_newton", 0), ("max_cg", 2.5), ("check_every", -1), ("nope", 1)):
            with pytest.raises(_lib.SaaError) as exc:
                st.set_option(name, value)
            assert exc.value.code == _lib.SAA_E_ARG
        with pytest.raises(_lib.SaaError) as exc:
            st.step(-1)
        assert exc.value.code == _lib.SAA_E_ARG
        with pytest.raises(_lib.SaaError) as exc:
            st.set_dt(0.0)
        assert exc.value.code == _lib.SAA_E_ARG
        buf = torch.zeros(p.n, dtype=torch.float64, device="cuda")
        assert st._lib.saa_operator_implicit_set_recorder(st._h, C.c_void_p(buf.data_ptr()), 0, 1, 0) == _lib.SAA_E_ARG
        assert st._lib.saa_operator_implicit_step(st._h, 1, None) == _lib.SAA_E_ARG
        with pytest.raises(ValueError):
            st.set_state(np.zeros(5))
    with pytest.raises(ValueError):
        b.op.shifted_apply(None, b.mass, None, "svk")


# ---- 5. the driver ------------------------------------------------------------------------------------------------------------

EXPLICIT_KEYS = {"order", "n_nodes", "n_elems", "n_free_dofs", "dt", "dt_crit", "dt_reference_rule", "ratio", "omega_max", "steps",
                 "tn", "max_abs_d", "tip_deflection", "path"}
NEWMARK_KEYS = {"scheme", "dt_factor", "newton_iterations", "cg_iterations", "converged", "failed_step"}


def _driver(tmp_path, *flags):
    cmd = [sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "dynamics", "--synthetic", "2", "--steps", "20",
           "--out", str(tmp_path), *flags]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_driver_runs_the_newmark_scheme(tmp_path):
    rep = _driver(tmp_path, "--scheme", "newmark", "--order", "2")
    print(rep)
    assert set(rep) == EXPLICIT_KEYS | NEWMARK_KEYS
    assert rep["converged"] is True and rep["failed_step"] == -1 and rep["scheme"] == "newmark" and rep["dt_factor"] == 10.0
    assert rep["order"] == 2 and rep["steps"] == 20 and abs(rep["dt"] - 10.0 * rep["dt_crit"]) <= 1e-15 * rep["dt"]
    assert abs(rep["tn"] - 20 * rep["dt"]) <= 1e-12 * rep["tn"]
    assert rep["newton_iterations"] >= 20 and rep["cg_iterations"] >= rep["newton_iterations"] and rep["max_abs_d"] > 0
    assert os.path.exists(rep["path"])


def test_driver_default_is_the_explicit_run_key_for_key(tmp_path):
    rep = _driver(tmp_path)
    assert set(rep) == EXPLICIT_KEYS and abs(rep["dt"] - 0.9 * rep["dt_crit"]) <= 1e-15 * rep["dt"]
