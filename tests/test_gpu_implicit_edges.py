"""The implicit stepper of ``csrc/saa_opimp.hip`` on the MI355X at its reduction and solver edges: launches past the 2048-workgroup
cap and folds of more than 256 partials (meshes padded with element-less nodes), ``check_every``, ``max_cg``, the curvature guard,
reason 2, nodes without elements, the ramp across ``t = 1``, ``set_dt`` in mid-run, power-of-two units and cases off the unit beam.
Against the doubles of tests/implicit_edges.py and tests/implicit_double.py; tests/test_implicit_edges.py qualifies every case,
cap, bar and margin on the CPU and shows that the named mutants fail.  None of the bars comes from what the GPU gave.

Meshes: ``structured288`` (order 1) and ``curved288`` (order 2) of ``finite_strain_double.mesh``, compact or padded to the eight node
counts of ``implicit_edges.PADDED_NODES``: every size on ``structured288`` under ``svk``, the four largest also on ``curved288`` under
``linear`` and ``neo_hookean``."""
import numpy as np
import pytest

import finite_strain_double as fd
import implicit_double as imp
import implicit_edges as ie
import operator_extended as ox
import test_gpu_implicit as tgi
from test_gpu_implicit import _dev, _host

pytestmark = pytest.mark.gpu

EPS = ie.EPS
PADDED_CASES = [(n, "svk", "structured288") for n in ie.PADDED_NODES] + \
               [(n, m, "curved288") for n in ie.LARGE_NODES for m in ("linear", "neo_hookean")]
PADDED_IDS = [f"{n}-{m}-{name}" for n, m, name in PADDED_CASES]


def _bits(t):
    import torch

    return t.view(torch.int64)


def _same(xs, ys):
    """Bit equality of two tuples of tensors (NaN equal to the same NaN)."""
    import torch

    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _counts(info):
    return {k: info[k] for k in ("steps_done", "converged", "reason", "newton_iterations", "cg_iterations")}


def _hold_counts(total, per_step, want_total, want_per_step, label):
    """The rule of the issue's section 1: Newton iterations per step equal to the mirrored double's, the call's PCG iterations
    within ``max(2 per solve, 2 S total)`` of it (``implicit_edges.count_bar``)."""
    print(f"{label}: Newton per step {per_step} (double {want_per_step}), PCG {total['cg_iterations']} (double "
          f"{want_total['cg_iterations']}, bar {ie.count_bar(want_total):.0f})")
    assert per_step == want_per_step
    assert abs(total["cg_iterations"] - want_total["cg_iterations"]) <= ie.count_bar(want_total)


class Padded:
    """A mesh of the double inside ``n_nodes`` points on the GPU: the handle, its lumped mass, the map."""

    def __init__(self, name, n_nodes):
        self.p, self.n_nodes = imp.problem(name), int(n_nodes)
        pts, cells, dd, self.node_map = ie.padded(self.p, n_nodes, n_nodes)
        self.dofs = ie.dof_map(self.node_map)
        self.dd = dd
        self.op = tgi._operator(pts, cells, dd)
        self.mass = self.op.lumped_mass()
        self.live = np.zeros(3 * self.n_nodes, dtype=bool)
        self.live[self.dofs] = self.p.live
        self.has = np.zeros(3 * self.n_nodes, dtype=bool)              # dofs of nodes with elements
        self.has[self.dofs] = True
        self.runs = {}

    def scatter(self, vec, fill=0.0):
        return ie.scatter(vec, self.node_map, self.n_nodes, fill)

    def stepper(self, material, load=None, mass=None, **options):
        from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper

        load = self.scatter(self.p.load(200.0)) if load is None else load
        st = ImplicitStepper(self.op, self.mass if mass is None else mass, _dev(load), 5.0 * self.p.dt_crit, 0.5, ramp=False,
                             material=material)
        for k, v in options.items():
            st.set_option(k, v)
        return st

    def run(self, material, garbage=False):
        """Create, ``set_state`` at the start of the nonlinear case, 3 steps: the states (tuples of ``d, v, a``) after ``set_state``
        and after every step, and the ``info`` of every step.  ``garbage``: NaN in ``mass``, ``load``, ``d``, ``v`` at the element-less
        nodes; NaN, inf, 1e300 in ``load``, ``d``, ``v`` on the Dirichlet dofs."""
        key = (material, garbage)
        if key in self.runs:
            return self.runs[key]
        load, d, mass = self.scatter(self.p.load(200.0)), self.scatter(imp.nonlinear_start(self.p)), self.mass
        v = None
        if garbage:
            mass = self.mass.clone()
            mass[_dev(~self.has).bool()] = float("nan")
            v = np.zeros_like(d)
            junk = np.array([np.nan, np.inf, 1e300, -np.inf, -1e300])
            for k, x in enumerate((load, d, v)):
                x[~self.has] = np.nan
                x[self.dd] = junk[(np.arange(len(self.dd)) + k) % len(junk)]
        with self.stepper(material, load, mass) as st:
            st.set_state(_dev(d), None if v is None else _dev(v))
            states, infos = [st.state()[:3]], []
            for _ in range(ie.EDGE_STEPS):
                infos.append(st.step(1))
                states.append(st.state()[:3])
            t_end = st.state()[3]
        self.runs[key] = (states, infos, t_end)
        return self.runs[key]


@pytest.fixture(scope="module")
def benches():
    made = {}

    def get(name):
        if name not in made:
            made[name] = tgi.Bench(name)
        return made[name]

    yield get
    for b in made.values():
        b.op.close()


@pytest.fixture(scope="module")
def pads():
    made = {}

    def get(name, n_nodes):
        if (name, n_nodes) not in made:
            made[name, n_nodes] = Padded(name, n_nodes)
        return made[name, n_nodes]

    yield get
    for b in made.values():
        b.op.close()


# ---- 2. the reductions at their edges -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_nodes,material,name", PADDED_CASES, ids=PADDED_IDS)
def test_padded_shifted_apply_is_the_compact_one_and_its_dot_is_the_dot(benches, pads, n_nodes, material, name):
    """(a) ``shifted_apply`` with a shift and ``dot=True`` on the padded mesh: on the mesh's dofs ``out`` is the compact call's bit for
    bit (the node sums are the same additions), 0 elsewhere; ``dot`` is within ``64 eps sum|v_i out_i|`` of the longdouble dot of
    the two returned vectors.  Measured on the MI355X: dot errors 6.3e-10 .. 1.2e-9 (bar 2.0e-7) on ``structured288``, 3.6e-9 .. 3.8e-9
    (bar 1.1e-6) on ``curved288``; 0.06 .. 0.25 s per case, the handle's creation included (1.9 s for the first, which starts the
    device)."""
    import torch

    b, pb = benches(name), pads(name, n_nodes)
    p = b.p
    u, v = ie.apply_vectors(p)
    s = ie.apply_shift(p, v)
    want, _ = b.op.shifted_apply(_dev(u), _dev(v), _dev(s), material, dot=True)
    vp = _dev(pb.scatter(v))
    out, dot = pb.op.shifted_apply(_dev(pb.scatter(u)), vp, _dev(pb.scatter(s, fill=1.0)), material, dot=True)
    mesh = torch.as_tensor(pb.dofs, device="cuda")
    assert torch.equal(_bits(out[mesh]), _bits(want)) and bool(want.abs().max() > 0)
    rest = out.clone()
    rest[mesh] = 0.0
    assert not bool(rest.any())
    vl, ol = np.asarray(_host(vp), dtype=np.longdouble), np.asarray(_host(out), dtype=np.longdouble)
    exact, size = (vl * ol).sum(), float(np.abs(vl * ol).sum())
    err = abs(float(np.longdouble(float(dot)) - exact))
    print(f"{n_nodes} {material} {name}: dot error {err:.2e}, bar {64 * EPS * size:.2e}")
    assert err <= 64 * EPS * size


@pytest.mark.parametrize("n_nodes,material,name", PADDED_CASES, ids=PADDED_IDS)
def test_padded_run_against_the_double(pads, n_nodes, material, name):
    """(b) Three steps of the nonlinear case from its start scattered through the map: ``d`` on the mesh's dofs within 1e-8 of ``max|d|``
    of the direct double at ``tol = 1e-13`` stepped 3 times, the Newmark identities to 1e-12, the iteration counts by the rule of
    ``_hold_counts``.  Measured on the MI355X, the same at every size: 8.5e-13 of ``max|d|`` (``structured288 svk``, Newton 4, 5, 6 per
    step, 217 PCG iterations), 1.1e-11 (``curved288 linear``, 2, 2, 2 and 165), 2.7e-13 (``curved288 neo_hookean``, 4, 4, 4 and 190);
    every count equal to the double's; 0.06 .. 1.4 s per case."""
    pb = pads(name, n_nodes)
    states, infos, t_end = pb.run(material)
    assert all(i["converged"] and i["steps_done"] == 1 for i in infos), infos
    dt = 5.0 * pb.p.dt_crit
    want = ie.reference3(name, material)
    d = _host(states[-1][0])
    err = float(np.abs(d[pb.dofs] - want).max() / np.abs(want).max())
    print(f"{n_nodes} {material} {name}: d after 3 steps {err:.2e} of max|d|")
    assert err <= 1e-8 and abs(t_end - ie.EDGE_STEPS * dt) <= 1e-12 * t_end
    for (d0, v0, a0), (d1, v1, a1) in zip(states, states[1:]):
        d0, v0, a0, d1, v1, a1 = (_host(x) for x in (d0, v0, a0, d1, v1, a1))
        ev = np.abs(v1 - (2.0 / dt * (d1 - d0) - v0)).max() / np.abs(v1).max()
        ea = np.abs(a1 - (4.0 / (dt * dt) * (d1 - d0 - dt * v0) - a0)).max() / np.abs(a1).max()
        assert ev <= 1e-12 and ea <= 1e-12, (ev, ea)
    _, total, per_step = ie.mirror3(name, material)
    got = {k: sum(i[k] for i in infos) for k in ("newton_iterations", "cg_iterations")}
    _hold_counts(got, [i["newton_iterations"] for i in infos], total, per_step, f"{n_nodes} {material} {name}")


@pytest.mark.parametrize("n_nodes,material,name", PADDED_CASES, ids=PADDED_IDS)
def test_padded_reported_residual_is_the_true_one(pads, n_nodes, material, name):
    """(c) One step at ``tol = 1e-6``: ``info["residual"]`` is ``|r| / ref`` evaluated by the compact float64 double from the GPU's own ``(d0,
    v0, a0) -> d1``, to ``implicit_edges.RESIDUAL_MARGIN = 1e-6`` of it - ten times what float64 and longdouble differ by there,
    3900 times below the 1 / 257 that one dropped partial of a uniform field moves it by; the dropped-partial and lost-tail
    mutants move it by 1e-5 or more (tests/test_implicit_edges.py).  The linear material's figure is the recurrence residual
    of its solve over the scale at the solved ``x``.  Measured on the MI355X, of the residual: 1.0e-10 .. 7.9e-10 (``structured288 svk``,
    residual 9.05e-8), 1.2e-9 .. 2.1e-9 (``curved288 linear``, 6.58e-7), 1.2e-8 .. 2.6e-8 (``curved288 neo_hookean``, 6.36e-8)."""
    pb = pads(name, n_nodes)
    p = pb.p
    with pb.stepper(material, tol=1e-6) as st:
        st.set_state(_dev(pb.scatter(imp.nonlinear_start(p))))
        d0, v0, a0, _ = st.state()
        info = st.step(1)
        d1 = st.state()[0]
    take = lambda x: _host(x)[pb.dofs]
    true = ie.true_residual(p, material, take(pb.mass), p.load(200.0), 5.0 * p.dt_crit, 0.5, 1.0, take(d0), take(v0), take(a0), take(d1))
    print(f"{n_nodes} {material} {name}: reported {info['residual']:.6e}, recomputed {true:.6e}, "
          f"difference {abs(info['residual'] - true) / true:.2e} of it", _counts(info))
    assert info["converged"] and info["steps_done"] == 1 and 0.0 < info["residual"] <= 1e-6
    assert abs(info["residual"] - true) <= ie.RESIDUAL_MARGIN * true


@pytest.mark.parametrize("n_nodes,material,name", PADDED_CASES, ids=PADDED_IDS)
def test_padded_run_reads_no_garbage(pads, n_nodes, material, name):
    """(d) NaN in ``mass``, ``load``, ``d``, ``v`` at the element-less nodes and NaN, inf, 1e300 in ``load``, ``d``, ``v`` on the Dirichlet dofs:
    across create, ``set_state`` and 3 steps no bit of ``d, v, a`` and no count differs from the clean padded run, and ``d, v, a``
    are exactly 0 off the live dofs."""
    pb = pads(name, n_nodes)
    clean, infos, t_end = pb.run(material)
    dirty, infos_d, t_end_d = pb.run(material, garbage=True)
    off = _dev(~pb.live).bool()
    for k, (a, b) in enumerate(zip(clean, dirty)):
        assert _same(a, b), k
        assert all(not bool(x[off].any()) and bool(x.isfinite().all()) for x in b), k
    assert [_counts(i) for i in infos] == [_counts(i) for i in infos_d] and t_end == t_end_d
    assert [i["residual"] for i in infos] == [i["residual"] for i in infos_d]


# ---- 3. the solver controls -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", ("svk", "linear"))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_the_iterate_does_not_depend_on_when_the_host_looks(benches, name, material):
    """``check_every`` in (1, 3, 25, 10^6): the 3-step run gives bit-equal ``d, v, a, t``, equal counts and residuals, and the counts
    of the mirrored double.  Measured on the MI355X: Newton 4, 5, 6 / 4, 4, 5 per step and 217 / 194 PCG iterations under ``svk``, 1,
    2, 2 / 2, 2, 2 and 167 / 165 under ``linear``, all equal to the double's; 0.4 .. 7.8 s (``curved288 svk``: the four runs, the
    handle, and 2 s of the double on the CPU)."""
    b = benches(name)
    runs = []
    for every in (1, 3, 25, 10 ** 6):
        with b.nonlinear(material, check_every=every) as st:
            infos = [st.step(1) for _ in range(ie.EDGE_STEPS)]
            runs.append((st.state(), [(_counts(i), i["residual"]) for i in infos]))
        assert all(i["converged"] for i in infos), (every, infos)
    for state, counts in runs[1:]:
        assert _same(state[:3], runs[0][0][:3]) and state[3] == runs[0][0][3] and counts == runs[0][1]
    _, total, per_step = ie.mirror3(name, material)
    got = {k: sum(c[k] for c, _ in runs[0][1]) for k in ("newton_iterations", "cg_iterations")}
    _hold_counts(got, [c["newton_iterations"] for c, _ in runs[0][1]], total, per_step, f"{name} {material}")


@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_max_cg_is_a_cap_per_solve(benches, name):
    """``svk`` at ``max_cg = 3``: reason 1 after 25 passes of 3 iterations, the state untouched bit for bit; at 5: converged, every
    solve at the cap, the Newton counts of the mirrored double with the same cap (15 .. 18 per step).  The linear material at
    ``tol = 1e-12`` and the cap 20 (its solve needs 60 or more): several passes per step, within ``10 N tol kappa`` of the direct
    double, with the mirrored double's counts.  Measured on the MI355X: every count equal to the double's (``svk`` at 5: 16, 16, 18
    / 15, 15, 16 passes, 246 / 227 iterations; linear at 20: 4, 4, 4 passes, 208 / 201), ``svk`` 1.7e-11 / 5.1e-12 of ``max|d|``,
    linear 4.1e-13 / 9.7e-14 (bar 7.8e-10); 0.4 / 4.3 s."""
    b = benches(name)
    p = b.p
    want = ie.nonlinear_stepper(p, "svk", max_cg=ie.CAP_FAILS).step(3)
    with b.nonlinear("svk", max_cg=ie.CAP_FAILS) as st:
        before = st.state()
        info = st.step(3)
        after = st.state()
    assert _counts(info) == _counts(want) and info["reason_name"] == "max_newton" and (want["reason"], want["steps_done"]) == (1, 0)
    assert _same(before[:3], after[:3]) and before[3] == after[3]
    for material, cap, options in (("svk", ie.CAP_CONVERGES, {}), ("linear", ie.CAP_LINEAR, {"tol": 1e-12})):
        nm = ie.nonlinear_stepper(p, material, max_cg=cap, **options)
        total, per_step, last = ie.run(nm, ie.EDGE_STEPS)
        with b.nonlinear(material, max_cg=cap, **options) as st:
            infos = [st.step(1) for _ in range(ie.EDGE_STEPS)]
            d = _host(st.state()[0])
        assert last["converged"] and all(i["converged"] for i in infos), infos
        got = {k: sum(i[k] for i in infos) for k in ("newton_iterations", "cg_iterations")}
        _hold_counts(got, [i["newton_iterations"] for i in infos], total, per_step, f"{name} {material} cap {cap}")
        ref = ie.reference3(name, "svk") if material == "svk" else ie.linear_direct3(name)
        bar = 1e-8 if material == "svk" else 10 * ie.EDGE_STEPS * 1e-12 * imp.modal_kappa(p, 5.0 * p.dt_crit)
        err = float(np.abs(d - ref).max() / np.abs(ref).max())
        print(f"{name} {material} cap {cap}: {err:.2e} bar {bar:.2e}")
        assert err <= bar and min(per_step) >= 3


@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_curvature_guard_stops_the_solve_on_the_device(benches, name):
    """At the compressed ``svk`` state of ``implicit_edges.guard_case`` ``K_T + s`` is indefinite and the mirrored PCG meets ``p . J p < 0``
    (robustly: 5.7e-3 of ``|p| |J p|`` or more on either side) in iteration ``k + 1 = 14 / 31``.  With ``max_newton = 1``: reason 1 with
    ``cg_iterations == k``, the state untouched, every entry finite; the stepper converges afterwards from the nonlinear start.
    Measured on the MI355X: ``k = 13 / 30``, residual 1.0."""
    b = benches(name)
    p = b.p
    u, dt, k, _, want = ie.guard_case(name)
    with b.stepper(p.load(200.0), dt, 0.0, False, "svk", max_newton=1) as st:
        st.set_state(_dev(u))
        before = st.state()
        info = st.step(1)
        after = st.state()
        print(f"{name}: k = {k}", info)
        assert _counts(info) == _counts(want) and (info["reason"], info["steps_done"], info["cg_iterations"]) == (1, 0, k)
        assert _same(before[:3], after[:3]) and before[3] == after[3] and all(bool(x.isfinite().all()) for x in after[:3])
        st.set_option("max_newton", 25)
        st.set_dt(5.0 * p.dt_crit)
        st.set_state(_dev(imp.nonlinear_start(p)))
        assert st.step(1)["converged"]


@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("kind", ("nan", "overflow"))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_a_residual_that_is_not_finite_is_reason_2(benches, name, kind, material):
    """A load with NaN at the highest live dof, and a finite load (1e200 of the nonlinear case's) whose squared norm
    overflows: ``(2, "non_finite", 0)``, the state untouched bit for bit; a new stepper on the handle with a sound load and a sound
    ``set_state`` converges."""
    b = benches(name)
    p = b.p
    load = p.load(200.0)
    if kind == "nan":
        load[p.idx[-1]] = np.nan
    else:
        load = load * 1e200
    with b.stepper(load, 5.0 * p.dt_crit, 0.5, False, material) as st:
        st.set_state(_dev(imp.nonlinear_start(p)))
        before = st.state()
        info = st.step(2)
        after = st.state()
    print(name, kind, material, info)
    assert (info["reason"], info["reason_name"], info["steps_done"], info["converged"]) == (2, "non_finite", 0, False)
    assert _same(before[:3], after[:3]) and before[3] == after[3]
    with b.nonlinear(material) as st:
        assert st.step(1)["converged"]


# ---- 4. time ------------------------------------------------------------------------------------------------------------------

class _Gpu:
    """What ``implicit_edges.time_run`` drives, on the GPU stepper."""

    def __init__(self, bench):
        self.bench = bench

    def __call__(self, prob, mass, load, dt, alpha, ramp=True, material="linear", **options):
        self.st = self.bench.stepper(load, dt, alpha, ramp, material, **options)
        self.newton_per_step, self.cg = [], 0
        return self

    def set_state(self, d=None, v=None, t=0.0):
        self.st.set_state(_dev(d), None if v is None else _dev(v), t)

    def set_dt(self, dt):
        self.st.set_dt(dt)

    def step(self, n):
        info = self.st.step(n)
        if info["converged"]:
            self.newton_per_step.append(info["newton_iterations"])
        self.cg += info["cg_iterations"]
        return info


@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("kind", ("ramp", "set_dt"))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_ramp_across_one_and_set_dt_in_mid_run(benches, name, kind, material):
    """The two cases of ``implicit_edges.time_run`` against the direct double doing the same - ``ramp=True`` from ``t = 1 - 1.5 dt``, 3
    steps (scales ``1 - dt/2``, 1, 1); 2 steps at ``5 dt_crit``, ``set_dt(12.5 dt_crit)``, 2 steps -: linear at ``tol = 1e-12`` within ``10 N
    tol kappa``, ``svk`` within 1e-8 of ``max|d|``, and the iteration counts of the mirrored double.  On the CPU a ramp clamped one step
    late misses the bars by a factor of 60 or more; an old shift misses the linear bar by 5e6, and under ``svk`` its Newton does
    not converge.  Measured on the MI355X: linear 1.1e-13 .. 3.7e-13 (bars 7.8e-10 and 6.3e-9), ``svk`` 1.4e-12 .. 9.0e-12 (bar 1e-8);
    every count equal to the double's (184 .. 198 PCG iterations over the ramp, 412 .. 440 over the four steps around ``set_dt``);
    0.1 .. 2.1 s."""
    b = benches(name)
    p = b.p
    want, bar, options = ie.time_reference(name, material, kind)
    mirror = ie.time_run(ie.NewmarkPCG, p, material, kind, **options)
    gpu = _Gpu(b)
    try:
        ie.time_run(gpu, p, material, kind, **options)
        d, _, _, t = gpu.st.state()
        d = _host(d)
    finally:
        gpu.st.close()
    err = float(np.abs(d - want.d).max() / np.abs(want.d).max())
    print(f"{name} {kind} {material}: {err:.2e} bar {bar:.2e}")
    assert gpu.last["converged"] and abs(t - want.t) <= 1e-12 * want.t and err <= bar
    total = {"newton_iterations": sum(mirror.newton_per_step), "cg_iterations": sum(mirror.cg_per_solve)}
    _hold_counts({"cg_iterations": gpu.cg}, gpu.newton_per_step, total, mirror.newton_per_step, f"{name} {kind} {material}")


# ---- 5. scales ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", ox.UNITS)
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_power_of_two_units_commute_bitwise(benches, name, u):
    """Lengths, ``dt`` and ``1 / alpha`` times ``2^(40 u)``, moduli and density times ``2^(20 u)`` (``implicit_edges.UNIT_EXPONENT``): 3
    nonlinear (``svk``) and 3 linear steps give ``d, v, a`` bit-equal to the unscaled run times ``2^(40 u)``, 1, ``2^(-40 u)`` and equal
    counts.  The mirrored double commutes itself, with every intermediate inside 4e-90 .. 3e72."""
    import torch

    b = benches(name)
    p = b.p
    mass0, load0, dt0, alpha0, start0 = ie.units_inputs(name, 0)
    _, load, dt, alpha, start = ie.units_inputs(name, u)
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    with ModalOperator(p.pts * ie.unit("points", u), p.cells.astype(np.int32), p.dd.astype(np.int32), imp.LMD * ie.unit("modulus", u),
                       imp.MU * ie.unit("modulus", u), fd.RHO * ie.unit("density", u)) as op:
        mass = op.lumped_mass()
        assert torch.equal(mass, b.mass * ie.unit("mass", u))
        for material in ("svk", "linear"):
            out = []
            for o, m, f, h, al, s0 in ((b.op, b.mass, load0, dt0, alpha0, start0), (op, mass, load, dt, alpha, start)):
                with ImplicitStepper(o, m, _dev(f), h, al, ramp=False, material=material) as st:
                    st.set_state(_dev(s0))
                    infos = [st.step(1) for _ in range(ie.EDGE_STEPS)]
                    out.append((st.state(), [(_counts(i), i["residual"]) for i in infos]))
                assert all(i["converged"] for i in infos), (material, infos)
            (base, counts0), (got, counts) = out
            assert counts == counts0, (material, counts, counts0)
            for key, x, y in zip(("d", "v", "a"), got[:3], base[:3]):
                assert bool(y.abs().max() > 0) and torch.equal(x, y * ie.unit(key, u)), (material, key)
            assert got[3] == base[3] * ie.unit("dt", u)


@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("family", ie.OFF_BEAM)
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_off_beam_reported_residual_is_the_true_one(name, family, material):
    """``nu = 0.499999`` and the ``sliver 1e-6`` family on the compact meshes, one step of the nonlinear case at ``tol = 1e-6``: the step
    converges, the reported residual is ``<= tol`` and is the true one - recomputed by the float64 double from the GPU's own states
    - to ``implicit_edges.OFF_BEAM_MARGIN = 5e-5`` of it: ten times what float64 and longdouble differ by on these cases (3.8e-6
    on ``curved288`` with slivers under ``svk``, where ``f_int`` cancels most), 78 times below 1 / 257.  No comparison of ``d``.
    Measured on the MI355X, of the residual: ``nu`` 2.3e-11 .. 3.6e-9; slivers on ``structured288`` 1.7e-9 / 1.5e-9 (linear / ``svk``), on
    ``curved288`` 7.1e-7 (linear) and 5.3e-6 (``svk``, 17 Newton passes).  The last case found a defect: with the order-2 geometry
    table formed from absolute coordinates it reported 1.004114e-7 against 1.004026e-7 recomputed, 8.7e-5 of it, and the force
    pass was 5.9e-10 of ``max|f|`` off the longdouble force at the same state, all of it at the sliver elements' nodes (the
    float64 double, which centres an element on its first node: 4.8e-11).  With ``opstep_geometry_kernel`` centring likewise
    the force is 3.9e-11 off."""
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    p = ie.off_beam_problem(name, family)
    dt = 5.0 * p.dt_crit
    with ModalOperator(p.pts, p.cells.astype(np.int32), p.dd.astype(np.int32), p.lmd, p.mu, p.rho) as op:
        mass = op.lumped_mass()
        with ImplicitStepper(op, mass, _dev(p.load(200.0)), dt, 0.5, ramp=False, material=material) as st:
            st.set_option("tol", 1e-6)
            st.set_state(_dev(ie.OFF_BEAM_AMPLITUDE * imp.nonlinear_start(p)))
            d0, v0, a0, _ = st.state()
            info = st.step(1)
            d1 = st.state()[0]
    true = ie.true_residual(p, material, _host(mass), p.load(200.0), dt, 0.5, 1.0, _host(d0), _host(v0), _host(a0), _host(d1))
    print(f"{p.name} {material}: reported {info['residual']:.6e}, recomputed {true:.6e}, "
          f"difference {abs(info['residual'] - true) / true:.2e} of it", _counts(info))
    assert info["converged"] and info["steps_done"] == 1 and 0.0 < info["residual"] <= 1e-6
    assert abs(info["residual"] - true) <= ie.OFF_BEAM_MARGIN * true
