"""The edge tests of the implicit stepper without a GPU: every case, cap, bar and margin that tests/test_gpu_implicit_edges.py
holds the kernels to is shown here to hold for the references alone (tests/implicit_edges.py, tests/implicit_double.py), and
each mutant that a GPU test must catch is shown to fail its check.

Measured with the doubles on the CPU (``structured288`` / ``curved288`` where two figures are given):

* :class:`implicit_edges.NewmarkPCG` against the direct double: the 12-step nonlinear cases 2.1e-13 .. 4.0e-12 of ``max|d|`` (bar
  1e-8), 4 .. 6 Newton and 52 .. 70 PCG iterations per step; the modal cases 9.9e-13 .. 5.0e-11 (bars 4.0e-9 .. 9.8e-7), 36 .. 145 PCG
  iterations per step.
* ``S``: over 8 draws of random summation orders the nonlinear cases (all four meshes, both materials, 12 steps) kept every
  Newton count and every PCG count.  Of the modal cases (40 steps at ``tol = 1e-12``) the lowest mode of ``structured288`` at ``50
  dt_crit`` moves most: 4764 .. 5045 iterations around the plain run's 4772, because a draw decides in which steps the scale at
  the solved ``x`` asks for a second, short solve (64 solves in the plain run).  ``S = 5.89e-2``, ``implicit_edges.S_SPREAD = 0.059``.
  (While the linear solve was still accepted on the predictor's scale the same case gave 4456 .. 4551 around 4480.)
* ``max_cg``: the nonlinear ``svk`` run ends with reason 1 at the caps 1, 2 and 3 (25 Newton passes, residual 5.3e-8 / 8.4e-9 at
  3) and converges at 4 (22 .. 23 passes per step), 5 (16 .. 18 / 15 .. 16), 6 and 8; the counts did not move over the 8 draws.
  The linear material at ``tol = 1e-12`` needs 60 .. 64 iterations for a step's first solve; at the cap 20 it makes 4 passes per
  step.
* the guard: at the uniform compression ``u_x = -0.2 x`` with ``dt = 100 dt_crit`` ``K_T + s`` has 14 / 26 negative eigenvalues, the
  lowest -3.3e4 / -1.1e4; the PCG stops at iteration 14 / 31 with ``p . J p = -2.5e-2 / -5.7e-3`` of ``|p| |J p|``, the iterations
  before it at 2.6e-2 / 5.6e-3 or more."""
import numpy as np
import pytest

import finite_strain_double as fd
import implicit_double as imp
import implicit_edges as ie
import operator_extended as ox

EPS = ie.EPS


# ---- 1. the double that iterates --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_mirrored_double_lands_within_the_bar_of_the_nonlinear_case(name, material):
    """The 12 steps of ``implicit_double.nonlinear_run`` with the kernel's solves at ``tol = 1e-10``: within 1e-8 of ``max|d|`` of
    the direct double at 1e-13, the bar of ``test_nonlinear_run_against_the_double``.  (``delaunay2`` and ``curved288`` were measured
    too, see the header; they are left out of the suite for their time.)"""
    p = imp.problem(name)
    nm = ie.nonlinear_stepper(p, material)
    total, per_step, info = ie.run(nm, imp.NONLINEAR_STEPS)
    want = imp.nonlinear_reference(name, material)
    err = float(np.abs(nm.d - want).max() / np.abs(want).max())
    print(f"{name} {material}: {err:.2e} of max|d|", total, per_step)
    assert info["converged"] and total["steps_done"] == imp.NONLINEAR_STEPS and err <= 1e-8
    assert total["cg_iterations"] == sum(nm.cg_per_solve) and total["newton_iterations"] == len(nm.cg_per_solve)


@pytest.mark.parametrize("name", imp.MODAL_MESHES)
def test_mirrored_double_lands_within_the_bar_of_the_modal_cases(name):
    """The modal cases at ``tol = 1e-12``: the bar ``10 N tol kappa`` of ``test_linear_modes_turn_by_the_exact_discrete_angle``; one
    solve per step, taken at the recurrence residual, and a second short one where the scale at the solved ``x`` asks for it."""
    p = imp.problem(name)
    for j, factor in imp.modal_cases(p):
        dt = factor * p.dt_crit
        nm = ie.NewmarkPCG(p, p.mass, np.zeros(p.n), dt, 0.0, ramp=False, tol=1e-12)
        nm.set_state(p.mode(j))
        info = nm.step(imp.MODAL_STEPS)
        err = float(np.abs(nm.d - imp.modal_exact(p, j, dt, imp.MODAL_STEPS)).max())
        bar = 10 * imp.MODAL_STEPS * 1e-12 * imp.modal_kappa(p, dt)
        print(f"{name} mode {j}: {err:.2e} bar {bar:.2e}", info)
        assert info["converged"] and err <= bar and info["residual"] <= 1e-12
        assert imp.MODAL_STEPS <= info["newton_iterations"] <= 2 * imp.MODAL_STEPS


def test_iteration_counts_under_random_summation_orders():
    """``S``.  Every dot product and squared norm of :class:`NewmarkPCG` summed in a seeded random order, 8 draws: the spread of
    ``cg_iterations``, relative to the plain run.  Here on the cases that move at all and on the 3-step cases of the GPU
    tests (the header has all of them): the lowest mode of ``structured288`` at ``50 dt_crit`` gives ``S = 5.89e-2``; the nonlinear
    cases keep every Newton count and every PCG count, so no other start amplitude is needed."""
    spread = 0.0
    p = imp.problem("structured288")
    j, factor = imp.modal_cases(p)[0]
    counts = []
    for k in range(9):
        nm = ie.NewmarkPCG(p, p.mass, np.zeros(p.n), factor * p.dt_crit, 0.0, ramp=False, tol=1e-12,
                           order=None if k == 0 else np.random.default_rng(100 + k))
        nm.set_state(p.mode(j))
        counts.append(nm.step(imp.MODAL_STEPS)["cg_iterations"])
    spread = max(spread, (max(counts) - min(counts)) / counts[0])
    print("modal counts", counts, f"spread {spread:.3e}")
    for name in ie.EDGE_MESHES:
        for material in ("linear", "svk"):
            _, total, per_step = ie.mirror3(name, material)
            for k in range(1, 4):                                      # (8 draws were measured; 3 here, for the time)
                nm = ie.nonlinear_stepper(imp.problem(name), material, order=np.random.default_rng(100 + k))
                t, per, _ = ie.run(nm, ie.EDGE_STEPS)
                assert per == per_step, (name, material, per, per_step)
                spread = max(spread, abs(t["cg_iterations"] - total["cg_iterations"]) / total["cg_iterations"])
    assert 0.0 < spread <= ie.S_SPREAD < 0.1


# ---- 2. padding and the reductions ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_nodes", ie.PADDED_NODES)
def test_padded_meshes_put_live_dofs_where_the_passes_can_lose_them(n_nodes):
    """The map is strictly increasing and puts live dofs into the first and the last workgroup of both kinds of pass and,
    where the size has them, into a workgroup at or above 256 and behind item ``2048 * 256``; the sizes are the thresholds."""
    for name in ie.EDGE_MESHES:
        p = imp.problem(name)
        pts, cells, dd, node_map = ie.padded(p, n_nodes, n_nodes)
        assert pts.shape == (n_nodes, 3) and np.array_equal(pts[node_map], p.pts) and np.array_equal(cells, node_map[p.cells])
        assert np.array_equal(np.unique(cells), node_map) and len(np.unique(dd)) == len(p.dd)
        free = np.ones(3 * n_nodes, dtype=bool)
        free[dd] = False
        assert np.array_equal(free[ie.dof_map(node_map)], p.fs.free)
        for e in range(0, len(cells), 37):                             # ascending-element order of every node is kept
            assert np.array_equal(np.argsort(cells[e], kind="stable"), np.argsort(p.cells[e], kind="stable"))
        found = ie.places(p, node_map, n_nodes)
        want = found["wanted"]
        assert want["dof-fold"] == (3 * n_nodes > 65536) and want["node-fold"] == (n_nodes > 65536)
        assert want["dof-stride"] == (3 * n_nodes > 524288) and want["node-stride"] == (n_nodes > 524288)
        assert all(found[k] for k in want if want[k])
    assert ie.n_blocks(65536) == 256 and ie.n_blocks(65537) == 257 and ie.n_blocks(524288) == ie.n_blocks(524289) == 2048


def _accepted(name, material, tol=1e-6):
    """One step of the nonlinear case at ``tol``: ``(the stepper before, the stepper after, info)``."""
    p = imp.problem(name)
    nm = ie.nonlinear_stepper(p, material, tol=tol)
    before = (nm.d.copy(), nm.v.copy(), nm.a.copy())
    info = nm.step(1)
    assert info["converged"]
    return before, nm, info


@pytest.mark.parametrize("material", ("linear",) + tuple(fd.MATERIALS))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_residual_margin_and_the_fold_mutants(name, material):
    """Check (c).  The reported residual of one step at ``tol = 1e-6`` against ``|r| / ref`` evaluated afresh: the double's own float64
    evaluation against the longdouble one (``f_int`` and every sum in longdouble) at the double's accepted ``x`` differ by 2.1e-11
    .. 5.9e-8 of the residual (largest: ``curved288 neo_hookean``, residual 6.4e-8; the residuals are 6.4e-8 .. 6.8e-7); ten times
    the largest, rounded up, is ``implicit_edges.RESIDUAL_MARGIN = 1e-6``, 3900 times below the 1 / 257 of one dropped partial of
    a uniform field.  The linear material's reported figure - the recurrence residual over the scale at the solved ``x`` - is
    the fresh one to 1.6e-16 of it.  A fold that drops the partials at and above 256, and a stride loop that makes one trip,
    move the figure by more than ten times the margin (3.2e-5 of it or more: at ``N = 65537`` and ``174763`` one node alone sits
    behind the edge) at every padded size that has such partials or such a trip - and by nothing at the sizes below."""
    p = imp.problem(name)
    (d0, v0, a0), nm, info = _accepted(name, material)
    args = (p, material, nm.mass, nm.load, nm.dt, nm.alpha, 1.0, d0, v0, a0, nm.d)
    r64, rld = ie.true_residual(*args), ie.true_residual(*args, T=np.longdouble)
    own = abs(r64 - rld) / rld
    print(f"{name} {material}: reported {info['residual']:.3e} float64 {r64:.3e}; float64 - longdouble {own:.2e} of it, "
          f"reported - float64 {abs(info['residual'] - r64) / r64:.2e}")
    assert 1e-9 < info["residual"] <= 1e-6
    assert 10 * own <= ie.RESIDUAL_MARGIN and abs(info["residual"] - rld) <= ie.RESIDUAL_MARGIN * rld
    assert ie.RESIDUAL_MARGIN <= 1e-3 / 257
    # the mutants, on the sums the kernels form: the three reference norms and |r| of the node pass, |r_cg| of the dof pass
    f = nm.force(nm.d)[0]
    v1, a1 = 2.0 / nm.dt * (nm.d - d0) - v0, 4.0 / nm.dt ** 2 * (nm.d - d0 - nm.dt * v0) - a0
    ine = nm.mass * (a1 + nm.alpha * v1)
    terms = [np.where(p.live, x, 0.0) ** 2 for x in (nm.load - f - ine, nm.load, f, ine)]
    for n_nodes in ie.PADDED_NODES:
        node_map = ie.padded(p, n_nodes, n_nodes)[3]
        dofs = ie.dof_map(node_map)

        def figure(mutant):
            sums = [ie.kernel_sum(dofs // 3, t, n_nodes, mutant) for t in terms]
            if material == "linear":                                   # |r_cg| comes from the dof-wise update pass
                sums[0] = ie.kernel_sum(dofs, terms[0], 3 * n_nodes, mutant)
            return np.sqrt(sums[0]) / np.sqrt(max(sums[1:]))

        true = figure(None)
        assert abs(true - r64) <= 1e-12 * r64
        want = ie.places(p, node_map, n_nodes)["wanted"]
        for mutant, hit in (("fold", want["node-fold"] or (material == "linear" and want["dof-fold"])),
                            ("tail", want["node-stride"] or (material == "linear" and want["dof-stride"]))):
            moved = abs(figure(mutant) - true) / true
            assert (moved > 10 * ie.RESIDUAL_MARGIN) if hit else (moved == 0.0), (n_nodes, mutant, moved)


@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_fold_mutants_fail_the_dot_of_the_shifted_apply(name):
    """Check (a): ``dot`` of the node pass within ``64 eps sum|v_i out_i|``.  With the mutants the sum moves by 1e-3 of that size
    or more wherever the padded size has partials at and above 256, or a second trip."""
    p = imp.problem(name)
    u, v = ie.apply_vectors(p)
    out = np.where(p.fs.free, p.fs.tangent_matrix(u, "svk") @ v + ie.apply_shift(p, v) * v, 0.0)
    prod = v * out
    for n_nodes in ie.PADDED_NODES:
        node_map = ie.padded(p, n_nodes, n_nodes)[3]
        nodes = ie.dof_map(node_map) // 3
        want = ie.places(p, node_map, n_nodes)["wanted"]
        true, bar = ie.kernel_sum(nodes, prod, n_nodes), 64 * EPS * float(np.abs(prod).sum())
        assert abs(true - float(prod.sum())) <= bar
        for mutant, hit in (("fold", want["node-fold"]), ("tail", want["node-stride"])):
            moved = abs(ie.kernel_sum(nodes, prod, n_nodes, mutant) - true)
            assert (moved > 1e6 * bar) if hit else (moved == 0.0), (n_nodes, mutant, moved, bar)


# ---- 3. the solver controls -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_iteration_caps_give_both_outcomes(name):
    """``max_cg``: ``svk`` at the cap ``CAP_FAILS = 3`` ends the first step with reason 1 after 25 passes of 3 iterations and keeps the
    state; at ``CAP_CONVERGES = 5`` it converges in 15 .. 18 passes per step, to the 1e-8 bar.  The linear material at ``tol = 1e-12``
    and ``CAP_LINEAR = 20`` - its solve needs 60 or more - makes 4 passes per step and ends within ``10 N tol kappa`` of the direct
    double.  None of the counts moves over 8 draws of summation orders (measured; one draw here)."""
    p = imp.problem(name)
    nm = ie.nonlinear_stepper(p, "svk", max_cg=ie.CAP_FAILS)
    before = (nm.d.copy(), nm.v.copy(), nm.a.copy(), nm.t)
    info = nm.step(3)
    assert (info["reason"], info["steps_done"], info["newton_iterations"], info["cg_iterations"]) == (1, 0, 25, 25 * ie.CAP_FAILS)
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], (nm.d, nm.v, nm.a))) and nm.t == before[3]
    runs = []
    for k in range(2):
        nm = ie.nonlinear_stepper(p, "svk", max_cg=ie.CAP_CONVERGES, order=None if k == 0 else np.random.default_rng(100 + k))
        total, per_step, info = ie.run(nm, ie.EDGE_STEPS)
        assert info["converged"] and max(nm.cg_per_solve) == ie.CAP_CONVERGES and 10 <= min(per_step) and max(per_step) < 25
        runs.append((total["cg_iterations"], tuple(per_step)))
        if k == 0:
            want = ie.reference3(name, "svk")
            assert np.abs(nm.d - want).max() <= 1e-8 * np.abs(want).max()
    assert len(set(runs)) == 1, runs
    free = ie.nonlinear_stepper(p, "linear", tol=1e-12)
    assert ie.run(free, ie.EDGE_STEPS)[2]["converged"] and free.cg_per_solve[0] > 2 * ie.CAP_LINEAR
    nm = ie.nonlinear_stepper(p, "linear", tol=1e-12, max_cg=ie.CAP_LINEAR)
    total, per_step, info = ie.run(nm, ie.EDGE_STEPS)
    direct = ie.linear_direct3(name)
    err, bar = float(np.abs(nm.d - direct).max() / np.abs(direct).max()), 10 * ie.EDGE_STEPS * 1e-12 * imp.modal_kappa(p, nm.dt)
    print(f"{name}: linear at the cap {ie.CAP_LINEAR}: {per_step} passes, {err:.2e} bar {bar:.2e}")
    assert info["converged"] and min(per_step) >= 3 and err <= bar


@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_guard_case_has_negative_curvature_and_stops_robustly(name):
    p = imp.problem(name)
    u, dt, k, trace, info = ie.guard_case(name)
    J = p.fs.tangent_matrix(u, "svk")[np.ix_(p.idx, p.idx)] + np.diag(4.0 / dt ** 2 * p.mass[p.idx])
    w = np.linalg.eigvalsh(J)
    measure = [pap / (a * b) for pap, a, b in trace]
    print(f"{name}: lowest eigenvalue {w[0]:.3e}, {int((w < 0).sum())} negative; stops at iteration {k + 1}: {measure[-1]:.2e}, "
          f"before it at least {min(measure[:-1]):.2e}")
    assert w[0] < -1e-3 * w[-1] and float(p.fs.det_f(u).min()) > 0.5
    assert len(trace) == k + 1 and k >= 5 and measure[-1] <= -1e-6 and min(measure[:-1]) >= 1e-6
    assert (info["reason"], info["steps_done"], info["newton_iterations"], info["cg_iterations"]) == (1, 0, 1, k)


# ---- 4. time ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_ramp_across_one_and_the_late_clamp_mutant(name, material):
    """``ramp=True`` from ``t = 1 - 1.5 dt``, 3 steps: the scales are ``1 - dt/2``, 1, 1.  The mirrored double is within the bar of the
    direct one (linear at ``tol = 1e-12``: ``10 N tol kappa``; ``svk``: 1e-8); the mutant that clamps by the time before the step -
    scale ``1 + dt/2`` in the second step - misses it by a factor of 1000 or more."""
    p = imp.problem(name)
    want, bar, kw = ie.time_reference(name, material, "ramp")
    got = ie.time_run(ie.NewmarkPCG, p, material, "ramp", **kw)
    bad = ie.time_run(ie.NewmarkPCG, p, material, "ramp", late_clamp=True, **kw)
    e1, e2 = (float(np.abs(x.d - want.d).max() / np.abs(want.d).max()) for x in (got, bad))
    print(f"{name} {material}: {e1:.2e}, mutant {e2:.2e}, bar {bar:.2e}")
    assert abs(want.t - (1.0 + 1.5 * want.dt)) < 1e-12 and got.t == want.t
    assert got.last["converged"] and bad.last["converged"] and e1 <= bar and e2 > 5 * bar


@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_set_dt_in_mid_run_and_the_old_shift_mutant(name, material):
    """2 steps at ``5 dt_crit``, ``set_dt(12.5 dt_crit)``, 2 steps.  The mutant that keeps the old shift solves the linear material's
    one system with the wrong matrix and misses the bar by a factor of 1000 or more; under ``svk`` the residual is still the
    right one, so Newton converges to the right state with a wrong Jacobian - in more passes, which the count rule of the GPU
    test (equal Newton counts per step) catches."""
    p = imp.problem(name)
    want, bar, kw = ie.time_reference(name, material, "set_dt")
    got = ie.time_run(ie.NewmarkPCG, p, material, "set_dt", **kw)
    bad = ie.time_run(ie.NewmarkPCG, p, material, "set_dt", keep_shift=True, **kw)
    e1, e2 = (float(np.abs(x.d - want.d).max() / np.abs(want.d).max()) for x in (got, bad))
    print(f"{name} {material}: {e1:.2e}, mutant {e2:.2e}, bar {bar:.2e}; Newton per step", got.newton_per_step, bad.newton_per_step)
    assert abs(want.t - 35.0 * p.dt_crit) < 1e-12 and e1 <= bar and got.last["converged"] and len(got.newton_per_step) == 4
    if material == "linear":
        assert bad.last["converged"] and e2 > 1000 * bar
    else:
        assert bad.newton_per_step[:2] == got.newton_per_step[:2]
        assert not bad.last["converged"] or bad.newton_per_step[2:] != got.newton_per_step[2:]


# ---- 5. scales --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", ox.UNITS)
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_mirrored_double_commutes_bitwise_with_power_of_two_units(name, u):
    """The reference of the GPU's units test commutes itself: 3 nonlinear (``svk``) and 3 linear steps in the units ``u`` are the
    unscaled ones times ``2^(40 u)``, 1, ``2^(-40 u)`` bit for bit with equal counts, and no nonzero intermediate - the squared norms
    and ``4 / dt^2`` among them - leaves ``[1e-290, 1e290]`` (seen: 4e-79 .. 2e83 over both meshes and units)."""
    for material in ("svk", "linear"):
        seen = [np.inf, 0.0]
        base, total0, per0 = ie.units_run(name, material, 0)
        got, total, per = ie.units_run(name, material, u, seen=seen)
        print(f"{name} {material} u = {u:+d}: intermediates {seen[0]:.1e} .. {seen[1]:.1e}", total)
        assert 1e-290 <= seen[0] and seen[1] <= 1e290
        assert (total, per) == (total0, per0)
        for key, x, y in zip(("d", "v", "a"), got, base):
            assert np.abs(y).max() > 0 and np.array_equal(x, y * ie.unit(key, u)), (material, key)


@pytest.mark.parametrize("material", ("linear", "svk"))
@pytest.mark.parametrize("family", ie.OFF_BEAM)
@pytest.mark.parametrize("name", ie.EDGE_MESHES)
def test_off_beam_cases_converge_and_their_residual_resolves(name, family, material):
    """``nu = 0.499999`` and the ``sliver 1e-6`` family: one step of the nonlinear case (start amplitude
    ``implicit_edges.OFF_BEAM_AMPLITUDE``) at ``tol = 1e-6`` converges in the mirrored double, and float64 resolves the accepted
    residual: against the longdouble evaluation it differs by at most ``OFF_BEAM_MARGIN / 10`` of itself.  Measured: ``nu`` 6.6e-12
    .. 3.7e-9; slivers 8.0e-10 / 7.6e-9 (``structured288`` linear / ``svk``), 5.5e-7 / 3.8e-6 (``curved288``, 17 Newton passes under ``svk``):
    ``OFF_BEAM_MARGIN = 5e-5``, 78 times below 1 / 257 - less far than on the unit beam."""
    p = ie.off_beam_problem(name, family)
    nm = ie.nonlinear_stepper(p, material, tol=1e-6, amplitude=ie.OFF_BEAM_AMPLITUDE)
    d0, v0, a0 = nm.d.copy(), nm.v.copy(), nm.a.copy()
    info = nm.step(1)
    args = (p, material, nm.mass, nm.load, nm.dt, nm.alpha, 1.0, d0, v0, a0, nm.d)
    r64, rld = ie.true_residual(*args), ie.true_residual(*args, T=np.longdouble)
    own = abs(r64 - rld) / rld
    print(f"{p.name} {material}: {info}; float64 {r64:.3e}, float64 - longdouble {own:.2e} of it; dt_crit {p.dt_crit:.3e}, "
          f"PCG per solve {nm.cg_per_solve}")
    assert info["converged"] and info["residual"] <= 1e-6
    assert 10 * own <= ie.OFF_BEAM_MARGIN and abs(info["residual"] - rld) <= ie.OFF_BEAM_MARGIN * rld
