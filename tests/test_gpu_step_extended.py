"""The production step kernels (csrc/saa_kernels.hip: ``fused_step_kernel`` plain and ``FORCE_ONLY``, ``persistent_steps_kernel`` =
the resident kernel, ``det_items_kernel`` / ``det_nodes_kernel``, ``iface_finish_kernel``, ``halo_overwrite_kernel``) and the set-up
kernels (csrc/saa_setup.hip) off the unit beam, through ``HipExplicitSolver``, against the extended-precision reference of
tests/step_extended.py.

The bar, per output column (a trajectory: per step and state): ``err = max|y - r| / max|r| <= 1e-12 + 8 env``.
tests/test_step_extended.py shows on the CPU that every case qualifies for it and that four mutants miss it.  Every test
prints ``err``, ``env``, ``err / env`` and ``err / bar`` of its worst column per path before it asserts; every solver has
``wait_timeout_s = 5``; every caller-owned device buffer (recorder, force output, history, interface buffer, table) carries 64
sentinel doubles after its end.

* Force: ``internal_force`` and ``internal_force_device`` on the five ``ox`` columns, both plans, atomic and deterministic, against
  the unmasked ``K X``.
* One step: ``step(1)`` (one launch per step), fused and deterministic, both plans, every case and variant, both states; ``d1``
  of ``get_state()`` is recorder column 0 bit for bit, the new ``dn`` the old ``d0``, ``tn == tn0 + dt``.
* Eight steps (the fewest that run resident): resident, fused and deterministic, every recorder column against the
  reference step it belongs to; on plan A (one wave per workgroup) resident and fused are the same bits in every column and
  in ``tn``, which is the repeated sum (``cross1``: across the ramp's kink).
* Partitions: ranks in one process (``step_begin``, the interface buffers summed in rank order, ``step_finish(hist, 0)``,
  ``step_predicted(1, table, ...)`` from the same state), fused and deterministic; slots the rank does not hold are exactly 0
  after ``step_finish`` (three more slots than anybody holds carry garbage into it), a shared dof's ``d1`` is the same bits on
  all its holders.
* Units (``sx.scaled_case``, the runs of ``step_extended.UNIT_RUNS``): bitwise where the summation order is fixed (deterministic;
  plan A), under the bar elsewhere; ``device_setup_fields`` bitwise.
* Set-up fields under the bar on every case.
* The comparison itself: a solver given ``tn + dt`` and held to the reference of ``tn`` misses the bar.

Measured on an MI355X when these tests were written (DESIGN.md section 13 has the table): no kernel misses; the worst column
is at 0.0047 of its bar (4.9e-15, ``nu = 0.499999``, eight steps), the slivers at 3.4e-12 where ``env`` is 2e-10, the shift by 2^20 at
2.9e-15.  The late ramp misses by 3.4e3 x (``nu = 0.3``) and 2.8 x (shift 2^20) after one step.  Hand-made mutants of the library
that turn tests of this file red: ``tet_core`` without its Newton step (58 of 122); the resident kernel's ramp not clamped at 1
(``cross1``, ``tn1.5``, units); ``iface_finish_kernel`` without its clamp (the mod-3 partitions).  The resident kernel's ``tn`` as ``tn0 + (s +
1) dt`` is not seen in 8 steps from ``tn = 0.37`` (the same bits); tests/test_gpu_step_edges.py sees it after 200."""
import numpy as np
import pytest

import operator_extended as ox
import step_extended as stx
import stepper_extended as sx

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -1.2345e300
GUARD = 64
WAIT_S = 5.0


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


class Guarded:
    """``rows x cols`` doubles (``view``; ``cols = 0``: a vector) with 64 sentinels after their end."""

    def __init__(self, rows, cols=0, values=None):
        import torch

        self.n = int(rows) * max(int(cols), 1)
        self.whole = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
        self.view = self.whole[:self.n].view(int(rows), int(cols)) if cols else self.whole[:self.n]
        self.view.zero_()
        if values is not None:
            self.view.copy_(_dev(values).reshape(self.view.shape))

    def intact(self):
        return bool((self.whole[self.n:] == SENTINEL).all())

    def host(self):
        return self.view.cpu().numpy()


def _family(key):
    (_, fam, val), variant = key
    return f"{fam} {val:g}" if variant == "base" else variant


def _report(key, path, err, env, ratio):
    """One line per test and path for the table of DESIGN.md section 13."""
    print(f"TABLE|{_family(key)}|{path}|{err:.3e}|{err / max(env, 1e-300):.3e}|{ratio:.3e}")


def make_solver(case, plan, points=None, cells=None, dof=None, dirichlet=None, **shared):
    import torch

    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver

    dof = slice(None) if dof is None else dof
    sol = HipExplicitSolver(case["points"] if points is None else points, case["cells"] if cells is None else cells,
                            case["mass"][dof], case["load"][dof], case["dirichlet"] if dirichlet is None else dirichlet,
                            case["lmd"], case["mu"], case["dt"], case["alpha"], ramp=case["ramp"], **stx.PLANS[plan], **shared)
    sol.set_option("wait_timeout_s", WAIT_S)
    sol.set_stream(torch.cuda.current_stream().cuda_stream)           # the guarded buffers are filled on this stream
    return sol


def _mode(sol, path):
    sol.set_resident_kernel(path == "resident")
    sol.set_deterministic(path == "deterministic")
    if path == "resident":
        assert sol.resident_kernel_info()["capable"]


def run_steps(sol, case, j, n, path, tn=None):
    """``n`` steps from state ``j`` on a path: ``(recorder columns (n, n_dof), tn)``; asserts what is bitwise."""
    _mode(sol, path)
    tn0 = case["tn"] if tn is None else tn
    rec = Guarded(sol.n_dof, n)
    sol.set_state(case["d0"][j], case["dn"][j], tn0)
    sol.set_recorder(rec.view, 1, 0)
    sol.step(n)
    sol.synchronize()                                                  # raises if a bounded wait gave up
    d1, dn, tn = sol.get_state()
    sol.set_recorder(None)
    cols = rec.host().T
    assert rec.intact()
    assert np.array_equal(cols[-1], d1[:, 0])                          # the state is the last recorded column
    assert np.array_equal(dn[:, 0], cols[-2] if n > 1 else case["d0"][j])
    want = tn0
    for _ in range(n):
        want = want + case["dt"]
    assert tn == want                                                  # the repeated sum
    return cols, tn


def _trajectories(sol, case, n, path):
    return np.stack([run_steps(sol, case, j, n, path)[0] for j in range(2)], axis=1)      # (n, 2, n_dof)


# ---- force ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", stx.case_ids(), ids=ox.case_name)
def test_internal_force_is_within_the_bar(cid):
    ocase, ref, env = stx.force_reference(cid)
    case = stx.build_case(cid)
    bad = []
    for plan in stx.PLANS:
        sol = make_solver(case, plan)
        for path in ("fused", "deterministic"):
            _mode(sol, path)
            host = np.stack([sol.internal_force(x)[:, 0] for x in ocase["X"]])
            out = [Guarded(sol.n_dof) for _ in ocase["X"]]
            for x, g in zip(ocase["X"], out):
                sol.internal_force_device(_dev(x), g.view)
            sol.synchronize()
            assert all(g.intact() for g in out)
            device = np.stack([g.host() for g in out])
            if path == "deterministic":
                assert np.array_equal(device, host)
            for what, got in (("host", host), ("device", device)):
                e, v, r, b = stx.hold(got, ref, env, ox.KERNEL_FACTOR, f"{ox.case_name(cid)} K X plan {plan} {path} {what}")
                _report((cid, "base"), "force", e, v, r)
                bad += b
        sol.close()
    assert not bad, bad


# ---- one step, eight steps -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", stx.case_keys(), ids=stx.key_name)
def test_one_step_is_within_the_bar(key):
    case, ref, env = stx.reference(*key)
    bad = []
    for plan in stx.PLANS:
        sol = make_solver(case, plan)
        assert sol.plan_stats()["n_blocks"] > 1
        for path in ("fused", "deterministic"):
            got = _trajectories(sol, case, 1, path)
            e, v, r, b = stx.hold(got, ref, env, ox.KERNEL_FACTOR, f"{stx.key_name(key)} 1 step plan {plan} {path}", steps=[0])
            _report(key, path, e, v, r)
            bad += b
        sol.close()
    assert not bad, bad


@pytest.mark.parametrize("key", stx.case_keys(), ids=stx.key_name)
def test_eight_steps_are_within_the_bar_in_every_column(key):
    case, ref, env = stx.reference(*key)
    bad = []
    for plan in stx.PLANS:
        sol = make_solver(case, plan)
        if plan == "A":
            assert sol.plan_stats()["threads"] == 64
        got = {}
        for path in ("resident", "fused", "deterministic"):
            got[path] = _trajectories(sol, case, stx.N_STEPS, path)
            e, v, r, b = stx.hold(got[path], ref, env, ox.KERNEL_FACTOR, f"{stx.key_name(key)} 8 steps plan {plan} {path}")
            _report(key, path, e, v, r)
            bad += b
        if plan == "A":                                                # one wave: LDS adds in program order (tn: run_steps)
            assert np.array_equal(got["resident"], got["fused"])
        sol.close()
    assert not bad, bad


# ---- partitions ----------------------------------------------------------------------------------------------------------

N_EXTRA, GARBAGE = 3, 3.0e7


def run_partition(case, path):
    """The per-rank outputs of ``stx.partition_reference`` from one ``HipExplicitSolver`` per rank; asserts what is bitwise."""
    import torch

    lays, n_gs = case["layouts"], case["n_gs"]
    n_all = n_gs + N_EXTRA                                             # the last slots: held by nobody
    out = {name: [None, None] for name in stx.rank_names(case)}
    sols = []
    try:
        for lay in lays:
            sol = make_solver(case, "B", points=case["points"][lay.nodes], cells=lay.cells_local, dof=lay.local_dof,
                              dirichlet=lay.dirichlet_dofs, shared_local=lay.shared_local, shared_slots=lay.shared_slots,
                              n_global_shared=n_all)
            _mode(sol, path)
            sols.append(sol)
        ifaces = [Guarded(3 * n_all) for _ in sols]
        for sol, g in zip(sols, ifaces):
            sol.set_interface_buffer(g.view)
        held = []
        nobody = torch.ones(3 * n_all, dtype=torch.bool, device=DEV)
        for lay in lays:
            slots = torch.as_tensor(np.asarray(lay.shared_slots, dtype=np.int64), device=DEV)
            gd = (3 * slots[:, None] + torch.arange(3, device=DEV)[None, :]).reshape(-1)
            mask = torch.zeros(3 * n_all, dtype=torch.bool, device=DEV)
            mask[gd] = True
            nobody &= ~mask
            held.append((gd, mask, np.asarray(lay.loc_dof_shared, dtype=np.int64)))
        assert int(nobody.sum()) == 3 * N_EXTRA
        for j in range(2):
            def start(i):
                dof = lays[i].local_dof
                sols[i].set_state(case["d0"][j][dof], case["dn"][j][dof], case["tn"])

            # one synchronised step
            hists = [Guarded(3 * len(lay.shared_local)) for lay in lays]
            for i, sol in enumerate(sols):
                start(i)
                ifaces[i].view.zero_()
                sol.step_begin()
            for sol in sols:
                sol.synchronize()
            total = torch.zeros(3 * n_all, dtype=torch.float64, device=DEV)
            for g in ifaces:                                           # rank order
                total += g.view
            total[nobody] = GARBAGE
            for i, sol in enumerate(sols):
                ifaces[i].view.copy_(total)
                sol.step_finish(hists[i].view, 0)
                sol.synchronize()
            seen = np.full(3 * n_all, np.nan)
            for i, sol in enumerate(sols):
                d1, dn, tn = sol.get_state()
                gd, mask, loc = held[i]
                assert ifaces[i].intact() and hists[i].intact()
                assert np.array_equal(dn[:, 0], case["d0"][j][lays[i].local_dof]) and tn == case["tn"] + case["dt"]
                assert not bool(ifaces[i].view[~mask].any())           # slots the rank does not hold: exactly 0
                assert torch.equal(ifaces[i].view[mask], total[mask])
                free = case["free"][sx._global_shared_dofs(lays[i])]
                p = f"r{i}."
                out[p + "d1"][j], out[p + "hist"][j] = d1[:, 0], hists[i].host()
                out[p + "iface"][j] = total[gd].cpu().numpy() * free    # (a clamped dof's slot: unmasked sums, unread)
                assert np.array_equal(hists[i].host(), d1[loc, 0])
                g = gd.cpu().numpy()
                first = np.isnan(seen[g])
                assert np.array_equal(seen[g][~first], d1[loc, 0][~first])  # the same bits on all holders
                seen[g] = d1[loc, 0]
            # one predicted step from the same state
            for i, sol in enumerate(sols):
                start(i)
                table = Guarded(3 * len(lays[i].shared_local), values=case["tables"][i][j])
                hist = Guarded(3 * len(lays[i].shared_local))
                sol.step_predicted(1, table.view, 0, hist.view, 0)
                sol.synchronize()
                d1, dn, tn = sol.get_state()
                assert table.intact() and hist.intact() and ifaces[i].intact()
                assert np.array_equal(hist.host(), case["tables"][i][j]) and np.array_equal(table.host(), case["tables"][i][j])
                assert np.array_equal(d1[held[i][2], 0], case["tables"][i][j])
                assert np.array_equal(dn[:, 0], case["d0"][j][lays[i].local_dof]) and tn == case["tn"] + case["dt"]
                out[f"r{i}.p.d1"][j], out[f"r{i}.p.hist"][j] = d1[:, 0], hist.host()
    finally:
        for sol in sols:
            sol.close()
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("key", stx.partition_keys(), ids=stx.key_name)
def test_partition_steps_are_within_the_bar(key):
    case, ref, env = stx.partition_reference(*key)
    bad = []
    for path in ("fused", "deterministic"):
        got = run_partition(case, path)
        assert sorted(got) == sorted(ref)
        for name in stx.rank_names(case):
            e, v, r, b = stx.hold(got[name], ref[name], env[name], ox.KERNEL_FACTOR, f"{stx.key_name(key)} {path} {name}")
            _report((key[0], "base"), "partitions", e, v, r)
            bad += [(name,) + x for x in b]
    assert not bad, bad


# ---- units ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("mesh", ox.MESHES_P1)
def test_power_of_two_units(mesh, u):
    from synchronization_avoiding_algorithms_amd import fem_setup as fs

    cid = (mesh, "nu", 0.3)
    L = 2.0 ** (40 * u)
    differ, bad = [], []
    for variant, n in stx.UNIT_RUNS:
        case, ref, env = stx.reference(cid, variant)
        scaled = sx.scaled_case(case, u)
        for plan in stx.PLANS:
            base_sol, sol = make_solver(case, plan), make_solver(scaled, plan)
            for path in (("resident",) if n >= stx.N_STEPS else ()) + ("fused", "deterministic"):
                base, got = _trajectories(base_sol, case, n, path), _trajectories(sol, scaled, n, path)
                assert np.isfinite(got).all()
                label = f"{stx.key_name((cid, variant))} u {u:+d} plan {plan} {path}"
                if path == "deterministic" or plan == "A":             # a fixed summation order: the same bits
                    if not np.array_equal(got, base * L):
                        differ.append((label, int((got != base * L).sum())))
                else:
                    bad += stx.hold(got / L, ref, env, ox.KERNEL_FACTOR, label, steps=range(n))[3]
            base_sol.close()
            sol.close()
    case = stx.build_case(cid)
    S = sx.scaled_case(case, u)
    m0, f0, e0 = fs.device_setup_fields(case["points"], case["cells"].astype(np.int32), case["rho"], stx.FZ)
    m1, f1, e1 = fs.device_setup_fields(S["points"], case["cells"].astype(np.int32), S["rho"], stx.FZ * 2.0 ** (-20 * u))
    for name, a, b, ex in (("mass", m0, m1, 140), ("load", f0, f1, 100), ("edge", e0, e1, 40)):
        if not np.array_equal(np.asarray(b), np.asarray(a) * 2.0 ** (ex * u)):
            differ.append((f"device_setup_fields {name}", int(np.sum(np.asarray(b) != np.asarray(a) * 2.0 ** (ex * u)))))
    print(mesh, u, "runs that differ:", differ)
    assert not differ, differ
    assert not bad, bad


# ---- set-up fields -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", stx.case_ids(), ids=ox.case_name)
def test_setup_fields_are_within_the_bar(cid):
    from synchronization_avoiding_algorithms_amd import fem_setup as fs

    case, ref, env = stx.setup_reference(cid)
    mass, load, edge = fs.device_setup_fields(case["points"], case["cells"].astype(np.int32), case["rho"], stx.FZ)
    got = {"mass": mass.reshape(1, -1), "load": load.reshape(1, -1), "edge": np.array([[edge]])}
    bad = []
    for name in ("mass", "load", "edge"):
        e, v, r, b = stx.hold(got[name], ref[name], env[name], ox.KERNEL_FACTOR, f"{ox.case_name(cid)} set-up {name}")
        _report((cid, "base"), "set-up", e, v, r)
        bad += [(name,) + x for x in b]
    f = load.reshape(-1, 3)
    assert (f[:, 0] == 0).all() and not np.signbit(f[:, 0]).any() and np.array_equal(f[:, 1], f[:, 2])   # the compact forms
    m = mass.reshape(-1, 3)
    assert np.array_equal(m[:, 0], m[:, 1]) and np.array_equal(m[:, 0], m[:, 2])
    assert not bad, bad


# ---- the comparison itself -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [("structured2", "nu", 0.3), ("structured2", "shift", 20)], ids=ox.case_name)
def test_the_comparison_sees_a_ramp_read_one_step_late(cid):
    """The CPU mutant ``ramp_late`` through the GPU: the solver is given ``tn + dt`` and held to the reference of ``tn``."""
    case, ref, env = stx.reference(cid)
    sol = make_solver(case, "B")
    for path, n in (("fused", 1), ("resident", stx.N_STEPS)):
        got = np.stack([run_steps(sol, case, j, n, path, tn=case["tn"] + case["dt"])[0] for j in range(2)], axis=1)
        _, _, ratio, bad = stx.hold(got, ref, env, ox.KERNEL_FACTOR, f"{ox.case_name(cid)} late ramp {path}", steps=range(n))
        assert bad and ratio > 1, (path, ratio)
    sol.close()
