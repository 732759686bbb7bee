"""The operator stepper's kernels (csrc/saa_opstep.hip: ``opstep_node_kernel<MODE, ENERGY>``, ``opstep_finish_kernel<ENERGY>`` with
``opstep_update_dof``, the HRZ and row-sum mass kernels, ``opstep_elem_p2_kernel`` with its geometry table, the energy partials
and ``opstep_energy_final_kernel``) off the unit beam, one step at a time, against the extended-precision reference of
tests/stepper_extended.py.

The bar, per output and column (the two columns are the *random* and the *smooth* state): ``err = max|y - r| / max|r| <= 1e-12 + 8
env``; a column whose reference is exactly 0 must be exactly 0.  tests/test_stepper_extended.py shows on the CPU that every
case qualifies for the bar and that four mutants miss it.  Each test prints ``err``, ``env`` and ``err / env`` per output.

* The whole mesh: every id of ``ox.case_ids()`` at ``alpha = 0.5`` and the damping / ramp variants at ``nu = 0.3``; order 2 with
  ``stored_geometry`` 0 and 1.  ``lumped_mass`` against ``mass``; one step from each state with the balance on and off: ``d1`` (from
  ``state()``, bit-equal to recorder column 0 and between on and off) and the energy row; the new ``dn`` is the old ``d0`` bitwise.
* Partitions (two slabs; element index mod 3: three holders, foreign slots on every rank), the ranks stepped in one process
  with ``dynamics.sum_interfaces``: every per-rank output of a synchronised and of a predicted step, the shares summed over the
  ranks against the whole-mesh row, foreign slots exactly 0 after ``step_finish``, a shared dof's ``d1`` bitwise equal on all its
  holders.
* Units: bitwise, no bar.
* The comparison itself: the stepper given ``tn + dt`` must miss the bar where the CPU mutant of the late ramp does.
* Launch edges: sub-meshes of one element and of 255, 256, 257 nodes (``kThreads`` = 256 lanes, one per node); fake shared sets
  of 1, 85 and 86 nodes (255 and 258 lanes, one per shared dof) among 1 and 100 more slots than the rank holds.  Every
  caller-owned buffer (recorder, history, interface buffer, table) carries 64 sentinel doubles after its end."""
import numpy as np
import pytest

import operator_extended as ox
import stepper_extended as sx

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -1.2345e300
GUARD = 64


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _host(t):
    return t.cpu().numpy()


class Guarded:
    """``n`` doubles (``view``) with 64 sentinels after their end."""

    def __init__(self, n, values=None):
        import torch

        self.n = int(n)
        self.whole = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
        self.view = self.whole[:self.n]
        self.view.zero_()
        if values is not None:
            self.view.copy_(_dev(values).reshape(-1))

    def intact(self):
        return bool((self.whole[self.n:] == SENTINEL).all())


def _energy_columns(rows, prefix=""):
    """``rows (2, 5)``, one recorded row per state (``W``, ``D`` run from 0: the step's own ``dW``, ``dD``)."""
    rows = np.asarray(rows)
    return {prefix + name: rows[:, c:c + 1] for c, name in enumerate(sx.ENERGY)}


def run_whole(case, stored=None):
    """The whole-mesh outputs of ``sx.outputs`` from ``ModalOperator`` and ``OperatorStepper``; asserts what is bitwise."""
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    out, n_dof = {}, 3 * len(case["points"])
    with ModalOperator(case["points"], case["cells"].astype(np.int32), case["dirichlet"], case["lmd"], case["mu"], case["rho"]) as op:
        out["mass"] = _host(op.lumped_mass())[None]
        with OperatorStepper(op, case["mass"], case["load"], case["dt"], case["alpha"], ramp=case["ramp"]) as st:
            if stored is not None:
                st.set_option("stored_geometry", float(stored))
            d1s, rows = [], []
            for j in range(2):
                d0, dn = _dev(case["d0"][j]), _dev(case["dn"][j])
                got = {}
                for energy in (True, False):
                    st.set_state(d0, dn, case["tn"])
                    rec = Guarded(n_dof)
                    traj = st.record(1, out=rec.view)
                    e = st.record_energy(1 if energy else 0)
                    st.step(1)
                    new0, newn, tn = st.state()
                    assert rec.intact()
                    assert torch.equal(traj[:, 0], new0) and torch.equal(newn, d0)  # recorder column 0; dn is the old d0
                    assert tn == case["tn"] + case["dt"]
                    got[energy] = new0
                    if energy:
                        rows.append(_host(e[0]))
                assert torch.equal(got[True], got[False])               # the balance does not touch the state
                d1s.append(_host(got[True]))
    out["d1"] = np.array(d1s)
    out.update(_energy_columns(rows))
    return out


def run_partition(case, stored=None, garbage=None):
    """The per-rank outputs of ``sx.outputs`` from ``OperatorRank``: a synchronised step (``step_begin``, ``sum_interfaces``,
    ``step_finish``) and a predicted one from each state, balance on and off; asserts what is bitwise.  ``garbage``: written
    into the slots that no rank holds before ``step_finish`` (what a reduction over more ranks would leave there)."""
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorRank, sum_interfaces

    lays, n_gs = case["layouts"], case["n_gs"]
    out = {f"r{i}.{k}": [None, None] for i in range(len(lays)) for k in
           ("d1", "hist", "iface", "p.d1", "p.hist") + sx.ENERGY + tuple("p." + n for n in sx.ENERGY)}
    ranks = []
    try:
        for lay in lays:
            ranks.append(OperatorRank(case["points"], lay, np.arange(n_gs), case["mass"], case["load"], case["lmd"], case["mu"],
                                      case["rho"], case["dt"], case["alpha"], ramp=case["ramp"], stored_geometry=stored, layouts=lays))
        ifaces = [Guarded(3 * n_gs) for _ in ranks]
        for r, g in zip(ranks, ifaces):
            r.stepper.set_interface_buffer(g.view)
            r.iface = g.view
        total = torch.zeros(3 * n_gs, dtype=torch.float64, device=DEV)
        held = []
        for lay in lays:
            slots = torch.as_tensor(np.asarray(lay.shared_slots, dtype=np.int64), device=DEV)
            gd = (3 * slots[:, None] + torch.arange(3, device=DEV)[None, :]).reshape(-1)
            mask = torch.zeros(3 * n_gs, dtype=torch.bool, device=DEV)
            mask[gd] = True
            held.append((gd, mask, torch.as_tensor(np.asarray(lay.loc_dof_shared, dtype=np.int64), device=DEV)))
        nobody = torch.ones(3 * n_gs, dtype=torch.bool, device=DEV)
        for _, mask, _ in held:
            nobody &= ~mask
        for j in range(2):
            local = [(_dev(case["d0"][j][lay.local_dof]), _dev(case["dn"][j][lay.local_dof])) for lay in lays]
            got = {}
            for energy in (True, False):
                for mode in ("synced", "predicted"):
                    recs, hists, tables, rows = [], [], [], []
                    for i, r in enumerate(ranks):
                        r.stepper.set_state(local[i][0], local[i][1], case["tn"])
                        recs.append(Guarded(r.stepper.n_dof))
                        r.stepper.record(1, out=recs[i].view)
                        hists.append(Guarded(r.input_size))
                        tables.append(Guarded(r.input_size, case["tables"][i][j]))
                        rows.append(r.record_energy(1) if energy else r.stepper.record_energy(0))
                    if mode == "synced":
                        for r in ranks:
                            r.iface.zero_()
                            r.stepper.step_begin()
                        sum_interfaces(ranks, total)
                        if garbage is not None:
                            for r in ranks:
                                r.iface[nobody] = garbage
                        for i, r in enumerate(ranks):
                            r.stepper.step_finish(hists[i].view, 0)
                    else:
                        for i, r in enumerate(ranks):
                            r.stepper.step_predicted(1, tables[i].view, 0, hists[i].view, 0)
                    for i, r in enumerate(ranks):
                        d1, newn, tn = r.stepper.state()
                        gd, mask, loc = held[i]
                        assert all(g.intact() for g in (recs[i], hists[i], tables[i], ifaces[i]))
                        assert torch.equal(recs[i].view, d1) and torch.equal(newn, local[i][0])
                        assert tn == case["tn"] + case["dt"]
                        got[(energy, mode, i)] = (d1, hists[i].view.clone())
                        if mode == "synced":
                            assert not bool(r.iface[~mask].any())          # foreign slots: exactly 0 after step_finish
                            assert torch.equal(r.iface[mask], total[mask])
                        else:
                            assert torch.equal(hists[i].view, tables[i].view) and torch.equal(d1[loc], tables[i].view)
                        if not energy:
                            on = got[(True, mode, i)]
                            assert torch.equal(on[0], d1) and torch.equal(on[1], hists[i].view)
                            continue
                        p = f"r{i}." + ("" if mode == "synced" else "p.")
                        out[p + "d1"][j], out[p + "hist"][j] = _host(d1), _host(hists[i].view)
                        if mode == "synced":
                            free = _dev(case["free"][sx._global_shared_dofs(lays[i])])
                            out[f"r{i}.iface"][j] = _host(total[gd] * free)  # (a clamped dof's slot: unmasked sums, unread)
                        row = _host(rows[i][0])
                        for c, name in enumerate(sx.ENERGY):
                            out[p + name][j] = row[c:c + 1]
                    if energy and mode == "synced":                       # a shared dof: the same bits on all its holders
                        seen = torch.full((3 * n_gs,), float("nan"), dtype=torch.float64, device=DEV)
                        for i in range(len(ranks)):
                            gd, _, loc = held[i]
                            d1 = got[(True, "synced", i)][0][loc]
                            first = torch.isnan(seen[gd])
                            assert torch.equal(seen[gd][~first], d1[~first])
                            seen[gd] = d1
    finally:
        for r in ranks:
            r.close()
    return {k: np.array(v) for k, v in out.items()}


def _stored_variants(case):
    return (0, 1) if case["cells"].shape[1] == 10 else (None,)


def _hold(got, ref, env, label):
    _, bad = sx.check(got, ref, env, ox.KERNEL_FACTOR, label)
    assert not bad, bad


@pytest.mark.parametrize("key", sx.whole_case_keys(), ids=sx.key_name)
def test_whole_mesh_step_is_within_the_bar(key):
    case, ref, env = sx.reference(*key)
    for stored in _stored_variants(case):
        got = run_whole(case, stored)
        assert sorted(got) == sorted(ref)
        _hold(got, ref, env, f"{sx.key_name(key)} g{stored}")


def test_the_comparison_sees_a_ramp_read_one_step_late():
    """The first CPU mutant through the GPU: the stepper is given ``tn + dt`` and held to the reference of ``tn``.  It must miss
    the bar where the float64 mutant does, so the comparison above is not one that anything passes."""
    key = (("straight288", "nu", 0.3), "base")
    case, ref, env = sx.reference(*key)
    late = dict(case, tn=case["tn"] + case["dt"])
    _, bad = sx.check(run_whole(late, 1), ref, env, ox.KERNEL_FACTOR, sx.key_name(key) + " late ramp")
    missed = sorted(b[0] for b in bad)
    assert "d1" in missed and "dW" in missed and "mass" not in missed and "Un" not in missed, missed


@pytest.mark.parametrize("key", sx.partition_keys(), ids=sx.key_name)
def test_partition_steps_are_within_the_bar(key):
    case, ref, env = sx.partition_reference(*key)
    for stored in _stored_variants(case):
        got = run_partition(case, stored)
        assert sorted(got) == sorted(k for k in ref if k.startswith("r"))
        label = f"{sx.key_name(key)} g{stored}"
        _hold(got, ref, env, label)
        total = {name: sum(got[f"r{i}.{name}"] for i in range(len(case["layouts"]))) for name in sx.ENERGY}
        _hold(total, ref, env, label + " sum")                        # the shares add up to the whole-mesh row


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("mesh", ox.MESHES)
def test_power_of_two_units_commute_bitwise(mesh, u):
    case = sx.build_partition_case((mesh, "nu", 0.3), "mod3")
    scaled = sx.scaled_case(case, u)
    stored = _stored_variants(case)[-1]
    base = dict(run_whole(case, stored), **run_partition(case, stored))
    got = dict(run_whole(scaled, stored), **run_partition(scaled, stored))
    differ = []
    for name, want in base.items():
        want = want * 2.0 ** (u * sx.unit_exponent(name))               # exact: the CPU test shows nothing near the ends of the range
        assert np.isfinite(got[name]).all(), name
        if not np.array_equal(got[name], want):
            differ.append((name, int((got[name] != want).sum())))
    print(mesh, u, "outputs that differ:", differ)
    assert not differ, differ


@pytest.mark.parametrize("mesh", sx.EDGE_MESHES)
@pytest.mark.parametrize("n_nodes", sx.EDGE_NODES)
def test_node_pass_at_its_launch_edges(mesh, n_nodes):
    case, ref, env = sx.edge_reference(mesh, n_nodes)
    assert len(case["points"]) == (n_nodes or case["cells"].shape[1])
    for stored in _stored_variants(case):
        _hold(run_whole(case, stored), ref, env, f"{mesh}-{n_nodes}nodes g{stored}")


@pytest.mark.parametrize("mesh", sx.EDGE_MESHES)
@pytest.mark.parametrize("n_shared,n_extra", sx.FAKE_SETS)
def test_finish_pass_at_its_launch_edges(mesh, n_shared, n_extra):
    case, ref, env = sx.fake_reference(mesh, n_shared, n_extra)
    assert case["layouts"][0].shared_local.size == n_shared and case["n_gs"] - n_shared == n_extra
    got = run_partition(case, _stored_variants(case)[-1], garbage=3.0)
    _hold(got, ref, env, f"{mesh}-fake{n_shared}+{n_extra}")
