"""The partitioned loop on the operator stepper on the GPU: ``saa_operator_stepper_set_shared`` / ``_step_begin`` /
``_step_finish`` / ``_step_predicted`` / ``_halo_gather`` / ``_halo_scatter``, ``dynamics.OperatorRank``,
``dynamics.OperatorPartition`` and ``drivers dynamics --parts`` against the whole-mesh stepper (itself pinned to the dense
double by tests/test_gpu_p2_dynamics.py), the NumPy double of the partitioned loop (tests/p2_partition_double.py) and, for
order 1, the production step kernel.

Shapes: 25 shared nodes of the two slabs sit inside one block of the finish launch; the 484 / 425 / 534 shared nodes of
``epart = arange(288) % 3`` cross its 256-lane block edge, and that split has foreign slots, triple-held nodes and clamped
shared nodes; 625 nodes / 288 elements run partial last blocks in both passes.

Bars: rel-L2 < 1e-11 on states after a few hundred steps, the project's short-run bar - the partition differs from the whole
mesh only in the order of a few additions; 1e-13 for the fake shared set on the whole mesh, where even that order is the
same; bitwise wherever a value is only copied."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden, rel_l2

import p2_double as p2
import p2_dynamics_double as dyn
import p2_partition_double as pd

pytestmark = pytest.mark.gpu

E, NU, RHO, FZ = 1e6, 0.3, 1.0, 0.5
PARTITIONS = ("slab2", "mod3")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


class Case:
    """A clamped order-2 beam with its dense double: K, HRZ mass, load, dt = 0.9 dt_crit."""

    def __init__(self, points, cells10, dirichlet, lmd, mu, rho, fz):
        self.pts, self.c10, self.dd = points, cells10, np.asarray(dirichlet, dtype=np.int64)
        self.dnodes = np.unique(self.dd // 3)
        self.lmd, self.mu, self.rho, self.fz = lmd, mu, rho, fz
        self.K, _ = p2.assemble(points, cells10, self.dd, lmd, mu, rho)
        self.mass = dyn.hrz_mass(points, cells10, rho)
        self.load = p2.load(points, cells10, self.dd, (0.0, -fz, -fz))
        self.dt = 0.9 * 2.0 / dyn.omega_extremes(self.K, self.mass, self.dd)[1]

    def op(self):
        from synchronization_avoiding_algorithms_amd.modal import ModalOperator

        return ModalOperator(self.pts, self.c10, self.dd, self.lmd, self.mu, self.rho)

    def epart(self, name):
        from synchronization_avoiding_algorithms_amd.mesh import slab_partition, structured_beam

        assert len(self.c10) == 288
        return (slab_partition(structured_beam(2, length=6.0), 2), 2) if name == "slab2" else (np.arange(288) % 3, 3)

    def partition(self, name, stored=None):
        from synchronization_avoiding_algorithms_amd.dynamics import OperatorPartition

        epart, P = self.epart(name)
        return OperatorPartition(self.pts, self.c10, self.dnodes, epart, P, rho=self.rho, fz=self.fz, alpha=0.5, dt=self.dt,
                                 stored_geometry=stored, lame=(self.lmd, self.mu))

    def double(self, name):
        epart, P = self.epart(name)
        return pd.PartitionDouble.from_epart(self.pts, self.c10, self.dnodes, epart, P, self.mass, self.load, self.lmd, self.mu,
                                             self.rho, self.dt, 0.5)


@pytest.fixture(scope="module")
def curved288():
    g = load_golden("p2_beam.npz")
    lmd, mu, rho, fz = (float(g[k]) for k in ("lmd", "mu", "rho", "fz"))
    assert g["cells10"].shape == (288, 10) and len(g["points_curved"]) == 625
    return Case(g["points_curved"], g["cells10"], g["dirichlet_dofs"], lmd, mu, rho, fz)


@pytest.fixture(scope="module")
def beam36():
    """to_quadratic(structured_beam(1, length=6.0)) with every mid-edge node moved by a seeded +-0.025."""
    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

    quad = to_quadratic(structured_beam(1, length=6.0))
    nv = len(structured_beam(1, length=6.0).points)
    pts = quad.points.copy()
    pts[nv:] += np.random.default_rng(11).uniform(-0.025, 0.025, size=(len(pts) - nv, 3))
    assert quad.tets10.shape == (36, 10) and len(pts) == 117
    return Case(pts, quad.tets10, node_to_dof(plane_nodes(quad.points)), *lame(E, NU), RHO, FZ)


@pytest.fixture(scope="module")
def whole200(curved288):
    """(d0, dn, tn) of the whole-mesh stepper after 200 steps, per ``stored_geometry``: computed once."""
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    c, out = curved288, {}
    with c.op() as op:
        mass, load = op.lumped_mass(), op.load((0.0, -c.fz, -c.fz))
        for stored in (0, 1):
            with OperatorStepper(op, mass, load, c.dt, 0.5) as st:
                st.set_option("stored_geometry", stored)
                st.step(200)
                out[stored] = st.state()
    want = dyn.run(c.K, c.mass, c.load, c.dd, c.dt, 0.5, True, 200)
    assert rel_l2(out[0][0].cpu().numpy(), want[0]) < 1e-11
    return out


def _fake_layout(c, n_extra=4, seed=2):
    """The whole mesh as one rank in which every third node is declared shared; ``n_extra`` slots of Global_shared are held
    by nobody.  Returns (RankLayout, global_shared stand-in)."""
    from synchronization_avoiding_algorithms_amd.fem_setup import RankLayout, node_to_dof

    n = len(c.pts)
    shared = np.arange(0, n, 3)
    rng = np.random.default_rng(seed)
    shared = shared[rng.permutation(len(shared))]                     # table order is not node order
    slots = np.sort(rng.permutation(len(shared) + n_extra)[:len(shared)])
    lay = RankLayout(rank=0, elements=np.arange(len(c.c10)), nodes=np.arange(n), cells_local=np.asarray(c.c10, dtype=np.int32),
                     shared_nodes=shared, shared_local=shared.astype(np.int32), shared_slots=slots.astype(np.int32),
                     dirichlet_dofs=c.dd.astype(np.int32), loc_dof_shared=node_to_dof(shared))
    return lay, np.arange(len(shared) + n_extra)


# ---- 1. synchronised steps, order 2 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("stored", (0, 1))
@pytest.mark.parametrize("name", PARTITIONS)
def test_synchronised_partition_matches_the_whole_mesh(curved288, whole200, name, stored):
    import torch

    c = curved288
    w0, wn, wt = whole200[stored]
    with c.partition(name, stored) as part:
        part.step_synced(200)
        d0, dn = part.gather("d0"), part.gather("dn")
        e0, en = rel_l2(d0.cpu().numpy(), w0.cpu().numpy()), rel_l2(dn.cpu().numpy(), wn.cpu().numpy())
        print(name, f"stored_geometry={stored}: 200 synchronised steps against the whole mesh: d0", e0, "dn", en, "tn", part.tn, wt)
        assert e0 < 1e-11 and en < 1e-11
        assert part.tn == wt
        for r in part.ranks:                                         # every holder's copy of a node is the owner's, bit for bit
            s0, sn, tn = r.get_state()
            assert torch.equal(s0, d0[r.global_dof]) and torch.equal(sn, dn[r.global_dof]) and tn == wt
            dd = np.asarray(r.layout.dirichlet_dofs, dtype=np.int64)
            assert not s0.cpu().numpy()[dd].any() and not sn.cpu().numpy()[dd].any()
        assert not d0.cpu().numpy()[c.dd].any() and float(d0.abs().max()) > 0


# ---- 2. a fake shared set on the whole mesh -------------------------------------------------------------------------------

def test_fake_shared_set_on_the_whole_mesh_is_the_plain_step(beam36):
    import torch

    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    c = beam36
    lay, gs = _fake_layout(c)
    slots = torch.as_tensor(lay.shared_slots.astype(np.int64), device="cuda")
    gd = (3 * slots[:, None] + torch.arange(3, device="cuda")[None, :]).reshape(-1)
    loc = torch.as_tensor(np.asarray(lay.loc_dof_shared, dtype=np.int64), device="cuda")
    foreign = torch.ones(3 * len(gs), dtype=torch.bool, device="cuda")
    foreign[gd] = False
    assert int(foreign.sum()) == 12
    with c.op() as op:
        mass, load = op.lumped_mass(), op.load((0.0, -c.fz, -c.fz))
        with OperatorStepper(op, mass, load, c.dt, 0.5) as ref:
            ref.step(50)
            w0, wn, wt = ref.state()
        with OperatorStepper(op, mass, load, c.dt, 0.5) as st:
            st.set_shared(lay.shared_local, lay.shared_slots, len(gs))
            iface = torch.zeros(3 * len(gs), dtype=torch.float64, device="cuda")
            st.set_interface_buffer(iface)
            worst = 0.0
            for k in range(50):
                kd0 = op.apply(st.state()[0])[0]                    # K d0 of the masked operator: the node sums on free dofs
                st.step_begin()
                iface[foreign] = 3.0                                  # what a reduction leaves in slots of other ranks' nodes
                st.step_finish()
                assert not iface[foreign].any()
                free = op.free[loc] != 0
                got, want = iface[gd][free], kd0[loc][free]
                if float(want.abs().max()) > 0:
                    worst = max(worst, float((got - want).norm() / want.norm()))
            d0, dn, tn = st.state()
    e0, en = rel_l2(d0.cpu().numpy(), w0.cpu().numpy()), rel_l2(dn.cpu().numpy(), wn.cpu().numpy())
    print("begin + finish against step, 50 steps: d0", e0, "dn", en, "bit-equal:", torch.equal(d0, w0) and torch.equal(dn, wn),
          "iface against K d0, worst rel-L2", worst)
    assert e0 < 1e-13 and en < 1e-13 and tn == wt
    assert worst < 1e-13


# ---- 3. order 1 against the production path ---------------------------------------------------------------------------------

def test_order_one_against_the_production_step_kernel():
    import torch

    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorRank
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes, slab_partition, structured_beam
    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver

    mesh = structured_beam(2)
    lmd, mu = fs.lame(E, NU)
    lumped, fpre, min_edge = fs.device_setup_fields(mesh.points, mesh.tets, RHO, FZ, 0)
    dnodes = clamp_nodes(mesh)
    dt = fs.dt_from_min_edge(min_edge, E, NU, RHO, 0.9)
    lays, gs = fs.build_layouts(mesh.tets, slab_partition(mesh, 2), 2, len(mesh.points), dnodes)
    n_sync, n_pred = 100, 20
    stream = torch.cuda.current_stream().cuda_stream

    shared_tables = []                                               # made by the first run from its history, used by both

    def run(make, begin, finish, predicted, state):
        ranks = [make(lay) for lay in lays]
        hists = [torch.zeros((n_sync + n_pred, 3 * len(lay.shared_local)), dtype=torch.float64, device="cuda") for lay in lays]
        total = torch.zeros(3 * len(gs), dtype=torch.float64, device="cuda")
        for k in range(n_sync):
            for r in ranks:
                begin(r)
            total.copy_(ranks[0].iface)
            total += ranks[1].iface
            for r in ranks:
                r.iface.copy_(total)
            for r, h in zip(ranks, hists):
                finish(r, h, k)
        if not shared_tables:
            amp = max(float(h[n_sync - 1].abs().max()) for h in hists)
            rng = np.random.default_rng(7)
            shared_tables.extend(_dev(amp * rng.uniform(-1.0, 1.0, size=(n_pred, h.shape[1]))) for h in hists)
        tables = shared_tables
        for r, t, h in zip(ranks, tables, hists):
            predicted(r, n_pred, t, 0, h, n_sync)
        out = [(state(r), h.cpu().numpy(), t.cpu().numpy()) for r, h, t in zip(ranks, hists, tables)]
        for r in ranks:
            r.close()
        return out

    def make_production(lay):
        dof = lay.local_dof
        s = HipExplicitSolver(mesh.points[lay.nodes], lay.cells_local, lumped[dof], fpre[dof], lay.dirichlet_dofs, lmd, mu, dt, 0.5,
                              shared_local=lay.shared_local, shared_slots=lay.shared_slots, n_global_shared=len(gs), device=0)
        s.iface = torch.zeros(3 * len(gs), dtype=torch.float64, device="cuda")
        s.set_interface_buffer(s.iface)
        s.set_stream(stream)
        return s

    def production_state(s):
        d0, dn, tn = s.get_state()
        return d0.ravel(), dn.ravel(), tn

    want = run(make_production, lambda s: s.step_begin(), lambda s, h, k: s.step_finish(h, k),
               lambda s, n, t, t0, h, h0: s.step_predicted(n, t, t0, h, h0), production_state)

    def operator_state(r):
        d0, dn, tn = r.get_state()
        return d0.cpu().numpy(), dn.cpu().numpy(), tn

    got = run(lambda lay: OperatorRank(mesh.points, lay, gs, lumped, fpre, lmd, mu, RHO, dt, 0.5),
              lambda r: r.stepper.step_begin(), lambda r, h, k: r.stepper.step_finish(h, k),
              lambda r, n, t, t0, h, h0: r.step_predicted(n, t, t0, h, h0), operator_state)
    for i, ((gs_, gh, gt), (ws_, wh, wt)) in enumerate(zip(got, want)):
        e0, en, eh = rel_l2(gs_[0], ws_[0]), rel_l2(gs_[1], ws_[1]), rel_l2(gh[:n_sync], wh[:n_sync])
        print(f"order 1, rank {i}: {n_sync} synchronised + {n_pred} predicted steps against HipExplicitSolver: d0", e0, "dn", en,
              "synchronised history", eh, "tn", gs_[2], ws_[2])
        assert e0 < 1e-11 and en < 1e-11 and eh < 1e-11 and abs(gs_[2] - ws_[2]) <= 1e-14 * ws_[2]
        assert np.array_equal(gt, wt) and np.array_equal(gh[n_sync:], gt) and np.array_equal(wh[n_sync:], wt)
        assert np.abs(gh[:n_sync]).max() > 0


# ---- 4. predicted steps, order 2 ------------------------------------------------------------------------------------------

def test_predicted_steps_against_the_double(curved288):
    import torch

    c = curved288
    double = c.double("mod3")
    double.step_synced(20)
    rng = np.random.default_rng(9)
    amp = max(np.abs(r.d0).max() for r in double.ranks)
    tables = [amp * rng.uniform(-1.0, 1.0, size=(30, len(r.loc))) for r in double.ranks]
    double.step_predicted(30, tables)
    with c.partition("mod3") as part:
        part.step_synced(20)
        dev_tables = [_dev(t) for t in tables]
        widths = [r.input_size for r in part.ranks]
        assert widths == [3 * 484, 3 * 425, 3 * 534]
        # the history: 2 rows that stay as they are, 30 rows to fill, and a guard of one more row
        hists = [torch.full((33 * w,), -7.0, dtype=torch.float64, device="cuda") for w in widths]
        part.step_predicted(10, dev_tables, 0, hists, 2)
        part.step_predicted(20, dev_tables, 10, hists, 12)
        for i, r in enumerate(part.ranks):
            h = hists[i].view(33, widths[i])
            assert torch.equal(h[2:32], dev_tables[i]) and bool((h[:2] == -7.0).all()) and bool((h[32] == -7.0).all())
            d0, dn, tn = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in r.get_state())
            w = double.ranks[i]
            e0, en = rel_l2(d0, w.d0), rel_l2(dn, w.dn)
            print(f"rank {i}: 20 synchronised + 30 predicted steps against the double: d0", e0, "dn", en, "tn", tn, double.tn)
            assert e0 < 1e-11 and en < 1e-11 and abs(tn - double.tn) <= 1e-14 * double.tn
            assert np.array_equal(d0[w.loc], tables[i][29]) and np.array_equal(dn[w.loc], tables[i][28])
            clamped = np.intersect1d(w.loc, w.dd)                    # a clamped shared dof takes the table value
            assert len(clamped) > 0 and d0[clamped].all()
            assert not d0[np.setdiff1d(w.dd, w.loc)].any()           # (a clamped dof that is not shared stays 0)


# ---- 5. history and halo ---------------------------------------------------------------------------------------------------

def test_history_rows_are_the_new_shared_dofs_and_the_halo_round_trips(curved288):
    import torch

    c = curved288
    with c.partition("mod3") as part:
        hists = [torch.zeros((6, r.input_size), dtype=torch.float64, device="cuda") for r in part.ranks]
        part.step_synced(3)
        for k in range(3, 6):
            part.step_synced(1, hists, k)
            for r, h in zip(part.ranks, hists):
                row = torch.full((r.input_size + 1,), -7.0, dtype=torch.float64, device="cuda")
                r.stepper.halo_gather(row)
                assert torch.equal(row[:-1], h[k]) and float(row[-1]) == -7.0 and bool(h[k].any())
                loc = torch.as_tensor(np.asarray(r.layout.loc_dof_shared, dtype=np.int64), device="cuda")
                assert torch.equal(r.get_state()[0][loc], h[k])
        assert not any(bool(h[:3].any()) for h in hists)
        r = part.ranks[1]
        before = r.get_state()
        row = _dev(np.random.default_rng(1).uniform(-1.0, 1.0, size=r.input_size))
        r.stepper.halo_scatter(row)
        back = torch.empty_like(row)
        r.stepper.halo_gather(back)
        after = r.get_state()
        loc = torch.as_tensor(np.asarray(r.layout.loc_dof_shared, dtype=np.int64), device="cuda")
        other = torch.ones(r.stepper.n_dof, dtype=torch.bool, device="cuda")
        other[loc] = False
        assert torch.equal(back, row) and torch.equal(after[0][loc], row)
        assert torch.equal(after[0][other], before[0][other]) and torch.equal(after[1], before[1])


# ---- 6. recorder across begin / finish ---------------------------------------------------------------------------------------

def test_recorder_columns_of_a_partitioned_run(curved288):
    import torch

    c = curved288
    with c.partition("mod3") as part:
        states = {}
        done = 0
        for upto in (1, 4, 7, 10):
            part.step_synced(upto - done)
            done = upto
            states[upto - 1] = [r.get_state()[0] for r in part.ranks]
    with c.partition("mod3") as part:
        guards = [torch.full((r.stepper.n_dof * 4 + 5,), -7.0, dtype=torch.float64, device="cuda") for r in part.ranks]
        trajs = [r.stepper.record(4, save_every=3, out=g) for r, g in zip(part.ranks, guards)]
        part.step_synced(10)
        for i, r in enumerate(part.ranks):
            for col, step in enumerate((0, 3, 6, 9)):
                assert torch.equal(trajs[i][:, col], states[step][i]), (i, col)
            assert bool((guards[i][-5:] == -7.0).all())
            loc = np.asarray(r.layout.loc_dof_shared, dtype=np.int64)
            assert bool(trajs[i][:, 3][torch.as_tensor(loc, device="cuda")].any())      # shared rows are recorded by finish


# ---- 7. launch splits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stored", (0, 1))
def test_launch_splits_are_bitwise_equal(curved288, stored):
    import torch

    c = curved288

    def run(chunks):
        with c.partition("mod3", stored) as part:
            for n in chunks:
                part.step_synced(n)
            return [r.get_state() for r in part.ranks]

    ref = run([7])
    for chunks in ([3, 4], [1] * 7):
        got = run(chunks)
        for a, b in zip(got, ref):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2], chunks


# ---- 8. state machine ------------------------------------------------------------------------------------------------------

def test_state_machine_and_argument_checks(beam36):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper

    c = beam36
    lay, gs = _fake_layout(c)
    lib = _lib.load()

    def refused(code, text, fn, *args):
        with pytest.raises(_lib.SaaError, match=text) as ei:
            fn(*args)
        assert ei.value.code == code, (ei.value.code, text)

    with c.op() as op:
        mass, load = op.lumped_mass(), op.load((0.0, -c.fz, -c.fz))
        with OperatorStepper(op, mass, load, c.dt, 0.5) as st:
            refused(_lib.SAA_E_STATE, "no step in flight", st.step_finish)
            n = len(c.pts)
            refused(_lib.SAA_E_ARG, "out of range", st.set_shared, [0, n], [0, 1], 2)
            refused(_lib.SAA_E_ARG, "out of range", st.set_shared, [0, -1], [0, 1], 2)
            refused(_lib.SAA_E_ARG, "out of range", st.set_shared, [0, 1], [0, 2], 2)
            refused(_lib.SAA_E_ARG, "repeated", st.set_shared, [5, 5], [0, 1], 2)
            refused(_lib.SAA_E_ARG, "repeated", st.set_shared, [5, 6], [1, 1], 2)
            refused(_lib.SAA_E_ARG, "n_shared <= n_global_shared", st.set_shared, [5, 6], [0, 1], 1)
            assert st.n_shared == 0
            st.step_begin()                                          # no shared set: begin + finish is a plain step
            st.step_finish()
            st.set_shared(lay.shared_local, lay.shared_slots, len(gs))
            refused(_lib.SAA_E_STATE, "no interface buffer", st.step_begin)
            iface = torch.zeros(3 * len(gs), dtype=torch.float64, device="cuda")
            with pytest.raises(ValueError):
                st.set_interface_buffer(iface[:-3])
            st.set_interface_buffer(iface)
            table = torch.zeros((2, 3 * st.n_shared), dtype=torch.float64, device="cuda")
            assert lib.saa_operator_stepper_step_predicted(st._h, 1, None, 0, None, 0) == _lib.SAA_E_ARG
            assert b"null table" in lib.saa_last_error()
            tp = table.data_ptr()
            for args in ((-1, tp, 0, None, 0), (1, tp, -1, None, 0), (1, tp, 0, tp, -1)):
                assert lib.saa_operator_stepper_step_predicted(st._h, *args) == _lib.SAA_E_ARG, args
            assert lib.saa_operator_stepper_step_finish(st._h, tp, -1) == _lib.SAA_E_ARG
            assert lib.saa_operator_stepper_halo_gather(st._h, None) == _lib.SAA_E_ARG
            assert lib.saa_operator_stepper_halo_scatter(st._h, None) == _lib.SAA_E_ARG
            with pytest.raises(ValueError):
                st.step_predicted(3, table)                          # the table has two rows
            before = st.state()
            st.step_begin()
            for fn, args in ((st.step, (1,)), (st.step_predicted, (1, table)), (st.step_begin, ()), (st.set_state, (None, None, 0.0)),
                             (st.record, (2,)), (st.set_option, ("stored_geometry", 1.0)),
                             (st.set_shared, (lay.shared_local, lay.shared_slots, len(gs))), (st.set_interface_buffer, (iface,)),
                             (st.halo_scatter, (table,))):
                refused(_lib.SAA_E_STATE, "in flight|not finished", fn, *args)
            st.step_finish()
            after = st.state()
            assert after[2] == before[2] + c.dt and torch.equal(after[1], before[0])
            st.step(1)                                               # with a shared set: the local step without overwrite
            st.step_predicted(2, table)
            st.set_shared([], [], 0)                                 # cleared: no buffer needed any more
            st.set_interface_buffer(None)
            st.step_begin()
            st.step_finish()
            assert bool(torch.isfinite(st.state()[0]).all())


# ---- 9. the hybrid schedule --------------------------------------------------------------------------------------------------

N_PAST, N_FUTURE, FILTER = 2, 2, 5


def _persist_torch(i, hist):
    return hist[i - 1].repeat(N_FUTURE * FILTER, 1).contiguous()


def _persist_numpy(i, hist):
    return np.tile(hist[i - 1], (N_FUTURE * FILTER, 1))


def test_run_hybrid_of_the_partition_matches_the_double(curved288):
    c = curved288
    want = c.double("slab2").run_hybrid(40, [_persist_numpy] * 2, N_PAST, N_FUTURE, FILTER)
    with c.partition("slab2") as part:
        got = part.run_hybrid(40, [_persist_torch] * 2, N_PAST, N_FUTURE, FILTER)
        for i, (g, w) in enumerate(zip(got, want)):
            err = rel_l2(g.cpu().numpy(), w)
            print(f"run_hybrid, rank {i}: history of 40 steps (10 synchronised, 3 predicted windows) against the double", err)
            assert g.shape == (40, 75) and err < 1e-11
            assert np.array_equal(g[10:20].cpu().numpy(), np.tile(g[9].cpu().numpy(), (10, 1)))


def test_one_rank_through_distributed_run_hybrid(beam36):
    import torch

    from synchronization_avoiding_algorithms_amd import distributed
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorRank, sum_interfaces

    c = beam36
    lay, gs = _fake_layout(c, n_extra=0)
    double = pd.PartitionDouble(c.pts, [lay], gs, c.mass, c.load, c.lmd, c.mu, c.rho, c.dt, 0.5)
    want = double.run_hybrid(40, [_persist_numpy], N_PAST, N_FUTURE, FILTER)[0]
    total = torch.zeros(3 * len(gs), dtype=torch.float64, device="cuda")
    ranks = []
    with OperatorRank(c.pts, lay, gs, c.mass, c.load, c.lmd, c.mu, c.rho, c.dt, 0.5,
                      reduce=lambda iface: sum_interfaces(ranks, total)) as rank:
        ranks.append(rank)
        hist = distributed.run_hybrid(rank, 40, _persist_torch, N_PAST, N_FUTURE, FILTER)
        d0 = rank.get_state()[0].cpu().numpy()
    err, e0 = rel_l2(hist.cpu().numpy(), want), rel_l2(d0, double.ranks[0].d0)
    print("one OperatorRank through distributed.run_hybrid, 40 steps against the double: history", err, "d0", e0)
    assert hist.shape == (40, rank.input_size) and err < 1e-11 and e0 < 1e-11 and rank.steps_done == 40


# ---- 10. driver --------------------------------------------------------------------------------------------------------------

def test_driver_dynamics_with_parts(tmp_path):
    from synchronization_avoiding_algorithms_amd.results_io import load_displacement

    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    res, data = {}, {}
    for key, extra in (("whole", []), ("parts", ["--parts", "2"])):
        out_dir = tmp_path / key
        out_dir.mkdir()
        out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "dynamics", "--synthetic", "1",
                              "--order", "2", "--steps", "50", "--out", str(out_dir), *extra], cwd=str(out_dir), capture_output=True,
                             text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        res[key] = json.loads(out.stdout.strip().splitlines()[-1])
        data[key] = load_displacement(str(out_dir / "Results" / "Dynamics" / "Displacement_order2.hdf5"))
    print(res["parts"])
    err = rel_l2(data["parts"], data["whole"])
    print("drivers dynamics --parts 2 against the whole mesh, 50 saved columns: rel-L2", err)
    assert data["parts"].shape == data["whole"].shape == (3 * res["whole"]["n_nodes"], 50) and err < 1e-11
    assert res["parts"]["parts"] == 2 and res["parts"]["n_global_shared"] > 0
    assert len(res["parts"]["shared_per_rank"]) == 2 and "parts" not in res["whole"]
    for k in ("order", "n_nodes", "n_elems", "n_free_dofs", "dt", "steps"):
        assert res["parts"][k] == res["whole"][k], k
    assert res["parts"]["tn"] == pytest.approx(res["whole"]["tn"]) and res["parts"]["max_abs_d"] == pytest.approx(res["whole"]["max_abs_d"])
