"""The partitioned loop on the operator stepper without a GPU: the library's seven new entry points and their argument
checks, the register budget of the new kernels of csrc/saa_opstep.hip, the layouts ``fem_setup.build_layouts`` makes of the
10-column fixture mesh, and the NumPy double of the partitioned loop (tests/p2_partition_double.py) against the whole-mesh
double (tests/p2_dynamics_double.py).

Bars: the synchronised run of the partition double against the whole-mesh double differs only in the order in which a
shared node's element forces are added (per rank, then over the ranks, instead of one dense row): 1e-12 over 200 steps
(measured 7.0e-15 for two slabs and 7.2e-15 for the three interleaved parts)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import p2_double as p2
import p2_dynamics_double as dyn
import p2_partition_double as pd
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd import fem_setup as fs
from synchronization_avoiding_algorithms_amd.mesh import slab_partition, structured_beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("saa_operator_stepper_set_shared", "saa_operator_stepper_set_interface_buffer", "saa_operator_stepper_step_begin",
               "saa_operator_stepper_step_finish", "saa_operator_stepper_step_predicted", "saa_operator_stepper_halo_gather",
               "saa_operator_stepper_halo_scatter")


def test_library_exports_the_partition_entry_points():
    assert _lib.ABI_VERSION == 16
    lib = _lib.load()
    assert lib.saa_abi_version() == 16
    header = open(_lib.HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    assert _lib.SOURCES[-1] == "saa_api.cpp"


def test_argument_checks_need_no_device():
    lib = _lib.load()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is looked at
    one = (C.c_int32 * 1)(0)
    assert lib.saa_operator_stepper_set_shared(None, 0, None, None, 0) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error()
    assert lib.saa_operator_stepper_set_interface_buffer(None, None) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_step_begin(None) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_step_finish(None, None, 0) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_step_predicted(None, 1, None, 0, None, 0) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_halo_gather(None, None) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_halo_scatter(None, None) == _lib.SAA_E_ARG
    # a handle that is a struct holding a null implementation pointer is a null handle too
    empty = C.c_void_p(0)
    assert lib.saa_operator_stepper_step_begin(C.byref(empty)) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error()


def test_layouts_of_the_fixture_mesh():
    """``build_layouts`` is width-agnostic: the 10-column cells of the 288-tet fixture."""
    g = load_golden("p2_beam.npz")
    c10, pts = g["cells10"], g["points_curved"]
    assert c10.shape == (288, 10) and len(pts) == 625
    dnodes = np.unique(g["dirichlet_dofs"] // 3)
    is_d = np.zeros(625, dtype=bool)
    is_d[dnodes] = True

    lays, gs = fs.build_layouts(c10, slab_partition(structured_beam(2, length=6.0), 2), 2, 625, dnodes)
    assert len(gs) == 25 and [len(l.shared_local) for l in lays] == [25, 25]
    assert len(lays[0].dirichlet_dofs) > 0 and len(lays[1].dirichlet_dofs) == 0
    assert [l.cells_local.shape[1] for l in lays] == [10, 10]

    lays, gs = fs.build_layouts(c10, np.arange(288) % 3, 3, 625, dnodes)
    assert len(gs) == 566 and [len(l.shared_local) for l in lays] == [484, 425, 534]
    mult = np.zeros(625, dtype=int)
    for l in lays:
        mult[l.nodes] += 1
    assert mult.max() == 3 and int(is_d[gs].sum()) == 21
    for l in lays:
        assert np.array_equal(gs[l.shared_slots], l.shared_nodes) and np.array_equal(l.nodes[l.shared_local], l.shared_nodes)
        assert np.array_equal(np.asarray(pts)[l.nodes][l.cells_local], np.asarray(pts)[c10[l.elements]])


@pytest.fixture(scope="module")
def curved():
    g = load_golden("p2_beam.npz")
    lmd, mu, rho, fz = (float(g[k]) for k in ("lmd", "mu", "rho", "fz"))
    pts, c10, dd = g["points_curved"], g["cells10"], g["dirichlet_dofs"]
    K, _ = p2.assemble(pts, c10, dd, lmd, mu, rho)
    mass = dyn.hrz_mass(pts, c10, rho)
    load = p2.load(pts, c10, dd, (0.0, -fz, -fz))
    dt = 0.9 * 2.0 / dyn.omega_extremes(K, mass, dd)[1]
    return dict(pts=pts, c10=c10, dd=dd, dnodes=np.unique(dd // 3), mat=(lmd, mu, rho), K=K, mass=mass, load=load, dt=dt)


@pytest.mark.parametrize("name", ("slab2", "mod3"))
def test_synchronised_double_reproduces_the_whole_mesh_double(curved, name):
    c = curved
    epart, P = (slab_partition(structured_beam(2, length=6.0), 2), 2) if name == "slab2" else (np.arange(288) % 3, 3)
    want = dyn.run(c["K"], c["mass"], c["load"], c["dd"], c["dt"], 0.5, True, 200)
    part = pd.PartitionDouble.from_epart(c["pts"], c["c10"], c["dnodes"], epart, P, c["mass"], c["load"], *c["mat"], c["dt"], 0.5)
    hists = [np.zeros((200, len(r.loc))) for r in part.ranks]
    part.step_synced(200, hists)
    e0, en = rel_l2(part.gather("d0"), want[0]), rel_l2(part.gather("dn"), want[1])
    print(name, "partition double against the whole-mesh double, 200 steps: d0", e0, "dn", en)
    assert e0 < 1e-12 and en < 1e-12 and abs(part.tn - want[2]) <= 1e-14 * want[2]
    for i, r in enumerate(part.ranks):                               # every holder's copy is the owner's; histories record d1
        assert np.array_equal(r.d0, part.gather("d0")[r.dof])
        assert np.array_equal(hists[i][-1], r.d0[r.loc]) and np.array_equal(hists[i][-2], r.dn[r.loc])
        assert not r.d0[r.dd].any()


def test_predicted_double_overwrites_and_records(curved):
    c = curved
    part = pd.PartitionDouble.from_epart(c["pts"], c["c10"], c["dnodes"], np.arange(288) % 3, 3, c["mass"], c["load"], *c["mat"],
                                         c["dt"], 0.5)
    part.step_synced(5)
    rng = np.random.default_rng(5)
    tables = [rng.uniform(-1e-4, 1e-4, size=(4, len(r.loc))) for r in part.ranks]
    hists = [np.full((6, len(r.loc)), -7.0) for r in part.ranks]
    part.step_predicted(3, tables, 1, hists, 2)
    for i, r in enumerate(part.ranks):
        assert np.array_equal(r.d0[r.loc], tables[i][3]) and np.array_equal(hists[i][2:5], tables[i][1:4])
        assert (hists[i][:2] == -7.0).all() and (hists[i][5] == -7.0).all()
        clamped = np.intersect1d(r.loc, r.dd)
        assert len(clamped) > 0 and r.d0[clamped].all()              # a clamped shared dof takes the table value


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_partition_kernels_use_no_scratch_and_reach_occupancy_eight():
    """The node pass of a partition is the node pass plus a slot lookup and a table read (the existing one holds 30 vector
    registers): it, the finish kernel and the halo kernels must stay at 64 registers or fewer, eight waves per SIMD."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opstep.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
    print(out.stdout)
    for name, r in rows.items():
        assert r["vspill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
    for kernel, count in (("opstep_node_kernel<1, false>", 1), ("opstep_node_kernel<2, false>", 1), ("opstep_node_kernel<1, true>", 1),
                          ("opstep_node_kernel<2, true>", 1), ("opstep_finish_kernel", 2), ("opstep_halo_kernel", 2)):
        hit = [r for name, r in rows.items() if kernel in name]
        assert len(hit) == count, (kernel, rows)
        for r in hit:
            assert r["vgpr"] <= 64 and r["occ"] == 8, (kernel, r)
    for name in rows:                                                # the pins of tests/test_p2_dynamics.py stay unambiguous
        if "opstep_finish" in name or "opstep_halo" in name:
            assert "opstep_node_kernel" not in name and "opstep_elem_p2_kernel" not in name
