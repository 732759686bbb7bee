"""The energy balance of the operator stepper without a GPU: the new entry point and its argument checks, the discrete
identity in the NumPy double (tests/energy_double.py), what a step above the stability limit looks like in it, and the
register budget of the energy instantiations of csrc/saa_opstep.hip next to the rows of the kernels they share it with.

Bars.  The identity ``B_n = B_0`` is exact for the exact update.  A step rounds ``d1`` by ``eps |d0|``, which perturbs the
increment ``d1 - d0`` the energies are made of by the relative ``eps |d0| / |d1 - d0|``; from rest ``d0`` is the sum of at
most ``nsteps`` increments, so this is of the order ``eps nsteps``, and at most ``nsteps`` steps add up: ``r0 <= eps
nsteps^2`` = 2.0e-11 for 300 steps.  Measured on the 36-tet beam, ``r0 = max |B_n - B_0| / max(W, T + U)``:
order 2 5.7e-13 (alpha 0.5, ramp) and 3.5e-13 (alpha 0, no ramp); order 1 6.0e-14 and 4.2e-14."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import energy_double as ed
import p2_dynamics_double as dyn
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NU, RHO, FZ = 1e6, 0.3, 1.0, 0.5
EPS = np.finfo(np.float64).eps
OMEGA_MAX_36 = 8893.974037          # the dense omega_max of the 36-tet order-2 beam that tests/test_p2_dynamics.py pins

# tools/kernel_resources.py --file=saa_opstep.hip: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy.  The rows of the kernels
# that the energy balance never touched, as they were before it existed:
PARENT_ROWS = {
    "saa::opstep_geometry_kernel": (30, 108, 0, 0, 0, 4),
    "saa::opstep_elem_p2_kernel": (36, 148, 0, 0, 0, 3),
    "saa::opstep_hrz_mass_kernel": (32, 124, 0, 0, 0, 4),
    "saa::opstep_p1_mass_kernel": (18, 34, 0, 0, 0, 8),
    "saa::opstep_mass_node_kernel": (14, 12, 0, 0, 0, 8),
    "saa::opstep_mass_check_kernel": (18, 6, 0, 0, 0, 8),
    "void saa::opstep_halo_kernel<true>": (15, 9, 0, 0, 0, 8),
    "void saa::opstep_halo_kernel<false>": (14, 11, 0, 0, 0, 8),
}
# The node pass <MODE, ENERGY>, the finish pass <ENERGY> and the final kernel of the balance, as hipcc gives them.
MERGED_ROWS = {
    "void saa::opstep_node_kernel<0, false>": (32, 30, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<1, false>": (38, 30, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<2, false>": (38, 30, 0, 0, 0, 8),
    "void saa::opstep_finish_kernel<false>": (20, 22, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<0, true>": (32, 54, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<1, true>": (44, 54, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<2, true>": (44, 58, 0, 0, 0, 8),
    "void saa::opstep_finish_kernel<true>": (30, 32, 0, 0, 0, 8),
    "saa::opstep_energy_final_kernel": (19, 26, 0, 0, 0, 8),
}
# An energy-off instantiation against the kernel it replaced (opstep_node_update_kernel, opstep_shared_node_kernel<false>,
# <true>, opstep_shared_finish_kernel, before the balance was merged into them): the same row, sgpr at most that kernel's.
REPLACED_ROWS = {
    "void saa::opstep_node_kernel<0, false>": (32, 30, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<1, false>": (38, 30, 0, 0, 0, 8),
    "void saa::opstep_node_kernel<2, false>": (42, 30, 0, 0, 0, 8),
    "void saa::opstep_finish_kernel<false>": (20, 22, 0, 0, 0, 8),
}
# the energy-on node passes: (vgpr, occupancy)
NODE_PASSES = {"void saa::opstep_node_kernel<0, true>": (54, 8), "void saa::opstep_node_kernel<1, true>": (54, 8),
               "void saa::opstep_node_kernel<2, true>": (58, 8)}


def test_library_exports_the_energy_entry_point():
    name = "saa_operator_stepper_set_energy"
    lib = _lib.load()
    header = open(_lib.HEADER).read()
    assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert _lib.SIGNATURES[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p])
    decl = header[header.index("int " + name + "("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int saa_operator_stepper_set_energy(saa_operator_stepper *st, double *energy_dev, int64_t n_rows, "
                    "int32_t every, int64_t next_step_index, const uint8_t *shared_owned_host)")
    assert "saa_openergy.hip" not in _lib.SOURCES and _lib.SOURCES.index("saa_opstep.hip") < _lib.SOURCES.index("saa_api.cpp") == len(_lib.SOURCES) - 1
    from synchronization_avoiding_algorithms_amd import dynamics, drivers, results_io

    assert hasattr(dynamics.OperatorStepper, "record_energy") and hasattr(dynamics.OperatorRank, "record_energy")
    assert hasattr(dynamics.OperatorPartition, "record_energy") and hasattr(dynamics.OperatorPartition, "energy")
    assert drivers.PATHS["energy"].format(p=2) == "Results/Dynamics/Energy_order2.hdf5"
    assert results_io.DATASET == "Displacement" and results_io.ENERGY_DATASET != results_io.DATASET


def test_argument_checks_need_no_device():
    lib = _lib.load()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is looked at
    assert lib.saa_operator_stepper_set_energy(fake, fake, -1, 1, 0, None) == _lib.SAA_E_ARG
    assert b"n_rows < 0" in lib.saa_last_error()
    for every in (0, -3):
        assert lib.saa_operator_stepper_set_energy(fake, fake, 4, every, 0, None) == _lib.SAA_E_ARG
        assert b"every < 1" in lib.saa_last_error()
    assert lib.saa_operator_stepper_set_energy(fake, fake, 4, 1, -1, None) == _lib.SAA_E_ARG
    assert b"next_step_index < 0" in lib.saa_last_error()
    assert lib.saa_operator_stepper_set_energy(None, fake, 4, 1, 0, None) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error()
    empty = C.c_void_p(0)           # a handle that holds a null implementation pointer is a null handle too
    assert lib.saa_operator_stepper_set_energy(C.byref(empty), None, 0, 1, 0, None) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error()


def test_energy_balance_and_ownership_are_pure_functions():
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import energy_balance, energy_report, shared_ownership

    rows = np.array([[1.0, 2.0, 9.0, 0.5, 0.25], [2.0, 2.5, 9.0, 2.0, 0.5], [0.0, 1.0, 9.0, 0.0, 3.0]])
    assert np.array_equal(energy_balance(rows), np.array([0.0, 0.25, 1.25]))
    assert np.array_equal(energy_balance(rows), ed.balance(rows)) and len(energy_balance(rows[:0])) == 0
    rep = energy_report(rows)
    assert rep == {"rows": 3, "T": 0.0, "U": 1.0, "W": 0.0, "D": 3.0, "max_abs_balance": 1.25, "scale": 4.5}
    quad = to_quadratic(structured_beam(2, length=6.0))
    lays, gs = fs.build_layouts(quad.tets10, np.arange(288) % 3, 3, len(quad.points), plane_nodes(quad.points))
    own = shared_ownership(lays, len(gs))
    count = np.zeros(len(gs), dtype=int)
    for lay, o, want in zip(lays, own, ed.ownership(lays, len(gs))):
        assert o.dtype == bool and len(o) == len(lay.shared_local) and np.array_equal(o, want)
        count[lay.shared_slots[o]] += 1
    assert (count == 1).all() and own[0].all() and not own[2].all()   # every shared node has one owner, the lowest holder


@pytest.fixture(scope="module")
def beams36():
    """The 36-tet beam, order 2 and its order-1 counterpart: the double's problem and dt = 0.9 * 2/omega_max."""
    lin = structured_beam(1, length=6.0)
    quad = to_quadratic(lin)
    assert quad.tets10.shape == (36, 10) and lin.tets.shape == (36, 4)
    lmd, mu = lame(E, NU)
    out = {}
    for order, pts, cells in ((2, quad.points, quad.tets10), (1, lin.points, lin.tets)):
        dd = node_to_dof(plane_nodes(pts))
        p = ed.problem(pts, cells, dd, lmd, mu, RHO, FZ)
        p["dd"] = dd
        p["omega_max"] = dyn.omega_extremes(p["K"], p["mass"], dd)[1]
        out[order] = p
    assert abs(out[2]["omega_max"] / OMEGA_MAX_36 - 1.0) < 1e-9
    return out


@pytest.mark.parametrize("alpha,ramp", ((0.5, True), (0.0, False)))
@pytest.mark.parametrize("order", (2, 1))
def test_the_identity_holds_in_the_double(beams36, order, alpha, ramp):
    """300 steps from rest: ``r0`` is round-off (the module docstring derives the bar and quotes the measured values)."""
    p = beams36[order]
    n = 300
    rows, (d0, _, _) = ed.run_whole(p["K"], p["mass"], p["load"], p["dd"], p["live"], 0.9 * 2.0 / p["omega_max"], alpha, ramp, n)
    r0 = np.abs(ed.balance(rows)).max() / ed.scale(rows)
    print(f"order {order}, alpha {alpha}, ramp {ramp}: r0 = {r0:.3e}, scale {ed.scale(rows):.3e}, last row {rows[-1]}")
    assert np.abs(d0).max() > 0 and ed.scale(rows) > 0
    assert r0 < EPS * n * n
    assert (rows[:, 0] >= 0).all() and (rows[:, 2] >= 0).all() and (np.diff(rows[:, 4]) >= 0).all()
    if alpha == 0.0:
        assert not rows[:, 4].any()
    # the cross form and U_n differ by 1/2 (d1 - d0) . K d0: small against U once the beam moves, never equal
    assert np.abs(rows[-1, 1] - rows[-1, 2]) < 0.05 * rows[-1, 2] and rows[-1, 1] != rows[-1, 2]


def test_a_step_above_the_limit_shows_in_the_energy_not_in_the_balance(beams36):
    """200 steps at 1.02 dt_crit (order 2, alpha 0.5, ramp).  The balance measures consistency, ``T + U`` stability: the
    cross form ``T + U_{n+1/2}`` is positive definite only below the limit, and above it it runs away - downwards, ``T`` and
    ``U`` growing with opposite signs and five digits of cancellation, the damping loss ``D`` taking the difference -
    while ``B`` stays constant.  Measured: ``|T + U|`` 4.3e-6 at step 50, 9.5e11 at step 100, 4.6e46 at step 200 (the
    stable run's scale is 2.6e-6); ``max |B_n - B_0|`` is 2.0e-15 of the largest column so far (bar: 1e-12, the project's bar
    for sums of a few hundred float64 terms; the state is rounded at its own size here, so nothing is amplified) and
    4.3e-11 of ``max(|W|, |T + U|)``, which is smaller than ``T`` and ``|U|`` by the cancelled digits."""
    p = beams36[2]
    rows, _ = ed.run_whole(p["K"], p["mass"], p["load"], p["dd"], p["live"], 1.02 * 2.0 / OMEGA_MAX_36, 0.5, True, 200)
    assert np.isfinite(rows).all()
    tu = np.abs(rows[:, 0] + rows[:, 1])
    largest = np.maximum.accumulate(np.abs(rows).max(axis=1))
    b = np.abs(ed.balance(rows))
    print("|T + U| at steps 50, 100, 200:", tu[49], tu[99], tu[199], "max |B_n - B_0| / largest column so far:",
          (b[1:] / largest[1:]).max(), "/ max(|W|, |T + U|):", (b[1:] / np.maximum.accumulate(np.maximum(np.abs(rows[:, 3]), tu))[1:]).max())
    assert tu[199] > 1e40 * tu[49] and (np.diff(tu[99:]) > 0).all()
    assert (b[1:] <= 1e-12 * largest[1:]).all()
    stable, _ = ed.run_whole(p["K"], p["mass"], p["load"], p["dd"], p["live"], 0.9 * 2.0 / OMEGA_MAX_36, 0.5, True, 200)
    assert tu[199] > 1e40 * ed.scale(stable)


def _rows(file):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), f"--file={file}"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    print(out.stdout)
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = tuple(int(v) for v in f[-6:])
    return rows


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_energy_kernels_use_no_scratch_and_the_stepper_kernels_are_the_parents():
    """The energy node passes carry five accumulators and the operands of the update past their last use in it: 54 / 54 / 58
    vector registers against 30 with the balance off, still eight waves per SIMD.  With the balance off the ENERGY = false
    instantiations of the same kernels are launched: they carry none of it, and their rows are those of the separate kernels
    they replaced (sgpr: at most)."""
    rows = _rows("saa_opstep.hip")
    assert len(rows) == len(PARENT_ROWS) + len(MERGED_ROWS) == 17, rows
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, rows[name])
    for name, (vgpr, occ) in NODE_PASSES.items():
        assert rows[name][1] == vgpr and rows[name][5] == occ, (name, rows[name])
    assert rows["void saa::opstep_finish_kernel<true>"][5] == 8 and rows["saa::opstep_energy_final_kernel"][5] == 8
    for name, was in REPLACED_ROWS.items():
        assert rows[name][0] <= was[0] and rows[name][1:] == was[1:], (name, rows[name], was)
    assert rows == {**PARENT_ROWS, **MERGED_ROWS}
