"""Explicit dynamics for quadratic tetrahedra without a GPU: the library's new entry points and their argument checks, the
NumPy double's HRZ mass (tests/p2_dynamics_double.py) against its closed forms, the reason the feature exists (row-sum
lumping gives a negative vertex mass), the sharp stability limits of the two beams against the reference's edge-length
rule, the driver's command list and the register budget of csrc/saa_opstep.hip.

Bars: 1e-14 for the closed-form masses of a straight element (``integral N_a^2`` is ``V/70`` at a vertex and ``8V/105`` on an
edge, so the HRZ masses are ``rho V/36`` and ``4 rho V/27``), 1e-13 for the total mass, 1e-9 for the dense ``omega_max``
(quoted to ten digits)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

import p2_double as p2
import p2_dynamics_double as dyn
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NU, RHO = 1e6, 0.3, 1.0
# dense eigh of M_L^-1/2 K M_L^-1/2, HRZ mass, clamped on x = 0: the 36-tet and the 288-tet elevation of the 6 x 1 x 1 beam
OMEGA_MAX = {1: 8893.974037, 2: 17548.990195}
DT_CRIT = {1: 2.248714e-4, 2: 1.139667e-4}

NEW_SYMBOLS = ("saa_operator_lumped_mass", "saa_operator_stepper_create", "saa_operator_stepper_set_state",
               "saa_operator_stepper_get_state", "saa_operator_stepper_set_recorder", "saa_operator_stepper_set_option",
               "saa_operator_stepper_step", "saa_operator_stepper_destroy")


def test_library_exports_the_stepper_entry_points():
    assert _lib.ABI_VERSION == 16
    assert "saa_opstep.hip" in _lib.SOURCES
    lib = _lib.load()
    assert lib.saa_abi_version() == _lib.ABI_VERSION
    header = open(_lib.HEADER).read()
    assert "16: saa_operator_lumped_mass, saa_operator_stepper_*" in header
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name


def test_argument_checks_need_no_device():
    lib = _lib.load()
    h = C.c_void_p()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is looked at
    assert lib.saa_operator_lumped_mass(None, None) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_create(None, None, None, 1e-4, 0.5, 1, None) == _lib.SAA_E_ARG
    for dt in (0.0, -1e-4, float("nan")):
        assert lib.saa_operator_stepper_create(fake, fake, fake, dt, 0.5, 1, C.byref(h)) == _lib.SAA_E_ARG
        assert b"dt must be" in lib.saa_last_error() and not h.value
    assert lib.saa_operator_stepper_create(fake, fake, fake, 1e-4, -0.5, 1, C.byref(h)) == _lib.SAA_E_ARG
    assert b"alpha must be" in lib.saa_last_error() and not h.value
    assert lib.saa_operator_stepper_create(None, fake, fake, 1e-4, 0.5, 1, C.byref(h)) == _lib.SAA_E_ARG
    assert b"null handle" in lib.saa_last_error() and not h.value
    assert lib.saa_operator_stepper_set_state(None, None, None, 0.0) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_get_state(None, None, None, None) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_set_recorder(None, None, 0, 1, 0) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_set_option(None, b"stored_geometry", 1.0) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_step(None, 1) == _lib.SAA_E_ARG
    assert lib.saa_operator_stepper_destroy(None) == _lib.SAA_OK


def _straight_element():
    verts = np.array([(0.2, 0.1, 0.0), (1.3, 0.0, 0.1), (0.1, 0.9, 0.2), (0.3, 0.2, 1.1)])
    from synchronization_avoiding_algorithms_amd.mesh import TET10_EDGES

    pts = np.concatenate([verts, [0.5 * (verts[a] + verts[b]) for a, b in TET10_EDGES]])
    vol = np.linalg.det(verts[1:] - verts[0]) / 6.0
    return pts, np.arange(10)[None, :], vol


def test_hrz_mass_of_a_straight_element_is_v_36_and_4v_27():
    pts, cell, vol = _straight_element()
    rho = 1.7
    wd, _, N = p2.geometry(pts, cell, 4)
    I = np.einsum("eq,qa->ea", wd, N ** 2)[0]
    assert np.abs(I[:4] / vol - 1.0 / 70.0).max() < 1e-14 and np.abs(I[4:] / vol - 8.0 / 105.0).max() < 1e-14
    m = dyn.hrz_element_masses(pts, cell, rho)[0]
    print("HRZ masses / (rho V)", m / (rho * vol))
    assert np.abs(m[:4] / (rho * vol) - 1.0 / 36.0).max() < 1e-14
    assert np.abs(m[4:] / (rho * vol) - 4.0 / 27.0).max() < 1e-14


def test_row_sum_lumping_gives_a_negative_vertex_mass():
    """The reason the feature exists: ``integral N_vertex = -V/20`` on the quadratic tetrahedron."""
    pts, cell, vol = _straight_element()
    m = dyn.row_sum_element_masses(pts, cell, 1.0)[0]
    assert np.abs(m[:4] / vol + 1.0 / 20.0).max() < 1e-14 and np.abs(m[4:] / vol - 1.0 / 5.0).max() < 1e-14
    assert (m[:4] < 0).all() and (dyn.hrz_element_masses(pts, cell, 1.0) > 0).all()


def test_hrz_mass_is_positive_on_curved_elements_and_sums_to_the_total():
    g = load_golden("p2_beam.npz")
    rho = 1.3
    for name in ("straight", "curved"):
        pts, c10 = g[f"points_{name}"], g["cells10"]
        me = dyn.hrz_element_masses(pts, c10, rho)
        m = dyn.hrz_mass(pts, c10, rho)
        volume = p2.geometry(pts, c10, 4)[0].sum()
        print(name, "smallest element mass", me.min(), "total / (rho volume) - 1", m[0::3].sum() / (rho * volume) - 1.0)
        assert (me > 0).all() and (m > 0).all()
        assert abs(m[0::3].sum() - rho * volume) < 1e-13 * rho * volume
        assert np.array_equal(m[0::3], m[1::3]) and np.array_equal(m[0::3], m[2::3])
    quad = to_quadratic(structured_beam(1, length=6.0))
    assert abs(dyn.hrz_mass(quad.points, quad.tets10, rho)[0::3].sum() - rho * 6.0) < 1e-13 * rho * 6.0


@pytest.mark.parametrize("n", (1, 2))
def test_dense_stability_limit_and_the_reference_rule(n):
    from synchronization_avoiding_algorithms_amd.dynamics import reference_rule_dt

    quad = to_quadratic(structured_beam(n, length=6.0))
    assert quad.tets10.shape == ((36, 288)[n - 1], 10) and len(quad.points) == (117, 625)[n - 1]
    lmd, mu = lame(E, NU)
    dd = node_to_dof(plane_nodes(quad.points))
    K, _ = p2.assemble(quad.points, quad.tets10, dd, lmd, mu, RHO)
    _, omega_max = dyn.omega_extremes(K, dyn.hrz_mass(quad.points, quad.tets10, RHO), dd)
    rule = reference_rule_dt(quad.points, quad.tets10, E, NU, RHO, 0.9)
    print("omega_max", omega_max, "dt_crit", 2.0 / omega_max, "reference rule", rule, "ratio", rule * omega_max / 2.0)
    assert abs(omega_max / OMEGA_MAX[n] - 1.0) < 1e-9
    assert abs(2.0 / omega_max / DT_CRIT[n] - 1.0) < 1e-6           # (quoted to seven digits)
    assert rule > 2.0 / omega_max
    if n == 1:
        assert abs(rule / 3.505e-4 - 1.0) < 1e-3 and abs(rule * omega_max / 2.0 - 1.56) < 0.01


def test_driver_help_lists_dynamics():
    out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "--help"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dynamics" in out.stdout
    from synchronization_avoiding_algorithms_amd import drivers

    assert drivers.PATHS["dynamics"].format(p=2) == "Results/Dynamics/Displacement_order2.hdf5"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_stepper_kernels_use_no_scratch_and_spill_no_vector_register():
    """One lane per element or node: an array pushed into scratch memory would keep every parity test green and cost a
    multiple of the step time.  The stored-geometry element pass holds 36 + 4 geometry values and the 36 gradients of
    p2_apply_k_kernel without its thirty coordinates: it must fit three waves per SIMD (170 registers per lane)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opstep.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
    print(out.stdout)
    for kernel in ("opstep_geometry_kernel", "opstep_elem_p2_kernel", "opstep_hrz_mass_kernel", "opstep_p1_mass_kernel",
                   "opstep_mass_node_kernel", "opstep_mass_check_kernel", "opstep_node_kernel<0, false>"):
        assert any(kernel in k for k in rows), (kernel, rows)
    for name, r in rows.items():
        assert r["vspill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
    for name, r in rows.items():
        if "opstep_elem_p2_kernel" in name:
            assert r["vgpr"] <= 170 and r["occ"] >= 3, (name, r)
        if "opstep_node_kernel<0, false>" in name:
            assert r["occ"] == 8, (name, r)
