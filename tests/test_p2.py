"""Quadratic (10-node) tetrahedra without a GPU: the mesh elevation, the NumPy double of the element formulas
(tests/p2_double.py) against the reference's own results (tests/golden/p2_beam.npz, written by make_golden_p2.py), the
reason for the mass-rule deviation, the library's new entry points and the register budget of csrc/saa_p2.hip.

Bars: rel-L2 < 1e-13 for ``K X``, ``F``, ``diag K`` and the element matrices (the project's ``K d`` bar);
< 1e-9 for the steady solution (the p = 1 bar of tests/test_steady.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import p2_double as p2
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd.mesh import TET10_EDGES, read_vtk, structured_beam, to_quadratic
from synchronization_avoiding_algorithms_amd.Tools.Shape_function_Deriv import Shape_Function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("straight", "curved")


@pytest.fixture(scope="module")
def gold():
    return load_golden("p2_beam.npz")


# ---- mesh ------------------------------------------------------------------------------------------------------------

def test_to_quadratic_adds_one_midpoint_node_per_unique_edge():
    lin = structured_beam(2, length=6.0)
    quad = to_quadratic(lin)
    t10 = quad.tets10
    edges = np.unique(np.sort(np.concatenate([lin.tets[:, list(e)] for e in TET10_EDGES]), axis=1), axis=0)
    assert len(quad.points) == len(lin.points) + len(edges) == 625 and t10.shape == (288, 10)
    assert np.array_equal(quad.tets, lin.tets) and np.array_equal(quad.triangles, lin.triangles)
    assert np.array_equal(t10[:, :4], lin.tets) and np.array_equal(quad.points[:len(lin.points)], lin.points)
    # appended in lexicographic order of (min id, max id), each at its edge's midpoint
    assert np.array_equal(quad.points[len(lin.points):], 0.5 * (lin.points[edges[:, 0]] + lin.points[edges[:, 1]]))
    for k, (a, b) in enumerate(TET10_EDGES):
        assert np.array_equal(quad.points[t10[:, 4 + k]], 0.5 * (quad.points[t10[:, a]] + quad.points[t10[:, b]]))
    # elements sharing an edge share its node: the node id is a function of the vertex pair
    seen = {}
    for cell in t10:
        for k, (a, b) in enumerate(TET10_EDGES):
            key = (min(cell[a], cell[b]), max(cell[a], cell[b]))
            assert seen.setdefault(key, cell[4 + k]) == cell[4 + k]
    assert len(seen) == len(edges)
    again = to_quadratic(structured_beam(2, length=6.0))
    assert np.array_equal(again.points, quad.points) and np.array_equal(again.tets10, t10)


def test_local_node_order_is_the_shape_functions_order():
    ref = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.float64)
    nodes = np.concatenate([ref, [0.5 * (ref[a] + ref[b]) for a, b in TET10_EDGES]])
    N = np.array([Shape_Function(2, x) for x in nodes])
    assert np.abs(N - np.eye(10)).max() < 1e-15


def test_vtk_type_24_round_trip(tmp_path):
    from synchronization_avoiding_algorithms_amd.steady import write_vtk_point_data

    quad = to_quadratic(structured_beam(1, length=2.0))
    d = np.arange(3 * len(quad.points), dtype=np.float64)
    path = write_vtk_point_data(str(tmp_path / "q.vtk"), quad.points, quad.tets10, d)
    back = read_vtk(path)
    assert set(back.cells_dict) == {"tetra10"}
    assert np.array_equal(back.tets10, quad.tets10) and np.array_equal(back.points, quad.points)
    text = open(path).read()
    assert f"CELLS {len(quad.tets10)} {11 * len(quad.tets10)}" in text and "\n24\n" in text
    # a linear file parses as before
    lin = structured_beam(1, length=2.0)
    back = read_vtk(write_vtk_point_data(str(tmp_path / "l.vtk"), lin.points, lin.tets, np.zeros(3 * len(lin.points))))
    assert set(back.cells_dict) == {"tetra"} and np.array_equal(back.tets, lin.tets)


# ---- the double against the reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SETS)
def test_double_matches_the_reference_assembly(gold, name):
    pts, c10, dd = gold[f"points_{name}"], gold["cells10"], gold["dirichlet_dofs"]
    lmd, mu, rho, fz = (float(gold[k]) for k in ("lmd", "mu", "rho", "fz"))
    KX = p2.apply_k(pts, c10, dd, lmd, mu, gold["X"].T)
    errs = [rel_l2(KX[j], gold[f"KX_{name}"][:, j]) for j in range(3)]
    ef = rel_l2(p2.load(pts, c10, dd, (0.0, -fz, -fz)), gold[f"F_{name}"])
    ed = rel_l2(p2.diagonals(pts, c10, dd, lmd, mu, rho)[0], gold[f"diagK_{name}"])
    print(name, "K X", errs, "F", ef, "diag K", ed)
    assert max(errs) < 1e-13 and ef < 1e-13 and ed < 1e-13
    assert np.all(KX[:, dd] == 0.0)


@pytest.mark.parametrize("name", SETS)
def test_double_matches_the_reference_element_matrices(gold, name):
    pts, c10 = gold[f"points_{name}"], gold["cells10"]
    lmd, mu, rho, fz = (float(gold[k]) for k in ("lmd", "mu", "rho", "fz"))
    Me4, Ke, Fe = p2.element_matrices(pts, c10[gold["elements"]], lmd, mu, rho, (0.0, -fz, -fz), mass_rule=2)
    ek, ef, em = rel_l2(Ke, gold[f"Ke_{name}"]), rel_l2(Fe, gold[f"Fe_{name}"]), rel_l2(Me4, gold[f"Me_{name}"])
    print(name, "Ke", ek, "Fe", ef, "Me (4-point)", em)
    assert ek < 1e-13 and ef < 1e-13 and em < 1e-13


@pytest.mark.parametrize("name", SETS)
def test_cg_on_the_double_reaches_the_reference_steady_solution(gold, name):
    pts, c10, dd = gold[f"points_{name}"], gold["cells10"], gold["dirichlet_dofs"]
    lmd, mu, rho, fz = (float(gold[k]) for k in ("lmd", "mu", "rho", "fz"))
    b = p2.load(pts, c10, dd, (0.0, -fz, -fz))
    dk, _ = p2.diagonals(pts, c10, dd, lmd, mu, rho)
    d, its = p2.pcg(lambda v: p2.apply_k(pts, c10, dd, lmd, mu, v)[0], b, dk)
    err = rel_l2(d, gold[f"d_steady_{name}"])
    print(name, "iterations", its, "rel-L2 to d_steady", err)
    assert err < 1e-9


# ---- mass: why the 14-point rule ------------------------------------------------------------------------------------------

def test_reference_four_point_mass_has_rank_twelve(gold):
    for name in SETS:
        for Me in gold[f"Me_{name}"]:
            assert np.linalg.matrix_rank(Me) == 12


def test_fourteen_point_mass_is_positive_definite_and_exact_in_total():
    quad = to_quadratic(structured_beam(1, length=6.0))
    assert quad.tets10.shape == (36, 10) and 3 * len(quad.points) == 351
    rho = 1.7
    _, M14 = p2.assemble(quad.points, quad.tets10, [], 1.0, 1.0, rho)
    _, M4 = p2.assemble(quad.points, quad.tets10, [], 1.0, 1.0, rho, mass_rule=2)
    ev14, ev4 = np.linalg.eigvalsh(M14), np.linalg.eigvalsh(M4)
    print("14-point: smallest", ev14[0], " 4-point: smallest", ev4[0], "zeros", int((np.abs(ev4) < 1e-12 * ev4[-1]).sum()))
    assert ev14[0] > 1e-3 * rho
    assert (np.abs(ev4) < 1e-12 * ev4[-1]).sum() == 18            # the reference's assembled mass is singular
    ones = np.zeros(351)
    ones[0::3] = 1.0
    assert abs(ones @ M14 @ ones - rho * 6.0) < 1e-13 * rho * 6.0  # total mass = rho x volume
    assert rel_l2(p2.apply_m(quad.points, quad.tets10, [], rho, ones)[0], M14 @ ones) < 1e-13
    assert rel_l2(p2.diagonals(quad.points, quad.tets10, [], 1.0, 1.0, rho)[1], np.diag(M14)) < 1e-13


# ---- library -----------------------------------------------------------------------------------------------------------

# Four new entry points (include/saa_hip.h, ABI 15); the fifth function the order-2 handle works through, saa_operator_apply,
# exists since ABI 11 and changes in meaning only, so it is checked for presence but is no new symbol.
NEW_SYMBOLS = ("saa_operator_create_p2", "saa_operator_order", "saa_operator_load", "saa_operator_diagonal")


def test_library_exports_the_order_two_entry_points():
    assert _lib.ABI_VERSION >= 15
    assert "saa_p2.hip" in _lib.SOURCES
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.saa_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS + ("saa_operator_apply",):
        assert hasattr(lib, name), name
    header = open(_lib.HEADER).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    # argument checks that need no device
    h = C.c_void_p()
    assert lib.saa_operator_create_p2(0, 0, 0, None, None, None, 0, 1.0, 1.0, 1.0, C.byref(h)) == _lib.SAA_E_ARG
    assert lib.saa_operator_order(None) == _lib.SAA_E_ARG
    assert lib.saa_operator_load(None, 0.0, 0.0, 0.0, None) == _lib.SAA_E_ARG
    assert lib.saa_operator_diagonal(None, None, None) == _lib.SAA_E_ARG
    pts = np.zeros(3 * 10)
    bad = np.arange(10, dtype=np.int32)
    bad[9] = 10
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.saa_operator_create_p2(0, 10, 1, pts.ctypes.data_as(dp), bad.ctypes.data_as(ip), None, 0, 1.0, 1.0, 1.0,
                                      C.byref(h)) == _lib.SAA_E_ARG
    assert b"node id out of range" in lib.saa_last_error()


def test_drop_ins_take_order_two_and_reject_other_orders():
    from synchronization_avoiding_algorithms_amd.Tools import Steady_solvers as SS

    quad = to_quadratic(structured_beam(1, length=2.0))
    elas = type("E", (), {"lmd": 1.0, "mu": 1.0, "rho": 1.0, "fz": 0.5, "R": False})()
    for p in (0, 3):
        with pytest.raises(NotImplementedError):
            SS.Steady_Elasticity_solver(p, quad.tets10, quad.points, [], elas)
        with pytest.raises(NotImplementedError):
            SS.Eigen_mode(p, quad.tets10, quad.points, [], elas)
    with pytest.raises(NotImplementedError, match="10-node"):
        SS.Steady_Elasticity_solver(2, quad.tets, quad.points, [], elas)


def test_driver_help_lists_order():
    from synchronization_avoiding_algorithms_amd import drivers

    ap_help = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "modal", "--help"],
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert ap_help.returncode == 0 and "--order" in ap_help.stdout
    assert drivers.steady_state.__defaults__[-1] == 1 and drivers.modal.__defaults__[-1] == 1


# ---- compile time ------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_p2_kernels_use_no_scratch_and_spill_no_vector_register():
    """One lane per element: the kernels of saa_p2.hip keep the element in registers only because the element pass streams
    the displacements instead of holding 30 + 30 + 30 values (saa_p2.hip, header).  A change that pushes an array into
    scratch memory would keep every parity test green and cost a multiple of the run time."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_p2.hip"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
    print(out.stdout)
    for kernel in ("p2_apply_k_kernel", "p2_apply_m_kernel", "p2_load_kernel", "p2_diag_k_kernel", "p2_diag_m_kernel",
                   "p1_load_diag_kernel"):
        assert any(kernel in k for k in rows), (kernel, rows)
    for name, r in rows.items():
        assert r["vspill"] == 0 and r["scratch"] == 0, (name, r)
    # two waves per SIMD at least for the two hot kernels (256 registers per lane)
    for name, r in rows.items():
        if "p2_apply" in name:
            assert r["vgpr"] <= 256 and r["occ"] >= 2, (name, r)
