"""Finite-strain materials on the operator handle without a GPU: the NumPy double of tests/finite_strain_double.py checked
against itself (force = gradient of the stored energy, linearisation to the handle's K, rigid motions), the new entry points
and the argument checks that need no device, and the register budget of csrc/saa_opfs.hip.

Bars.  Force against the central difference of ``Pi`` in longdouble at ``h = 1e-6``: the truncation is ``h^2 Pi'''/6`` and the
round-off ``eps_ld Pi / h`` with ``eps_ld = 1.1e-19``, both far below the bar 1e-8 of ``max|f|`` (a float64 prototype gave
6e-11 and 1.6e-10).  Linearisation: ``|f_fs(eps u) - K eps u| / |K eps u|`` is first order in ``eps``, so halving ``eps``
halves it; each ratio in [1.9, 2.1].  Rigid motion ``u = (R - I) X + c``, 0.5 rad, no Dirichlet dofs: ``F = R``, ``E = 0``,
``P = 0`` exactly, so ``max|f_fs| <= 1e-12 max|K u|`` (measured: 2e-18 .. 5e-15 in longdouble)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import finite_strain_double as fd
from synchronization_avoiding_algorithms_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = fd.lame(fd.E, fd.NU)

# tools/kernel_resources.py --file=saa_opfs.hip as hipcc gives them: sgpr vgpr sgpr_spill vgpr_spill scratch occupancy
OPFS_ROWS = {
    "void saa::opfs_elem_p2_kernel<1, false>": (44, 126, 0, 0, 0, 4),
    "void saa::opfs_elem_p1_kernel<1, false>": (22, 72, 0, 0, 0, 7),
    "void saa::opfs_elem_p2_kernel<2, false>": (34, 237, 0, 0, 0, 2),
    "void saa::opfs_elem_p1_kernel<2, false>": (20, 91, 0, 0, 0, 5),
    "void saa::opfs_elem_p2_kernel<1, true>": (46, 130, 0, 0, 0, 3),
    "void saa::opfs_elem_p1_kernel<1, true>": (22, 78, 0, 0, 0, 6),
    "void saa::opfs_elem_p2_kernel<2, true>": (42, 242, 0, 0, 0, 2),
    "void saa::opfs_elem_p1_kernel<2, true>": (24, 84, 0, 0, 0, 5),
}

SIGNATURES = {
    "saa_operator_internal_force": (
        (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
        "int saa_operator_internal_force(saa_operator *op, int32_t material, const double *x_dev, double *f_dev, "
        "double *energy_elem_dev /* n_elems or NULL */, int64_t *n_inverted /* or NULL */)"),
    "saa_operator_stepper_set_material": (
        (C.c_int, [C.c_void_p, C.c_int32]), "int saa_operator_stepper_set_material(saa_operator_stepper *st, int32_t material)"),
    "saa_operator_stepper_inverted": (
        (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "int saa_operator_stepper_inverted(saa_operator_stepper *st, int64_t *count, int64_t *first_step /* -1: none */)"),
}


@pytest.fixture(scope="module")
def doubles():
    """name -> (FiniteStrain clamped, FiniteStrain free, a seeded field with min det F >= 0.2 and max|H| >= 0.1)."""
    out = {}
    for k, name in enumerate(fd.MESHES):
        pts, cells, dd = fd.mesh(name)
        fs = fd.FiniteStrain(pts, cells, LMD, MU, dd)
        u, det, hmax = fd.scale_to_strain(fs, fd.smooth_random_field(pts, 40 + k))
        assert det >= 0.2 and hmax >= 0.1
        out[name] = (fs, fd.FiniteStrain(pts, cells, LMD, MU, ()), u, pts)
    return out


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_force_is_the_gradient_of_the_energy(doubles, name, material):
    fs, _, u, _ = doubles[name]
    f = fs.force(u, material)
    rng = np.random.default_rng(7)
    dofs = rng.choice(np.nonzero(fs.free)[0], size=10, replace=False)
    h = np.longdouble(1e-6)
    worst = 0.0
    for i in dofs:
        up, um = np.asarray(u, dtype=np.longdouble), np.asarray(u, dtype=np.longdouble)
        up[i], um[i] = up[i] + h, um[i] - h
        g = (fs.total_energy(up, material) - fs.total_energy(um, material)) / (2 * h)
        worst = max(worst, float(abs(g - f[i]) / np.abs(f).max()))
    print(name, material, "max |dPi/du - f| / max|f| =", worst)
    assert worst <= 1e-8


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_linearises_to_the_handles_operator(doubles, name, material):
    fs, _, u, _ = doubles[name]
    rel = []
    for eps in (1e-3, 5e-4, 2.5e-4):
        ku = fs.linear_force(eps * u)
        d = fs.force(eps * u, material) - ku
        rel.append(float(np.sqrt((d * d).sum() / (ku * ku).sum())))
    print(name, material, "relative differences", rel, "ratios", rel[0] / rel[1], rel[1] / rel[2])
    assert 1.9 <= rel[0] / rel[1] <= 2.1 and 1.9 <= rel[1] / rel[2] <= 2.1


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_rigid_motion_gives_no_force(doubles, name, material):
    _, free, _, pts = doubles[name]
    u = fd.rigid_motion(pts, 0.5)
    ku = np.abs(free.linear_force(u)).max()
    f = np.abs(free.force(u, material)).max()
    print(name, material, "max|f_fs| / max|K u| =", float(f / ku), "max|K u| =", float(ku))
    assert float(ku) > 1e3 and f <= 1e-12 * ku
    assert float(free.det_f(u).min()) > 0.99


def test_inverted_elements_are_dropped_in_the_double(doubles):
    """A vertex pushed through its opposite faces inverts exactly the elements around it, under neo-Hooke only; they
    contribute nothing, and what is left is the force of the mesh without them."""
    fs, _, _, pts = doubles["beam36"]
    node, u, star = fd.inversion_state(fs, pts, 0.02 * fd.smooth_random_field(pts, 3))
    f, en, inv = fs.evaluate(u, "neo_hookean")
    assert list(np.nonzero(inv)[0]) == list(star) == list(np.nonzero((fs.cells[:, :4] == node).any(axis=1))[0])
    assert np.isfinite(np.asarray(f, dtype=np.float64)).all() and (en[inv] == 0).all() and float(np.abs(f).max()) > 1.0
    keep = np.setdiff1d(np.arange(fs.n_elems), star)
    rest = fd.FiniteStrain(pts, fs.cells[keep], LMD, MU, np.nonzero(~fs.free)[0])
    assert float(np.abs(rest.force(u, "neo_hookean") - f).max()) <= 1e-17 * float(np.abs(f).max())
    assert not fs.evaluate(u, "svk")[2].any()


def test_library_exports_the_entry_points():
    lib = _lib.load()
    header = open(_lib.HEADER).read()
    for name, (sig, text) in SIGNATURES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
        assert _lib.SIGNATURES[name] == sig
        decl = header[header.index("int " + name + "("):]
        assert " ".join(decl[:decl.index(";")].split()) == text
    for k, v in (("SAA_MATERIAL_LINEAR", 0), ("SAA_MATERIAL_SVK", 1), ("SAA_MATERIAL_NEO_HOOKEAN", 2)):
        assert f"#define {k} {v}" in header
    assert _lib.SOURCES.index("saa_opfs.hip") < _lib.SOURCES.index("saa_api.cpp") == len(_lib.SOURCES) - 1
    assert _lib.ABI_VERSION == 16 and lib.saa_abi_version() == 16
    assert [_lib.material_id(n) for n in ("linear", "svk", "neo_hookean", "neo-hookean")] == [0, 1, 2, 2]
    with pytest.raises(ValueError):
        _lib.material_id("rubber")
    from synchronization_avoiding_algorithms_amd import dynamics, modal

    assert hasattr(modal.ModalOperator, "internal_force")
    assert hasattr(dynamics.OperatorStepper, "set_material") and hasattr(dynamics.OperatorStepper, "inverted")
    assert hasattr(dynamics.OperatorPartition, "inverted")


def test_argument_checks_need_no_device():
    lib = _lib.load()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is looked at
    n = C.c_int64(0)
    for material in (-1, 3, 99):
        assert lib.saa_operator_internal_force(fake, material, fake, fake, None, C.byref(n)) == _lib.SAA_E_ARG
        assert b"material" in lib.saa_last_error() and b"none of" in lib.saa_last_error()
        assert lib.saa_operator_stepper_set_material(fake, material) == _lib.SAA_E_ARG
        assert b"material" in lib.saa_last_error() and b"none of" in lib.saa_last_error()
    empty = C.c_void_p(0)           # a handle that holds a null implementation pointer is a null handle too
    for handle in (None, C.byref(empty)):
        assert lib.saa_operator_internal_force(handle, 1, fake, fake, None, None) == _lib.SAA_E_ARG
        assert b"null handle" in lib.saa_last_error()
        assert lib.saa_operator_stepper_set_material(handle, 1) == _lib.SAA_E_ARG
        assert b"null handle" in lib.saa_last_error()
        assert lib.saa_operator_stepper_inverted(handle, C.byref(n), C.byref(n)) == _lib.SAA_E_ARG
        assert b"null handle" in lib.saa_last_error()


def test_driver_refuses_the_energy_balance_with_a_nonlinear_material(capsys):
    from synchronization_avoiding_algorithms_amd import drivers

    with pytest.raises(SystemExit) as exc:
        drivers.main(["dynamics", "--synthetic", "1", "--material", "svk", "--energy"])
    assert exc.value.code != 0
    assert "the energy balance is defined for the linear material only" in capsys.readouterr().err


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
def test_finite_strain_kernels_use_no_scratch_and_keep_two_waves():
    """No scratch and no spill anywhere in saa_opfs.hip, at least two waves per SIMD for the order-2 passes; the rows as
    hipcc gives them.  St. Venant-Kirchhoff fits the linear stored-geometry pass's budget (126 against 148 vector registers,
    four waves against three, because each point reads its own G instead of all 36 up front); neo-Hooke's cofactors and the
    fp64 log1p take it to 237 and two waves (225 with the textbook form from F, which lost its digits at small strain)."""
    rows = _rows("saa_opfs.hip")
    for name, (sgpr, vgpr, sspill, vspill, scratch, occ) in rows.items():
        assert sspill == 0 and vspill == 0 and scratch == 0, (name, rows[name])
        if "opfs_elem_p2_kernel" in name:
            assert occ >= 2, (name, rows[name])
    assert rows == OPFS_ROWS
