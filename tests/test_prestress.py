"""Prestressed modal analysis, on the CPU: the dense double of tests/prestress_double.py is qualified here - against the
unstressed pair, against the figures the load case was sized with - and the pieces of the product that need no GPU: the
argument checks of ``saa_operator_tangent_apply_block``, the driver's refusals, and the iteration of ``modal.lowest_modes`` on a
tangent that may be indefinite, fed the dense pair."""
import ctypes as C

import numpy as np
import pytest

import finite_strain_double as fd
import p2_double
import prestress_double as pd


# ---- the library's argument checks ----------------------------------------------------------------------------------------------

def _block(lib, handle, material, m, u=8, v=8, kv=8, ldv=100, ldkv=100):
    ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
    return lib.saa_operator_tangent_apply_block(ptr(handle), material, ptr(u), m, ptr(v), ldv, ptr(kv), ldkv, None)


def test_the_binding_has_the_block_entry():
    from synchronization_avoiding_algorithms_amd import _lib, modal

    assert _lib.SIGNATURES["saa_operator_tangent_apply_block"] == (
        C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)])
    assert "saa_optan_block.hip" in _lib.SOURCES
    assert hasattr(modal.ModalOperator, "tangent_apply_block") and hasattr(modal, "prestressed_modes")


def test_the_block_entry_checks_its_arguments_before_the_device():
    from synchronization_avoiding_algorithms_amd import _lib

    lib = _lib.load()
    for material in (-1, 3):
        assert _block(lib, 8, material, 1) == _lib.SAA_E_ARG
        assert b"saa_operator_tangent_apply_block" in lib.saa_last_error() and b"material" in lib.saa_last_error()
    for m in (0, 17):
        assert _block(lib, 8, 1, m) == _lib.SAA_E_ARG
        assert b"1 <= m <= 16" in lib.saa_last_error() and f"m = {m}".encode() in lib.saa_last_error()
    for ld in ({"ldv": -1}, {"ldkv": -1}):
        assert _block(lib, 8, 1, 2, **ld) == _lib.SAA_E_ARG and b"negative leading dimension" in lib.saa_last_error()
    assert _block(lib, None, 1, 1) == _lib.SAA_E_ARG and b"null handle" in lib.saa_last_error()
    assert _block(lib, None, 0, 16, u=None) == _lib.SAA_E_ARG and b"null handle" in lib.saa_last_error()


# ---- the double agrees with itself ------------------------------------------------------------------------------------------------

def test_at_rest_the_double_is_the_unstressed_pair():
    from scipy.linalg import eigh

    pts, cells, dd, fs = pd.problem("beam36")
    K, M = p2_double.assemble(pts, cells, dd, pd.LMD, pd.MU, fd.RHO, mass_rule=4)
    free = np.nonzero(fs.free)[0]
    want = eigh(K[np.ix_(free, free)], M[np.ix_(free, free)], eigvals_only=True)
    zero = np.zeros(3 * len(pts))
    for material in fd.MATERIALS:
        got = pd.eigenvalues("beam36", material, zero)
        assert np.abs(got / want - 1.0).max() <= 1e-9, material
    # order 1: both materials linearise to one K, and the mass carries rho times the volume on every axis
    a, b = pd.eigenvalues("structured288", "svk", np.zeros(3 * 117)), pd.eigenvalues("structured288", "neo_hookean", np.zeros(3 * 117))
    assert np.abs(a / b - 1.0).max() <= 1e-9 and (a > 0).all()
    pts, cells, dd, fs = pd.problem("structured288")
    p = pts[cells]
    Mfull = pd.mass_matrix("structured288")
    ones = np.tile(np.array([1.0, 0.0, 0.0]), len(pts))
    volume = np.abs(np.linalg.det(p[:, 1:] - p[:, :1])).sum() / 6.0
    assert abs(volume - 6.0) < 1e-12
    clamped = np.asarray(fs.free, dtype=np.float64)
    # x^T M x of the unit translation restricted to the free dofs is below rho V and above that of the elements off the clamp
    assert 0.8 * fd.RHO * volume < (ones * clamped) @ Mfull @ (ones * clamped) < fd.RHO * volume


@pytest.mark.parametrize("name", pd.MESHES)
@pytest.mark.parametrize("material", fd.MATERIALS)
def test_the_double_reproduces_the_load_case(name, material):
    """Newton to 1e-12, nothing near inversion, a positive definite tangent, and the shift of the lowest ``omega^2`` to the three
    digits the load case was sized with: tens of per cent either way."""
    fs = pd.problem(name)[3]
    w0 = pd.unstressed(name)
    for fx in pd.FX:
        u, res = pd.equilibrium(name, material, fx)
        w = pd.prestressed(name, material, fx)
        ratio = float(w[0] / w0[0])
        print(f"{name} {material} fx {fx:+.0f}: residual {res:.1e}, min det F {float(fs.det_f(u).min()):.4f}, ratio {ratio:.6f}")
        assert res <= 1e-12 and float(fs.det_f(u).min()) >= 0.99 and w[0] > 0
        assert abs(ratio - pd.RATIO[fx][name][material]) <= 5.01e-4
        assert (ratio < 1.0) == (fx < 0)
    u, w = pd.unstable(name, material)
    print(f"{name} {material} 3 u*: lowest omega^2 {w[0]:.3f}, {int((w < 0).sum())} negative, min det F {float(fs.det_f(u).min()):.4f}")
    assert float(fs.det_f(u).min()) >= 0.97
    assert int((w < 0).sum()) == pd.UNSTABLE[name]["negative"] and abs(w[0] - pd.UNSTABLE[name][material]) <= 0.51


# ---- the driver's refusals --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,message", ((["--fx", "5"], "a linear operator's modes do not depend on the load"),
                                           (["--material", "svk", "--load-steps", "0"], "modal --load-steps must be >= 1")))
def test_driver_refuses(capsys, extra, message):
    from synchronization_avoiding_algorithms_amd import drivers

    with pytest.raises(SystemExit) as exc:
        drivers.main(["modal", "--synthetic", "1", *extra])
    assert exc.value.code != 0
    err = capsys.readouterr().err
    assert message in " ".join(err.split()) and "Traceback" not in err
    assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


# ---- the iteration on the CPU -----------------------------------------------------------------------------------------------------

def _dense_modes(name, material, u, **kw):
    import torch

    from synchronization_avoiding_algorithms_amd import modal

    K, M, _ = pd.pair(name, material, u)
    fs = pd.problem(name)[3]
    Kt, Mt = torch.as_tensor(K), torch.as_tensor(M)
    K0 = torch.as_tensor(pd.pair(name, "svk", np.zeros_like(u))[0])       # the preconditioner: diag K of the linear operator
    free = torch.as_tensor(np.asarray(fs.free, dtype=np.float64))
    return modal.lowest_modes(lambda X: X @ Kt, lambda X: X @ Mt, 4, free, diag_k=torch.diagonal(K0) * free, **kw)


@pytest.mark.parametrize("name,material", (("structured288", "neo_hookean"), ("beam36", "svk")))
def test_the_iteration_converges_at_an_equilibrium(name, material):
    u = pd.equilibrium(name, material, -2000.0)[0]
    want = pd.prestressed(name, material, -2000.0)[:4]
    got = _dense_modes(name, material, u, indefinite=True)
    err = float(np.abs(got["omega2"] / want - 1.0).max())
    print(f"{name} {material}: {got['outer_iterations']} sweeps, {got['inner_iterations']} inner iterations, residuals "
          f"{got['residuals'].max():.1e}, omega^2 against eigh {err:.1e}")
    assert got["stable"] is True and got["converged"] and got["residuals"].max() <= 1e-8 and err <= 1e-8
    assert got["lowest_ritz"] == got["omega2"][0]
    plain = _dense_modes(name, material, u)                               # the iteration itself is what it was
    assert set(got) == set(plain) | {"stable", "lowest_ritz"}
    assert np.array_equal(plain["omega2"], got["omega2"]) and plain["inner_iterations"] == got["inner_iterations"]


@pytest.mark.parametrize("name", pd.MESHES)
@pytest.mark.parametrize("material", fd.MATERIALS)
def test_the_iteration_answers_an_unstable_state(name, material):
    """``3 u*``: the tangent has negative eigenvalues; without ``indefinite`` this is the case that raises inside scipy."""
    u, w = pd.unstable(name, material)
    got = _dense_modes(name, material, u, indefinite=True)
    print(f"{name} {material}: lowest_ritz {got['lowest_ritz']:.3f} (dense {w[0]:.3f}) after {got['outer_iterations']} sweeps, "
          f"{got['inner_iterations']} inner iterations")
    assert got["stable"] is False and got["converged"] is False
    assert got["frequencies_hz"] is None and got["omega2"] is None
    assert np.isfinite(got["lowest_ritz"]) and got["lowest_ritz"] < 0 and got["lowest_ritz"] >= w[0] - 1e-8 * abs(w[0])
