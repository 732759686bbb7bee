"""Stress recovery and error estimate of quadratic tetrahedra without a GPU: the library's entry points and their argument
checks, the NumPy double (tests/p2_stress_double.py) against closed forms - the patch test, the h^2 rate of the estimate on a
cubic field, the energy identity on curved elements - the drivers on the double, and the register budget of
csrc/saa_stress_p2.hip.

Bars.  Patch test: a quadratic displacement has a linear stress, which the element-linear field, the recovered nodal stress
and the quadratic interpolant reproduce, so stresses agree to 1e-12 of their maximum and ``eta2_total <= 1e-22 * 2 *
energy_total`` (the bound of tests/test_estimate.py; measured eta^2 / 2W about 2e-30 and 8e-30 at n = 1, 2).  Cubic field
(``p2_stress_double.cubic_field``, seed 0): the stress is quadratic, the element-linear stress misses it by O(h^2), so eta
and the true error fall by 4 per halving: eta ratio in [3.7, 4.3] (measured 3.846 and 3.956 for n = 1 -> 2 -> 4, the true
error's 4.000 twice) and effectivity eta / |error| in [0.6, 1.0] (measured 0.715, 0.744, 0.752, boundary elements
included).  Energy: ``sum_e W_e = x . K x / 2`` to 1e-13 on the reference's curved fixture."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

import p2_double as p2
import p2_stress_double as psd
from estimate_double import quadratic_field
from stress_double import parse_vtk
from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd.fem_setup import lame
from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = lame(1e6, 0.3)
NEW_SYMBOLS = ("saa_operator_stress_p2", "saa_operator_nodal_stress_p2", "saa_operator_stress_error_p2")


def test_library_exports_the_entry_points_and_header_and_binding_agree():
    assert "saa_stress_p2.hip" in _lib.SOURCES
    lib = _lib.load()
    header = open(_lib.HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    # one ctypes argument per parameter of the declaration
    import re

    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        params = re.search(name + r"\s*\(([^)]*)\)", flat).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name][1]), name
    # the paragraph on the linear entry points stays and points to the new ones
    assert "on an order-2 handle they return SAA_E_ARG" in header and "saa_operator_stress_p2, saa_operator_nodal_stress_p2" in header


def test_argument_checks_need_no_device():
    lib = _lib.load()
    fake = C.c_void_p(8)            # never dereferenced: every check below fails before the handle is read
    calls = {
        "saa_operator_stress_p2": lambda h, m: lib.saa_operator_stress_p2(h, m, fake, 0, fake, 0, None, 0, None, 0, None, None, None),
        "saa_operator_nodal_stress_p2": lambda h, m: lib.saa_operator_nodal_stress_p2(h, m, fake, 0, fake, 0),
        "saa_operator_stress_error_p2": lambda h, m: lib.saa_operator_stress_error_p2(h, m, fake, 0, fake, 0, None, 0, fake, 0,
                                                                                      None, None, None),
    }
    for name, call in calls.items():
        assert call(None, 1) == _lib.SAA_E_ARG
        assert lib.saa_last_error().decode() == name + ": null handle"
        for m in (0, 17, -3):
            assert call(fake, m) == _lib.SAA_E_ARG
            msg = lib.saa_last_error().decode()
            assert msg.startswith(name + ": m = %d columns" % m), msg


def test_driver_help_names_stress_and_estimate_under_order_and_refuses_modeled():
    def run(*args):
        return subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=ROOT,
                              capture_output=True, text=True, timeout=300)

    out = run("--help")
    assert out.returncode == 0
    text = " ".join(out.stdout.split())
    at = text.index("--order {1,2}", text.index("options:") if "options:" in text else 0)
    para = text[at:at + 400]
    assert "stress" in para and "estimate" in para, para
    for cmd in ("stress", "estimate"):
        out = run(cmd, "--order", "2", "--modeled", "--synthetic", "1")
        assert out.returncode != 0 and "no modelled p = 2 run" in out.stderr, out.stderr[-500:]


@pytest.mark.parametrize("n", (1, 2))
def test_patch_test_of_the_double(n):
    quad = to_quadratic(structured_beam(n, length=6.0))
    ns = psd.NumpyQuadraticStress(quad.points, quad.tets10, LMD, MU)
    u, exact = quadratic_field(quad.points, ns.D)
    el = ns.element(u[None])
    _, at_gauss = quadratic_field(ns.gauss_positions().reshape(-1, 3), ns.D)
    top = np.abs(exact).max()
    e_gauss = np.abs(el["sigma"][0].reshape(-1, 6) - at_gauss).max() / top
    nodal = ns.nodal(el["sigma"])
    e_nodal = np.abs(nodal[0] - exact).max() / top
    er = ns.error(el["sigma"], nodal=nodal)
    ratio = er["eta2_total"][0] / (2.0 * el["energy_total"][0])
    print(f"n = {n}: Gauss {e_gauss:.2e} nodal {e_nodal:.2e} eta2 / 2W {ratio:.2e}")
    assert e_gauss < 1e-12 and e_nodal < 1e-12
    assert er["eta2_total"][0] <= 1e-22 * 2.0 * el["energy_total"][0]
    # the closed form of the issue for the vertex values of the element-linear field
    b, qv = 0.1381966011250105, (3, 0, 1, 2)
    S = el["sigma"].sum(axis=2)
    closed = np.stack([np.sqrt(5.0) * (el["sigma"][:, :, qv[v]] - b * S) for v in range(4)], axis=2)
    assert np.abs(ns.vertex_values(el["sigma"]) - closed).max() < 1e-13 * top


def test_cubic_field_eta_falls_like_h_squared():
    def make(points, cells10, u):
        ns = psd.NumpyQuadraticStress(points, cells10, LMD, MU)
        el = ns.element(u[None])
        return el["sigma"][0], ns.error(el["sigma"], nodal=ns.nodal(el["sigma"]))["eta2_total"][0]

    psd.check_cubic_series(*psd.cubic_series(make, LMD, MU))


@pytest.mark.parametrize("name", ("straight", "curved"))
def test_energy_is_half_x_k_x_on_the_reference_fixture(name):
    g = load_golden("p2_beam.npz")
    pts, c10 = g[f"points_{name}"], g["cells10"]
    lmd, mu = float(g["lmd"]), float(g["mu"])
    X = g["X"].T.copy()
    ns = psd.NumpyQuadraticStress(pts, c10, lmd, mu)
    assert (p2.geometry(pts, c10, 2)[0] > 0).all()
    W = ns.element(X)["energy_total"]
    want = 0.5 * np.einsum("mi,mi->m", X, p2.apply_k(pts, c10, (), lmd, mu, X))
    print(name, "energy", W, "x.Kx/2 - 1", W / want - 1.0)
    assert np.abs(W / want - 1.0).max() < 1e-13


def test_drivers_on_the_double(tmp_path):
    """``drivers.stress_p2`` and ``drivers.estimate_p2`` with the NumPy double as the recovery: the report, the history
    file and the VTK files (type-24 cells, the arrays in place)."""
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio

    mesh = structured_beam(1, length=6.0)
    quad = to_quadratic(mesh)
    ns = psd.NumpyQuadraticStress(quad.points, quad.tets10, LMD, MU)
    u, _ = psd.cubic_field(quad.points, ns.D)
    traj = np.stack([0.0 * u, 0.5 * u, u], axis=1)
    rio.save_displacement(str(tmp_path / drivers.PATHS["dynamics"].format(p=2)), traj)
    make = lambda p, c, l, m: psd.NumpyQuadraticStress(p, c, l, m)  # noqa: E731
    rep = drivers.stress_p2(mesh, str(tmp_path), columns=(0, -1), history=True, recovery=make)
    el = ns.element(traj.T)
    assert rep["order"] == 2 and rep["n_elems"] == 36 and rep["n_nodes"] == 117 and rep["n_saved"] == 3
    assert [c["column"] for c in rep["columns"]] == [0, 2]
    last = rep["columns"][1]
    assert set(last) >= {"column", "strain_energy", "von_mises_max", "element", "gauss_point", "position", "centroid"}
    assert last["strain_energy"] == pytest.approx(el["energy_total"][2], rel=1e-13)
    assert last["von_mises_max"] == pytest.approx(el["von_mises_max"][2], rel=1e-13)
    assert 4 * last["element"] + last["gauss_point"] == el["von_mises_argmax"][2]
    assert np.allclose(last["position"], ns.gauss_positions()[last["element"], last["gauss_point"]], atol=1e-14)
    assert rep["columns"][0]["von_mises_max"] == 0.0 and rep["columns"][0]["element"] == 0
    with np.load(rep["history"]) as h:
        assert np.allclose(h["strain_energy"], el["energy_total"], rtol=1e-13) and h["von_mises_element"][2] == last["element"]
    est = drivers.estimate_p2(mesh, str(tmp_path), columns=(-1,), recovery=make)
    want = ns.estimate(traj.T)
    col = est["columns"][0]
    assert set(col) >= {"column", "eta", "energy_norm", "relative", "element", "eta2_max", "centroid"}
    assert col["eta"] == pytest.approx(np.sqrt(want["eta2_total"][2]), rel=1e-12)
    assert col["relative"] == pytest.approx(want["relative"][2], rel=1e-12) and 0.0 < col["relative"] < 1.0
    assert col["element"] == want["eta2_argmax"][2]
    for path, cells in ((rep["files"][1], ("von-mises-max", "energy")), (est["files"][0], ("von-mises-max", "energy", "eta2"))):
        assert os.path.basename(path).startswith(("Stress-order2-col-2", "Estimate-order2-col-2"))
        text = open(path).read()
        assert f"CELLS 36 {36 * 11}" in text
        types = text[text.index("CELL_TYPES 36"):].split("\n")[1:37]
        assert set(types) == {"24"}
        v = parse_vtk(path)
        assert v["cells"].shape == (36, 10) and set(cells) <= set(v["cell_data"])
        assert {"sigma-xx", "sigma-xy", "von-mises"} <= set(v["point_data"])
        assert np.allclose(v["point_data"]["sigma-xx"], ns.nodal(el["sigma"][2:3])[0][:, 0], rtol=1e-13, atol=1e-20)
    # the linear writer is unchanged: four-node cells stay type 10
    p = rio.write_vtk_fields(str(tmp_path / "lin.vtk"), mesh.points, mesh.tets, None, {"a": np.zeros(len(mesh.tets))})
    text = open(p).read()
    assert f"CELLS {len(mesh.tets)} {5 * len(mesh.tets)}" in text and set(text[text.index("CELL_TYPES"):].split("\n")[1:7]) == {"10"}
    with pytest.raises(FileNotFoundError, match="dynamics --order 2"):
        drivers.stress_p2(mesh, str(tmp_path / "empty"), recovery=make)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_kernels_use_no_scratch_spill_nothing_and_keep_their_occupancy():
    """One lane per element or node.  The element pass holds the inverse Jacobians of four points and the four parametric
    gradients (76 fp64) like p2_apply_k_kernel and must keep its two waves per SIMD, as must the error pass; the nodal
    pass gets the eight waves of nodal_average_kernel."""
    def table(name):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=" + name],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr
        rows = {}
        for ln in out.stdout.splitlines()[1:]:
            f = ln.split()
            rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
        print(out.stdout)
        return rows

    rows = table("saa_stress_p2.hip")
    for kernel in ("p2_stress_vol_kernel", "p2_stress_node_weight_kernel", "p2_stress_elem_kernel", "p2_stress_nodal_kernel<true>",
                   "p2_stress_nodal_kernel<false>", "p2_stress_error_kernel<true>", "p2_stress_error_kernel<false>"):
        assert any(kernel in k for k in rows), (kernel, rows)
    linear = table("saa_stress.hip")
    nodal_floor = min(r["occ"] for k, r in linear.items() if "nodal_average_kernel" in k)
    for name, r in rows.items():
        assert r["vspill"] == 0 and r["scratch"] == 0 and r["sspill"] == 0, (name, r)
        if "p2_stress_elem_kernel" in name or "p2_stress_error_kernel" in name:
            assert r["occ"] >= 2, (name, r)
        if "p2_stress_nodal_kernel" in name:
            assert r["occ"] >= nodal_floor, (name, r, nodal_floor)
