"""Finite-strain stress recovery without a GPU: the C entry point's exports and refusals, the NumPy double of
tests/fs_stress_double.py against itself (float64 against longdouble, the identities ``F S = P`` and ``P F^T / J = sigma``,
a rigid motion, the small-strain limit), and ``drivers stress`` / ``estimate --material`` on a NumPy stand-in recovery.

Bars: 1e-12 of the largest entry for float64 against longdouble (measured 9.4e-17 .. 1.2e-15), 1e-15 for the identities in
longdouble (measured 0 .. 2.1e-19), ``1e-12 (lambda + 2 mu) max|H|`` for the rigid motion (measured 1.7e-15 .. 2.5e-14 of that
scale, float64 and longdouble alike: the floor is the rounding of ``u``)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import finite_strain_double as fd
import fs_stress_double as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = fd.lame(fd.E, fd.NU)
NAME = "saa_operator_stress_finite"


# ---- exports and refusals -----------------------------------------------------------------------------------------------------

def test_entry_point_is_exported_declared_and_bound():
    from synchronization_avoiding_algorithms_amd import _lib

    assert _lib.ABI_VERSION == 16 and _lib.load().saa_abi_version() == 16
    assert "saa_stress_fs.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "saa_api.cpp"
    assert hasattr(_lib.load(), NAME)
    header = open(_lib.HEADER).read()
    assert "#define SAA_STRESS_PK2 0" in header and "#define SAA_STRESS_CAUCHY 1" in header
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert decl, "not declared in include/saa_hip.h"
    n_declared = len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(","))
    api = open(os.path.join(ROOT, "synchronization_avoiding_algorithms_amd", "csrc", "saa_api.cpp")).read()
    n_defined = len(re.search(r"\bint " + NAME + r"\(([^)]*)\) \{", api).group(1).split(","))
    assert n_declared == n_defined == len(_lib.SIGNATURES[NAME][1]) == 18


def test_refusals_need_no_device():
    """Every refusal that comes before the handle is read, with a handle that is never dereferenced."""
    from synchronization_avoiding_algorithms_amd import _lib

    lib = _lib.load()
    fake = C.c_void_p(8)

    def call(h, material, measure, m, x=fake):
        return lib.saa_operator_stress_finite(h, material, measure, m, x, 0, None, 0, None, 0, None, 0, None, 0, None, None, None,
                                              None)

    for material in (0, 3, -1):                                         # the linear material is refused too
        assert call(fake, material, 0, 1) == _lib.SAA_E_ARG
        assert lib.saa_last_error().decode().startswith(f"{NAME}: material {material} ")
    for measure in (2, -1):
        assert call(fake, 1, measure, 1) == _lib.SAA_E_ARG
        assert lib.saa_last_error().decode().startswith(f"{NAME}: measure {measure} ")
    assert call(None, 3, 7, 1) == _lib.SAA_E_ARG and "material 3" in lib.saa_last_error().decode()   # material first
    assert call(None, 1, 7, 1) == _lib.SAA_E_ARG and "measure 7" in lib.saa_last_error().decode()    # then the measure
    assert call(None, 2, 1, 1) == _lib.SAA_E_ARG and lib.saa_last_error().decode() == NAME + ": null handle"
    assert call(fake, 2, 1, 1, x=None) == _lib.SAA_E_ARG and lib.saa_last_error().decode() == NAME + ": null displacement x_dev"
    for m in (0, 17, -3):
        assert call(fake, 1, 0, m) == _lib.SAA_E_ARG
        assert lib.saa_last_error().decode().startswith(NAME + ": m = %d columns" % m)


def test_python_layer_refuses_unknown_names_before_any_launch():
    from synchronization_avoiding_algorithms_amd.stress import _Recovery

    assert _Recovery._finite("linear", "cauchy") is None and _Recovery._finite("linear", "pk2") is None
    assert _Recovery._finite("svk", "pk2") == (1, 0, "pk2") and _Recovery._finite("neo-hookean", "cauchy") == (2, 1, "cauchy")
    with pytest.raises(ValueError, match="unknown measure"):
        _Recovery._finite("svk", "kirchhoff")
    with pytest.raises(ValueError, match="unknown material"):
        _Recovery._finite("mooney", "pk2")


# ---- the double ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def doubles():
    """name -> (points, longdouble double, float64 double, the ``max|H| = 0.3`` field of seed 40 + k)."""
    out = {}
    for k, name in enumerate(fd.MESHES):
        pts, cells, _ = fd.mesh(name)
        ld = sd.FsStress(pts, cells, LMD, MU)
        u, det, hmax = fd.scale_to_strain(ld.fs, fd.smooth_random_field(pts, 40 + k))
        assert det >= 0.2 and hmax >= 0.1
        out[name] = (pts, ld, sd.FsStress(pts, cells, LMD, MU, T=np.float64), u)
    return out


def _rel(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("measure", sd.MEASURES)
@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_double_float64_against_longdouble(doubles, name, material, measure):
    _, ld, f64, u = doubles[name]
    a, b = ld.recover(u, material, measure), f64.recover(u, material, measure)
    errs = {k: _rel(b[k], a[k]) for k in ("stress", "von_mises", "det_f", "energy")}
    errs["energy_total"] = abs(float(b["energy_total"] - a["energy_total"]) / float(a["energy_total"]))
    print(name, material, measure, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12
    assert a["n_inverted"] == b["n_inverted"] == 0 and a["von_mises_argmax"] == b["von_mises_argmax"]


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_double_measures_agree_with_the_first_piola_stress(doubles, name, material):
    """``F S = P`` of ``FiniteStrain.stress`` and ``P F^T / J = sigma``, in longdouble."""
    _, ld, _, u = doubles[name]
    P, F = ld.first_piola(u, material), ld.fs._f(ld.fs.gradient(u))
    pk2, cauchy = ld.recover(u, material, "pk2"), ld.recover(u, material, "cauchy")
    S, sg, J = sd.tensor(pk2["stress"]), sd.tensor(cauchy["stress"]), cauchy["det_f"]
    FS, PF = np.zeros_like(P), np.zeros_like(P)
    for i in range(3):
        for k in range(3):
            for l in range(3):
                FS[..., i, k] = FS[..., i, k] + F[..., i, l] * S[..., l, k]
                PF[..., i, k] = PF[..., i, k] + P[..., i, l] * F[..., k, l]
    e1, e2 = _rel(FS, P), _rel(PF / J[..., None, None], sg)
    print(name, material, f"F S = P {e1:.2e}, P F^T / J = sigma {e2:.2e}")
    assert e1 <= 1e-15 and e2 <= 1e-15


@pytest.mark.parametrize("T", (np.longdouble, np.float64))
@pytest.mark.parametrize("name", fd.MESHES)
def test_double_rigid_motion_gives_no_stress(doubles, name, T):
    pts, ld, f64, _ = doubles[name]
    dbl = ld if T is np.longdouble else f64
    u = np.asarray(fd.rigid_motion(pts, 0.5), dtype=np.float64)
    scale = float(LMD + 2 * MU) * float(np.abs(ld.fs.gradient(u)).max())
    lin = float(np.abs(dbl.linear_stress(u)).max())
    for material in fd.MATERIALS:
        for measure in sd.MEASURES:
            r = dbl.recover(u, material, measure)
            worst = float(np.abs(r["stress"]).max())
            print(name, T.__name__, material, measure, f"max|stress| / scale {worst / scale:.2e}; linear {lin:.3e}")
            assert worst <= 1e-12 * scale and float(r["von_mises_max"]) <= 1e-12 * scale and r["n_inverted"] == 0
    assert lin > 1e5                                                    # what the linear entries report for the same x


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_double_small_strain_limit(doubles, name, material):
    """``|sigma_fs - sigma_linear| / |sigma_linear|`` is first order in the strain: it halves with it.  Three halvings from
    ``max|H| = 1e-3`` in longdouble; measured ratios 1.99986 .. 2.00004."""
    _, ld, _, u = doubles[name]
    u = u * (1e-3 / 0.3)
    for measure in sd.MEASURES:
        rel = []
        for k in range(4):
            uk = u * 0.5 ** k
            lin = ld.linear_stress(uk)
            d = ld.recover(uk, material, measure)["stress"] - lin
            rel.append(float(np.sqrt((d * d).sum() / (lin * lin).sum())))
        ratios = [rel[k] / rel[k + 1] for k in range(3)]
        print(name, material, measure, rel, ratios)
        assert all(abs(r - 2.0) <= 1e-3 for r in ratios)


def test_double_inversion_rule(doubles):
    """An inverted element is 0 in stress, von Mises and energy and out of the total and the maximum, except under svk with
    pk2, which does not look at ``J``."""
    pts, ld, f64, u = doubles["beam36"]
    _, bad, elements = fd.inversion_state(f64.fs, pts, 0.1 * u)
    for material, measure in (("neo_hookean", "pk2"), ("neo_hookean", "cauchy"), ("svk", "cauchy")):
        r = f64.recover(bad, material, measure)
        assert sorted(np.nonzero(r["inverted"])[0]) == sorted(elements) and r["n_inverted"] == len(elements)
        assert not r["stress"][elements].any() and not r["von_mises"][elements].any() and not r["energy"][elements].any()
        assert (r["det_f"][elements].min(axis=1) <= 0).all()
        assert r["von_mises_argmax"] // f64.nq not in elements and np.isfinite(float(r["energy_total"]))
    r = f64.recover(bad, "svk", "pk2")
    assert r["n_inverted"] == 0 and r["stress"][elements].any()
    r = f64.recover(np.full_like(bad, np.nan), "neo_hookean", "cauchy")
    assert r["n_inverted"] == f64.n_elems and r["von_mises_argmax"] == -1 and float(r["energy_total"]) == 0.0


# ---- the drivers on a stand-in recovery -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", (1, 2))
def test_drivers_with_a_material_on_the_double(tmp_path, order):
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic

    mesh = structured_beam(1, length=6.0)
    q = to_quadratic(mesh) if order == 2 else mesh
    cells = np.asarray(q.tets10 if order == 2 else q.tets, dtype=np.int64)
    f64 = sd.FsStress(q.points, cells, LMD, MU, T=np.float64)
    u, _, _ = fd.scale_to_strain(f64.fs, fd.smooth_random_field(q.points, 7), target=0.2)
    traj = np.stack([0.0 * u, 0.5 * u, u], axis=1)
    rio.save_displacement(str(tmp_path / drivers.PATHS["dynamics"].format(p=order)), traj)
    make = sd.standin(order)

    rep = drivers.stress_finite(mesh, str(tmp_path), columns=(1, -1), material="svk", measure="cauchy", order=order, history=True,
                                recovery=make)
    want = f64.recover(u, "svk", "cauchy")
    json.dumps(rep)
    assert rep["order"] == order and rep["material"] == "svk" and rep["measure"] == "cauchy" and rep["n_saved"] == 3
    last = rep["columns"][1]
    linear_keys = {"column", "strain_energy", "von_mises_max", "element", "centroid"} | ({"gauss_point", "position"} if order == 2 else set())
    assert set(last) == linear_keys | {"material", "measure", "n_inverted", "min_det_f"}
    assert last["column"] == 2 and last["n_inverted"] == 0 and last["material"] == "svk" and last["measure"] == "cauchy"
    assert last["strain_energy"] == pytest.approx(float(want["energy_total"]), rel=1e-13)
    assert last["von_mises_max"] == pytest.approx(float(want["von_mises_max"]), rel=1e-13)
    assert last["min_det_f"] == pytest.approx(float(want["det_f"].min()), rel=1e-13)
    assert last["element"] == want["von_mises_argmax"] // f64.nq
    files = [os.path.relpath(f, str(tmp_path)) for f in rep["files"]]
    assert files == [f"Results/Stress/Stress-svk-order{order}-col-{j}.vtk" for j in (1, 2)]
    assert os.path.relpath(rep["history"], str(tmp_path)) == f"Results/Stress/history-svk-order{order}.npz"
    with np.load(rep["history"]) as h:
        assert set(h.files) == {"columns", "strain_energy", "von_mises_max", "von_mises_element", "von_mises_gauss_point",
                                "n_inverted", "min_det_f"}
        assert h["strain_energy"][2] == pytest.approx(last["strain_energy"], rel=1e-13) and not h["n_inverted"].any()
    text = open(rep["files"][1]).read()
    point, cell = text[text.index("POINT_DATA"):text.index("CELL_DATA")], text[text.index("CELL_DATA"):]
    for name in ["displacement-x", "displacement-y", "displacement-z", "von-mises"] + ["sigma-" + c for c in ("xx", "yy", "zz", "yz", "xz", "xy")]:
        assert f"SCALARS {name} double" in point, name
    assert [ln.split()[1] for ln in cell.splitlines() if ln.startswith("SCALARS")] == ["von-mises-max", "energy", "det-f-min"]

    est = drivers.estimate_finite(mesh, str(tmp_path), columns=(-1,), material="svk", order=order, recovery=make)
    json.dumps(est)
    col = est["columns"][0]
    assert est["measure"] == "pk2" and col["measure"] == "pk2" and col["n_inverted"] == 0
    assert set(col) == {"column", "eta", "energy_norm", "relative", "element", "eta2_max", "centroid", "material", "measure",
                        "n_inverted", "min_det_f"}
    assert col["energy_norm"] == pytest.approx(float(np.sqrt(2 * want["energy_total"])), rel=1e-13) and 0 < col["relative"] < 1
    assert [os.path.relpath(f, str(tmp_path)) for f in est["files"]] == [f"Results/Stress/Estimate-svk-order{order}-col-2.vtk"]
    cell = open(est["files"][0]).read()
    cell = cell[cell.index("CELL_DATA"):]
    assert [ln.split()[1] for ln in cell.splitlines() if ln.startswith("SCALARS")] == ["von-mises-max", "energy", "det-f-min", "eta2"]
    with pytest.raises(ValueError, match="linear material has"):
        drivers.stress_finite(mesh, str(tmp_path), material="linear", order=order, recovery=make)
    with pytest.raises(FileNotFoundError, match=f"dynamics --order {order}"):
        drivers.stress_finite(mesh, str(tmp_path / "empty"), material="svk", order=order, recovery=make)


def test_cli_refuses_modeled_and_linear_changes_nothing(tmp_path, monkeypatch, capsys):
    """``--material svk --modeled`` is refused by name; ``--material linear --measure pk2`` gives the report and the files,
    byte for byte, of a run that names neither option (the stand-in takes the place of the GPU recovery)."""
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic

    for command in ("stress", "estimate"):
        with pytest.raises(SystemExit):
            drivers.main([command, "--synthetic", "1", "--material", "svk", "--modeled"])
        assert "no modelled finite-strain run" in capsys.readouterr().err
    monkeypatch.setattr(drivers, "_device_recovery", lambda device=0, order=1: sd.standin(order))
    monkeypatch.setattr(drivers, "_dist_env", lambda: (0, 1, 0))
    q = to_quadratic(structured_beam(1))
    u = 1e-3 * fd.smooth_random_field(q.points, 3)
    outs = {}
    for tag, extra in (("plain", []), ("named", ["--material", "linear", "--measure", "pk2"])):
        where = tmp_path / tag
        rio.save_displacement(str(where / drivers.PATHS["dynamics"].format(p=2)), np.stack([0.5 * u, u], axis=1))
        reports = []
        for command in (["stress", "--history"], ["estimate"]):
            drivers.main([*command, "--synthetic", "1", "--order", "2", "--out", str(where), *extra])
            reports.append(capsys.readouterr().out.replace(str(where), "OUT"))
        files = {}
        for base, _, names in os.walk(str(where / "Results" / "Stress")):
            for n in names:
                files[n] = open(os.path.join(base, n), "rb").read()
        outs[tag] = (reports, files)
    assert outs["plain"][0] == outs["named"][0]
    assert sorted(outs["plain"][1]) == sorted(outs["named"][1]) == ["Estimate-order2-col-1.vtk", "Stress-order2-col-1.vtk",
                                                                     "history-order2.npz"]
    for n, data in outs["plain"][1].items():
        if n.endswith(".vtk"):
            assert data == outs["named"][1][n], n
