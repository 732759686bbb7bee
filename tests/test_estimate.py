"""The stress error estimate without a GPU: the conditions that the Zienkiewicz-Zhu definition itself meets, asserted on
the NumPy double (a quadratic field whose true error is known in closed form: asymptotic exactness on the lattice
interior, global effectivity, first-order convergence, the patch test), the file handling of ``drivers estimate`` with the
double standing in for the kernels on the reference's two-rank snapshots, its refusals, and the register budget of the
error kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from estimate_double import NumpyEstimate, interior_elements, quadratic_field
from stress_double import parse_vtk, write_tworank_tree

E, NU = 1e6, 0.3
KERNEL_FILE = "saa_stress.hip"  # holds stress_error_kernel


def _lame():
    from synchronization_avoiding_algorithms_amd import fem_setup as fs

    return fs.lame(E, NU)


def _mesh(family, n):
    from synchronization_avoiding_algorithms_amd import mesh

    return getattr(mesh, family)(n)


@pytest.fixture(scope="module")
def quadratic():
    """(family, n) -> estimate and true error of the quadratic field on that mesh."""
    lmd, mu = _lame()
    out = {}
    for family in ("structured_beam", "delaunay_beam"):
        for n in (4, 8):
            m = _mesh(family, n)
            ne = NumpyEstimate(m.points, m.tets, lmd, mu)
            u, exact = quadratic_field(m.points, ne.D)
            est = ne.estimate(u)
            sig = ne.element(u.reshape(1, -1))["sigma"][0]
            # the exact stress is linear: its nodal interpolant is the stress itself, so this is the true error
            true = ne.error(sig, nodal=exact)
            out[family, n] = dict(est=est, true=true, interior=interior_elements(m.points, m.tets))
    return out


def test_affine_field_has_no_estimated_error():
    lmd, mu = _lame()
    rng = np.random.default_rng(7)
    B, b = rng.normal(size=(3, 3)), rng.normal(size=3)
    for family in ("structured_beam", "delaunay_beam"):
        m = _mesh(family, 4)
        r = NumpyEstimate(m.points, m.tets, lmd, mu).estimate((m.points @ B.T + b).reshape(-1))
        print(family, "eta2_total / (2 energy_total) =", r["eta2_total"] / (2 * r["energy_total"]))
        assert r["energy_total"] > 0 and r["eta2_total"] <= 1e-22 * 2 * r["energy_total"], family
        assert r["relative"] <= 1e-11


def test_interior_effectivity_is_one_on_the_lattice(quadratic):
    q = quadratic["structured_beam", 4]
    inner = q["interior"]
    assert inner.any() and not inner.all()
    theta = np.sqrt(q["est"]["eta2"][inner].sum() / q["true"]["eta2"][inner].sum())
    print("interior theta - 1 =", theta - 1)
    assert abs(theta - 1) <= 1e-10


def test_global_effectivity_within_five_percent(quadratic):
    for family in ("structured_beam", "delaunay_beam"):
        q = quadratic[family, 4]
        theta = np.sqrt(q["est"]["eta2_total"] / q["true"]["eta2_total"])
        print(family, "theta =", theta, "eta =", np.sqrt(q["est"]["eta2_total"]))
        assert 0.95 <= theta <= 1.05, family


def test_estimate_halves_with_the_mesh_size(quadratic):
    for family in ("structured_beam", "delaunay_beam"):
        ratio = np.sqrt(quadratic[family, 4]["est"]["eta2_total"] / quadratic[family, 8]["est"]["eta2_total"])
        print(family, "eta(4) / eta(8) =", ratio)
        assert 1.9 <= ratio <= 2.1, family


def test_double_closed_form_and_element_form(beam_coarse):
    """The double's Gauss rule against the closed form of the definition, and the element form against a plain sum."""
    lmd, mu = _lame()
    ne = NumpyEstimate(beam_coarse.points, beam_coarse.tets, lmd, mu)
    rng = np.random.default_rng(2)
    S, N, O = (rng.normal(size=(2, k, 6)) for k in (len(beam_coarse.tets), len(beam_coarse.points), len(beam_coarse.tets)))
    d = N[:, ne.cells] - S[:, :, None, :]
    s = d.sum(axis=2)
    want = ne.vol / 20.0 * (np.einsum("mec,cd,med->me", s, ne.C, s) + np.einsum("meac,cd,mead->me", d, ne.C, d))
    got = ne.error(S, nodal=N)
    assert np.abs(got["eta2"] - want).max() <= 1e-13 * want.max()
    assert np.array_equal(got["eta2_argmax"], want.argmax(axis=1))
    # a nodal field that is the same constant at the four vertices is the element form
    el = ne.error(S, other=O)
    dd = O - S
    assert np.allclose(el["eta2"], ne.vol * np.einsum("mec,cd,med->me", dd, ne.C, dd), rtol=1e-13, atol=0)
    one = ne.error(S[1], other=O[1])
    assert np.array_equal(one["eta2"], el["eta2"][1]) and one["eta2_total"] == el["eta2_total"][1]
    with pytest.raises(ValueError, match="exactly one"):
        ne.error(S, nodal=N, other=O)
    with pytest.raises(ValueError, match="exactly one"):
        ne.error(S)


def _driver(mesh, out, **kw):
    from synchronization_avoiding_algorithms_amd import drivers

    return drivers.estimate(mesh, str(out), recovery=NumpyEstimate, **kw)


def _assembled_sigma(beam_coarse, g, snaps, col):
    """Element stress of the whole mesh, each element from the rank that owns it."""
    lmd, mu = _lame()
    sig = np.zeros((len(beam_coarse.tets), 6))
    W = 0.0
    for r in range(2):
        nodes, elems = g[f"r{r}_local_nodes"], g[f"r{r}_local_elements"]
        pos = np.full(len(beam_coarse.points), -1)
        pos[nodes] = np.arange(len(nodes))
        res = NumpyEstimate(beam_coarse.points[nodes], pos[beam_coarse.tets[elems]], lmd, mu).element(snaps[r][:, col][None])
        sig[elems] = res["sigma"][0]
        W += res["energy_total"][0]
    return sig, W


def test_driver_on_the_two_rank_tree(tmp_path, beam_coarse):
    g = write_tworank_tree(str(tmp_path))
    steps = [int(s) for s in g["steps"]]
    snaps = [np.stack([g[f"r{r}_step_{s}"] for s in steps], axis=1) for r in range(2)]
    rep = _driver(beam_coarse, tmp_path, columns=range(len(steps)))
    assert rep["n_ranks"] == 2 and rep["n_saved"] == len(steps) and len(rep["files"]) == len(steps)
    assert rep["n_elems"] == len(beam_coarse.tets) and rep["n_nodes"] == len(beam_coarse.points)
    lmd, mu = _lame()
    whole = NumpyEstimate(beam_coarse.points, beam_coarse.tets, lmd, mu)
    for j, step in enumerate(steps):
        c = rep["columns"][j]
        assert c["column"] == j and "modeled" not in c and "model_error" not in c
        sig, W = _assembled_sigma(beam_coarse, g, snaps, j)
        want = whole.error(sig, nodal=whole.nodal(sig[None])[0])
        f = parse_vtk(os.path.join(tmp_path, "Results", "Stress", f"Estimate-col-{j}.vtk"))
        assert rep["files"][j].endswith(f"Estimate-col-{j}.vtk")
        assert set(f["cell_data"]) == {"eta2", "error-density"} and not f["point_data"]
        assert np.array_equal(f["points"], beam_coarse.points) and np.array_equal(f["cells"], beam_coarse.tets)
        assert np.array_equal(f["cell_data"]["eta2"], want["eta2"])  # %.17g: exact
        assert np.allclose(f["cell_data"]["error-density"] * whole.vol, want["eta2"], rtol=1e-14, atol=0)
        if step == 1:  # the first snapshot is the zero state
            assert c["eta"] == 0.0 and c["energy_norm"] == 0.0 and c["relative"] == 0.0
            continue
        assert c["eta"] == np.sqrt(want["eta2_total"]) and c["energy_norm"] == np.sqrt(2 * W)
        assert abs(c["relative"] - c["eta"] / np.hypot(c["eta"], c["energy_norm"])) <= 1e-15
        assert 0 < c["relative"] < 1
        e = c["element"]
        assert e == int(np.argmax(want["eta2"])) and c["eta2_max"] == want["eta2"][e]
        assert np.allclose(c["centroid"], beam_coarse.points[beam_coarse.tets[e]].mean(axis=0))


def test_driver_modeled_splits_add_up_and_identical_runs_give_zero(tmp_path, beam_coarse):
    g = write_tworank_tree(str(tmp_path))
    steps = [int(s) for s in g["steps"]]
    snaps = [np.stack([g[f"r{r}_step_{s}"] for s in steps], axis=1) for r in range(2)]
    rng = np.random.default_rng(5)
    modeled = [s * (1.0 + 1e-3 * rng.normal(size=s.shape)) for s in snaps]
    write_tworank_tree(str(tmp_path), modeled=modeled)
    rep = _driver(beam_coarse, tmp_path, columns=[-1, 1], modeled=True)
    iface = np.isin(beam_coarse.tets, g["Global_shared"]).any(axis=1)
    lmd, mu = _lame()
    whole = NumpyEstimate(beam_coarse.points, beam_coarse.tets, lmd, mu)
    assert [c["column"] for c in rep["columns"]] == [len(steps) - 1, 1]
    for c in rep["columns"]:
        j = c["column"]
        st, _ = _assembled_sigma(beam_coarse, g, snaps, j)
        sm, Wm = _assembled_sigma(beam_coarse, g, modeled, j)
        me = whole.error(sm, other=st)
        zt = whole.error(st, nodal=whole.nodal(st[None])[0])
        zm = whole.error(sm, nodal=whole.nodal(sm[None])[0])
        assert c["n_interface"] == int(iface.sum()) and c["n_interface"] + c["n_interior"] == len(iface)
        assert 0 < c["n_interface"] < len(iface)
        assert abs(c["eta2_interface"] + c["eta2_interior"] - c["eta"] ** 2) <= 1e-12 * c["eta"] ** 2
        assert abs(c["model_error2_interface"] + c["model_error2_interior"] - c["model_error"] ** 2) <= 1e-12 * c["model_error"] ** 2
        assert c["model_error"] == np.sqrt(me["eta2_total"]) and c["model_error"] > 0
        assert c["model_error2_interface"] == me["eta2"][iface].sum() and c["eta2_interior"] == zt["eta2"][~iface].sum()
        assert c["model_over_discretisation"] == c["model_error"] / c["eta"]
        above = me["eta2"] > zt["eta2"]
        assert c["n_model_above_eta_interface"] == int((above & iface).sum())
        assert c["n_model_above_eta_interior"] == int((above & ~iface).sum())
        assert c["modeled"]["eta"] == np.sqrt(zm["eta2_total"]) and c["modeled"]["energy_norm"] == np.sqrt(2 * Wm)
        assert c["modeled"]["element"] == int(np.argmax(zm["eta2"]))
        f = parse_vtk(os.path.join(tmp_path, "Results", "Stress", f"Estimate-col-{j}.vtk"))
        assert list(f["cell_data"]) == ["eta2", "error-density", "model-error2"]
        assert np.array_equal(f["cell_data"]["model-error2"], me["eta2"]) and np.array_equal(f["cell_data"]["eta2"], zt["eta2"])
    # a modelled tree identical to the truth
    write_tworank_tree(str(tmp_path), modeled=snaps)
    same = _driver(beam_coarse, tmp_path, columns=[-1], modeled=True, vtk=False)
    c = same["columns"][0]
    assert same["files"] == []
    assert c["model_error"] == 0.0 and c["model_over_discretisation"] == 0.0
    assert c["model_error2_interface"] == 0.0 and c["model_error2_interior"] == 0.0
    assert c["n_model_above_eta_interface"] == 0 and c["n_model_above_eta_interior"] == 0
    assert c["modeled"] == {k: c[k] for k in ("eta", "energy_norm", "relative", "element", "eta2_max", "centroid")}


def test_driver_refuses_inconsistent_trees(tmp_path, beam_coarse):
    """The trees that ``drivers stress`` rejects (tests/test_stress.py), rejected here with the same messages."""
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.drivers import PATHS

    def tree(name):
        out = tmp_path / name
        g = write_tworank_tree(str(out))
        return str(out), g

    out, g = tree("missing")
    rio.save_int_list(os.path.join(out, PATHS["elements"].format(r=1)), g["r1_local_elements"][1:])
    with pytest.raises(ValueError, match="owned by no rank"):
        _driver(beam_coarse, out)
    out, g = tree("twice")
    rio.save_int_list(os.path.join(out, PATHS["elements"].format(r=1)),
                      np.concatenate([g["r1_local_elements"], g["r0_local_elements"][:1]]))
    with pytest.raises(ValueError, match="owned by ranks 0 and 1"):
        _driver(beam_coarse, out)
    out, g = tree("rows")
    rio.save_displacement(os.path.join(out, PATHS["truth"].format(r=0)), np.zeros((3 * len(g["r0_local_nodes"]) - 3, 5)))
    with pytest.raises(ValueError, match="rows, expected"):
        _driver(beam_coarse, out)
    out, g = tree("columns")
    with pytest.raises(ValueError, match="out of range"):
        _driver(beam_coarse, out, columns=[5])
    with pytest.raises(FileNotFoundError):
        _driver(beam_coarse, out, modeled=True)  # no Modeled_Local-rank-0.hdf5
    with pytest.raises(FileNotFoundError):
        _driver(beam_coarse, str(tmp_path / "empty"))
    assert not os.path.exists(os.path.join(out, "Results", "Stress"))  # refused before anything is written


def test_cli_knows_the_command_and_the_binding_the_entry_point():
    from synchronization_avoiding_algorithms_amd import _lib, drivers
    from synchronization_avoiding_algorithms_amd.stress import StressRecovery

    assert "saa_operator_stress_error" in _lib.SIGNATURES and _lib.ABI_VERSION >= 14
    assert all(hasattr(StressRecovery, k) for k in ("error_raw", "error", "estimate"))
    assert drivers.PATHS["estimate_vtk"] == "Results/Stress/Estimate-col-{j}.vtk"
    with pytest.raises(SystemExit):
        drivers.main(["estimate", "--help"])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_error_kernel_has_no_spills_and_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), f"--file={KERNEL_FILE}"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
    mine = {k: r for k, r in rows.items() if "stress_error_kernel" in k}
    assert len(mine) == 2, rows  # the nodal and the element form
    for name, r in mine.items():
        assert r["sspill"] == 0 and r["vspill"] == 0 and r["scratch"] == 0, (name, r)
