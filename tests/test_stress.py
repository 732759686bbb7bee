"""Stress recovery without a GPU: the VTK field writer, the file handling of ``drivers stress`` with a NumPy stand-in
for the kernels (on the reference's own two-rank snapshots), its refusals, and the register budget of saa_stress.hip."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from stress_double import NumpyStress, VOIGT, parse_vtk, serial_element_stress, write_tworank_tree

E, NU = 1e6, 0.3


def _lame():
    from synchronization_avoiding_algorithms_amd import fem_setup as fs

    return fs.lame(E, NU)


def test_vtk_fields_round_trip(tmp_path, beam_coarse):
    from synchronization_avoiding_algorithms_amd import results_io as rio

    rng = np.random.default_rng(0)
    n, ne = len(beam_coarse.points), len(beam_coarse.tets)
    pd = {"a": rng.normal(size=n) * 1e-7, "b-x": rng.normal(size=n) * 1e9}
    cd = {"c": rng.normal(size=ne), "d": np.full(ne, np.pi)}
    path = rio.write_vtk_fields(str(tmp_path / "sub" / "f.vtk"), beam_coarse.points, beam_coarse.tets, pd, cd)
    got = parse_vtk(path)
    assert np.array_equal(got["points"], beam_coarse.points) and np.array_equal(got["cells"], beam_coarse.tets)
    assert list(got["point_data"]) == list(pd) and list(got["cell_data"]) == list(cd)
    for name, a in pd.items():
        assert np.array_equal(got["point_data"][name], a), name  # %.17g: exact
    for name, a in cd.items():
        assert np.array_equal(got["cell_data"][name], a), name
    with pytest.raises(ValueError, match="shape"):
        rio.write_vtk_fields(str(tmp_path / "g.vtk"), beam_coarse.points, beam_coarse.tets, {"a": np.zeros(n + 1)})
    only_cells = parse_vtk(rio.write_vtk_fields(str(tmp_path / "h.vtk"), beam_coarse.points, beam_coarse.tets, None, cd))
    assert not only_cells["point_data"] and np.array_equal(only_cells["cell_data"]["c"], cd["c"])


def _driver(mesh, out, **kw):
    from synchronization_avoiding_algorithms_amd import drivers

    return drivers.stress(mesh, str(out), recovery=NumpyStress, **kw)


def test_driver_reproduces_the_serial_element_stress(tmp_path, beam_coarse):
    g = write_tworank_tree(str(tmp_path))
    steps = [int(s) for s in g["steps"]]
    rep = _driver(beam_coarse, tmp_path, columns=range(len(steps)), history=True)
    lmd, mu = _lame()
    want = serial_element_stress(beam_coarse.points, beam_coarse.tets, lmd, mu)
    assert rep["n_ranks"] == 2 and rep["n_saved"] == len(steps) and len(rep["files"]) == len(steps)
    for j, step in enumerate(steps):
        f = parse_vtk(os.path.join(tmp_path, "Results", "Stress", f"Stress-col-{j}.vtk"))
        got = np.stack([f["cell_data"][f"sigma-{c}"] for c in VOIGT], axis=1)
        if step == 1:
            assert not got.any() and rep["columns"][j]["strain_energy"] == 0.0
            continue
        scale = np.abs(want[step]).max()
        assert np.abs(got - want[step]).max() <= 1e-10 * scale, step
        vm = f["cell_data"]["von-mises"]
        assert rep["columns"][j]["von_mises_max"] == vm.max() and rep["columns"][j]["element"] == int(np.argmax(vm))
        e = rep["columns"][j]["element"]
        assert np.allclose(rep["columns"][j]["centroid"], beam_coarse.points[beam_coarse.tets[e]].mean(axis=0))
        assert set(f["point_data"]) == {*(f"displacement-{c}" for c in "xyz"), *(f"sigma-{c}" for c in VOIGT), "von-mises"}
    h = np.load(os.path.join(tmp_path, "Results", "Stress", "history.npz"))
    assert len(h["strain_energy"]) == len(steps)
    assert np.allclose(h["strain_energy"], [c["strain_energy"] for c in rep["columns"]], rtol=1e-14, atol=0)
    assert np.array_equal(h["von_mises_max"], [c["von_mises_max"] for c in rep["columns"]])


def test_driver_modeled_identical_to_truth_gives_zero_differences(tmp_path, beam_coarse):
    g = write_tworank_tree(str(tmp_path))
    snaps = [np.stack([g[f"r{r}_step_{s}"] for s in g["steps"]], axis=1) for r in range(2)]
    write_tworank_tree(str(tmp_path), modeled=snaps)
    rep = _driver(beam_coarse, tmp_path, columns=[-1], modeled=True, vtk=False)
    c = rep["columns"][0]
    assert c["von_mises_rel_l2"] == 0.0 and c["dvm_max"] == 0.0
    assert c["dvm_max_interface"] == 0.0 and c["dvm_max_interior"] == 0.0
    assert c["modeled"] == {k: c[k] for k in ("strain_energy", "von_mises_max", "element", "centroid")}
    assert rep["files"] == []


def test_driver_refuses_inconsistent_trees(tmp_path, beam_coarse):
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
        _driver(beam_coarse, str(tmp_path / "empty"))


def test_numpy_stand_in_energy_is_half_dKd(beam_coarse):
    """The identities the GPU tests hold the kernels to, checked on the stand-in itself."""
    from oracle import fem_oracle as fo

    lmd, mu = _lame()
    d = np.random.default_rng(1).normal(size=3 * len(beam_coarse.points))
    K = fo.assemble_local_stiffness(np.arange(len(beam_coarse.points)), beam_coarse.tets, beam_coarse.points, lmd, mu)
    r = NumpyStress(beam_coarse.points, beam_coarse.tets, lmd, mu).element(d.reshape(1, -1))
    want = 0.5 * d @ (K @ d)
    assert abs(r["energy_total"][0] - want) <= 1e-13 * abs(want)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_stress_kernels_have_no_spills_and_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--file=saa_stress.hip"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        f = ln.split()
        rows[" ".join(f[:-6])] = dict(zip(("sgpr", "vgpr", "sspill", "vspill", "scratch", "occ"), (int(v) for v in f[-6:])))
    assert any("stress_elem_kernel" in k for k in rows) and sum("nodal_average_kernel" in k for k in rows) == 8, rows
    for name, r in rows.items():
        assert r["sspill"] == 0 and r["vspill"] == 0 and r["scratch"] == 0, (name, r)
