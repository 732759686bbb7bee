"""The reports and files of the eight recovery drivers, pinned: ``drivers.stress`` and ``estimate`` on the two-rank tree
with a modelled run, ``stress_p2`` and ``estimate_p2``, ``stress_finite`` and ``estimate_finite`` of either order, all on
their NumPy stand-ins, against ``golden/recovery_reports.json``.  Every report's keys in order (nested ones too), strings
and integers exactly, file names relative to the output directory, the array names of each history file and the
``SCALARS`` names of each VTK file in order.  Floats at ``rel = 1e-12`` (the bound tests/test_p2_stress.py holds between a
driver and its double; it is there to catch a swapped field on another machine), an exact 0 exactly.  Needs neither the GPU
nor the built library.

``python tests/test_recovery_reports.py --write`` regenerates the fixture."""
import json
import os
import sys

import numpy as np

from conftest import GOLDEN, load_golden

import finite_strain_double as fd
import fs_stress_double as sd
import p2_stress_double as psd
from estimate_double import NumpyEstimate
from stress_double import NumpyStress, write_tworank_tree

FIXTURE = os.path.join(GOLDEN, "recovery_reports.json")
LMD, MU = fd.lame(fd.E, fd.NU)
REL = 1e-12


def _vtk_names(path):
    """``SCALARS`` names of a legacy VTK file, in order: point data, cell data."""
    names, section = {"point_data": [], "cell_data": []}, None
    with open(path) as fh:
        for ln in fh:
            if ln.startswith(("POINT_DATA", "CELL_DATA")):
                section = ln.split()[0].lower()
            elif ln.startswith("SCALARS"):
                names[section].append(ln.split()[1])
    return names


def _record(report, out):
    """The report with its paths relative to ``out``, the array names of its history file and the names in its VTK files."""
    rec = {"report": {**report, "files": [os.path.relpath(f, out) for f in report["files"]]}}
    if report.get("history"):
        rec["report"]["history"] = os.path.relpath(report["history"], out)
        with np.load(report["history"]) as h:
            rec["history_arrays"] = list(h.files)
    rec["vtk"] = {os.path.relpath(f, out): _vtk_names(f) for f in report["files"]}
    return json.loads(json.dumps(rec))      # what the CLI prints, read back: tuples are lists, the key order stays


def run_all(root):
    """The eight calls under ``root``: name -> :func:`_record`."""
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.mesh import Mesh, structured_beam, to_quadratic

    out = {}
    # the two-rank tree of tests/test_stress.py and tests/test_estimate.py with a modelled run; column 0 is the zero state
    g = load_golden("beam_coarse_mesh.npz")
    coarse = Mesh(g["points"], {"tetra": g["tetra"], "triangle": g["triangle"]})
    tree = os.path.join(root, "tree")
    t = write_tworank_tree(tree)
    snaps = [np.stack([t[f"r{r}_step_{s}"] for s in t["steps"]], axis=1) for r in range(2)]
    rng = np.random.default_rng(5)
    write_tworank_tree(tree, modeled=[s * (1.0 + 1e-3 * rng.normal(size=s.shape)) for s in snaps])
    out["stress"] = _record(drivers.stress(coarse, tree, columns=[-1, 1], modeled=True, history=True, recovery=NumpyStress), tree)
    out["estimate"] = _record(drivers.estimate(coarse, tree, columns=[-1, 1], modeled=True, recovery=NumpyEstimate), tree)

    mesh = structured_beam(1, length=6.0)
    quad = to_quadratic(mesh)
    # quadratic tetrahedra, linear material: the cubic field of tests/test_p2_stress.py, no column at rest
    where = os.path.join(root, "p2")
    u, _ = psd.cubic_field(quad.points, psd.NumpyQuadraticStress(quad.points, quad.tets10, LMD, MU).D)
    rio.save_displacement(os.path.join(where, drivers.PATHS["dynamics"].format(p=2)), np.stack([0.25 * u, 0.5 * u, u], axis=1))
    out["stress_p2"] = _record(drivers.stress_p2(mesh, where, columns=(1, -1), history=True,
                                                 recovery=psd.NumpyQuadraticStress), where)
    out["estimate_p2"] = _record(drivers.estimate_p2(mesh, where, columns=(1, -1), recovery=psd.NumpyQuadraticStress), where)

    # finite strain: the smooth field of tests/test_fs_stress.py at max|H| = 0.2, no column at rest
    for order in (1, 2):
        q = quad if order == 2 else mesh
        cells = np.asarray(q.tets10 if order == 2 else q.tets, dtype=np.int64)
        f64 = sd.FsStress(q.points, cells, LMD, MU, T=np.float64)
        u, _, _ = fd.scale_to_strain(f64.fs, fd.smooth_random_field(q.points, 7), target=0.2)
        where = os.path.join(root, f"fs{order}")
        rio.save_displacement(os.path.join(where, drivers.PATHS["dynamics"].format(p=order)),
                              np.stack([0.25 * u, 0.5 * u, u], axis=1))
        make = sd.standin(order)
        out[f"stress_finite_order{order}"] = _record(
            drivers.stress_finite(mesh, where, columns=(1, -1), material="svk", measure="cauchy", order=order, history=True,
                                  recovery=make), where)
        out[f"estimate_finite_order{order}"] = _record(
            drivers.estimate_finite(mesh, where, columns=(1, -1), material="neo_hookean", order=order, recovery=make), where)
    return out


def _compare(got, want, where):
    assert type(got) is type(want), f"{where}: {type(got).__name__}, expected {type(want).__name__}"
    if isinstance(want, dict):
        assert list(got) == list(want), f"{where}: keys {list(got)}, expected {list(want)}"
        for k in want:
            _compare(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), f"{where}: {len(got)} entries, expected {len(want)}"
        for i, (a, b) in enumerate(zip(got, want)):
            _compare(a, b, f"{where}[{i}]")
    elif isinstance(want, float) and want != 0.0:
        assert abs(got - want) <= REL * abs(want), f"{where}: {got!r}, expected {want!r}"
    else:                                       # strings, integers, booleans, None and the exact 0.0
        assert got == want, f"{where}: {got!r}, expected {want!r}"


def test_reports_files_and_array_names_are_those_of_the_fixture(tmp_path):
    with open(FIXTURE) as fh:
        want = json.load(fh)
    got = run_all(str(tmp_path))
    assert list(got) == list(want) and len(got) == 8
    for name in want:
        _compare(got[name], want[name], name)
    # what the fixture must hold for the comparison to mean something
    for name, rec in want.items():
        assert len(rec["report"]["columns"]) == 2 and len(rec["vtk"]) == len(rec["report"]["files"]) >= 2, name
        assert ("history_arrays" in rec) == name.startswith("stress"), name
        assert all(v["cell_data"] for v in rec["vtk"].values()), name


if __name__ == "__main__":
    import tempfile

    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_recovery_reports.py --write")
    with tempfile.TemporaryDirectory() as tmp:
        result = run_all(tmp)
    with open(FIXTURE, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
