"""Stress recovery on the MI355X: element stress / von Mises / strain energy against the oracle's B and D, the patch test,
vertex-order independence, the energy of recorded trajectories of the product's step kernels, strides, batching,
validation, repeatability, the nodal average, and the ``drivers stress`` command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import fem_oracle as fo
from stress_double import NumpyStress, VOIGT, parse_vtk, serial_element_stress, von_mises, write_tworank_tree
from test_modal import _meshes

pytestmark = pytest.mark.gpu

LMD, MU = fo.lame(1e6, 0.3)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def meshes():
    return _meshes()


def _rec(points, cells):
    from synchronization_avoiding_algorithms_amd.stress import StressRecovery

    return StressRecovery(points, cells, LMD, MU, device=0)


def _t(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def test_element_fields_match_the_oracle(meshes):
    for name, m in meshes.items():
        rng = np.random.default_rng(3)
        X = rng.normal(size=(3, 3 * len(m.points)))
        want = NumpyStress(m.points, m.tets, LMD, MU).element(X)
        with _rec(m.points, m.tets) as rec:
            got = {k: v.cpu().numpy() for k, v in rec.element(_t(X)).items()}
        smax = np.abs(want["sigma"]).max()
        assert np.abs(got["sigma"] - want["sigma"]).max() <= 1e-12 * smax, name
        assert np.abs(got["von_mises"] - want["von_mises"]).max() <= 1e-12 * smax, name
        Ke = fo.element_stiffness(m.points[m.tets], LMD, MU)
        K = fo.assemble_local_stiffness(np.arange(len(m.points)), m.tets, m.points, LMD, MU)
        for j in range(3):
            ue = X[j].reshape(-1, 3)[m.tets].reshape(len(m.tets), 12)
            We = 0.5 * np.einsum("ei,eij,ej->e", ue, Ke, ue)
            assert np.abs(got["energy"][j] - We).max() <= 1e-12 * np.abs(We).max(), name
            dKd = 0.5 * X[j] @ (K @ X[j])
            assert abs(got["energy_total"][j] - dKd) <= 1e-12 * abs(dKd), name
            assert got["von_mises_max"][j] == got["von_mises"][j].max(), name
            assert got["von_mises_argmax"][j] == int(np.argmax(got["von_mises"][j])), name


def test_patch_test_and_rigid_motion(meshes):
    m = meshes["delaunay_beam(2)"]
    rng = np.random.default_rng(7)
    A, b = rng.normal(size=(3, 3)), rng.normal(size=3)
    with _rec(m.points, m.tets) as rec:
        S = 0.5 * (A + A.T)
        want = fo.elasticity_D(LMD, MU) @ np.array([S[0, 0], S[1, 1], S[2, 2], 2 * S[1, 2], 2 * S[0, 2], 2 * S[0, 1]])
        u = m.points @ A.T + b
        r = rec.element(_t(u.reshape(-1)))
        sig = r["sigma"].cpu().numpy()
        nod = rec.nodal(r["sigma"]).cpu().numpy()
        scale = np.abs(want).max()
        assert np.abs(sig - want).max() <= 1e-11 * scale
        assert np.abs(nod - want).max() <= 1e-11 * scale
        W = A - A.T  # skew: rigid rotation
        rs = rec.element(_t((m.points @ W.T + b).reshape(-1)))["sigma"].cpu().numpy()
        assert np.abs(rs).max() <= 1e-11 * (LMD + 2 * MU) * np.abs(W).max()


def test_vertex_order_does_not_matter(meshes):
    m = meshes["delaunay_beam(2)"]
    rng = np.random.default_rng(11)
    tets = m.tets.copy()
    pick = rng.choice(len(tets), len(tets) // 10, replace=False)
    perms = np.array([[1, 0, 2, 3], [0, 2, 1, 3], [1, 2, 0, 3], [3, 2, 1, 0], [2, 0, 3, 1]])  # odd and even
    for k, e in enumerate(pick):
        tets[e] = tets[e][perms[k % len(perms)]]
    X = _t(rng.normal(size=(2, 3 * len(m.points))))
    out = []
    for cells in (m.tets, tets):
        with _rec(m.points, cells) as rec:
            r = rec.element(X)
            r["nodal"] = rec.nodal(r["sigma"])
            out.append({k: v.cpu().numpy() for k, v in r.items()})
    for k in ("sigma", "von_mises", "energy", "nodal"):
        assert np.abs(out[0][k] - out[1][k]).max() <= 1e-13 * np.abs(out[0][k]).max(), k


def test_energy_of_recorded_step_kernel_trajectory():
    import torch

    import synchronization_avoiding_algorithms_amd as saa
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(3)
    lay, _, l_M, F_rankwise, dt = fs.rank_problem(mesh.points, mesh.tets, None, np.zeros(len(mesh.tets), dtype=int), 0, 1,
                                                  1e6, 0.3, 1.0, 0.5, 0.9, device=0, facets=mesh.triangles)
    pts = mesh.points[lay.nodes]
    sol = saa.HipExplicitSolver(pts, lay.cells_local, l_M, F_rankwise, lay.dirichlet_dofs, LMD, MU, dt, 0.5, device=0)
    n_steps = 200
    traj = torch.zeros((sol.n_dof, n_steps), dtype=torch.float64, device=DEV)
    sol.set_recorder(traj, 1, 0)
    sol.step(n_steps)
    sol.synchronize()
    sol.set_recorder(None)
    with _rec(pts, lay.cells_local) as rec:
        h = rec.history(traj)
        got = h["energy_total"].cpu().numpy()
        for j in range(n_steps):
            d = traj[:, j].contiguous()
            f = torch.empty_like(d)
            sol.internal_force_device(d, f)
            want = 0.5 * float(torch.dot(d, f))
            assert abs(got[j] - want) <= 1e-12 * abs(want) + 1e-300, j
        el = rec.element(traj[:, -5:].T.contiguous())
        assert torch.equal(el["energy_total"], h["energy_total"][-5:]) and torch.equal(el["von_mises_argmax"], h["von_mises_argmax"][-5:])
    assert got[-1] > 0
    sol.close()


def test_strides_batching_null_outputs_and_validation(meshes):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    m = meshes["structured_beam(2)"]
    n, ne = 3 * len(m.points), len(m.tets)
    g = torch.Generator(DEV).manual_seed(5)
    with _rec(m.points, m.tets) as rec:
        for mc in (1, 5, 16):
            ldx, lds, lde = n + 5, 6 * ne + 7, ne + 3
            X = torch.rand((mc, ldx), dtype=torch.float64, device=DEV, generator=g) - 0.5
            S = torch.full((mc, lds), 7.0, dtype=torch.float64, device=DEV)
            V, W = (torch.full((mc, lde), 7.0, dtype=torch.float64, device=DEV) for _ in range(2))
            T, M = (torch.full((mc,), 7.0, dtype=torch.float64, device=DEV) for _ in range(2))
            A = torch.full((mc,), 7, dtype=torch.int32, device=DEV)
            rec.stress_raw(mc, X, ldx, S, lds, V, W, lde, T, M, A)
            torch.cuda.synchronize()
            assert (S[:, 6 * ne:] == 7.0).all() and (V[:, ne:] == 7.0).all() and (W[:, ne:] == 7.0).all()
            for j in range(mc):
                one = rec.element(X[j, :n].contiguous())
                assert torch.equal(S[j, :6 * ne], one["sigma"].reshape(-1)) and torch.equal(V[j, :ne], one["von_mises"])
                assert torch.equal(W[j, :ne], one["energy"]) and T[j] == one["energy_total"]
                assert M[j] == one["von_mises_max"] and A[j] == one["von_mises_argmax"]
            # every combination of NULL outputs
            for mask in range(64):
                outs = [torch.full_like(t, 9) for t in (S, V, W, T, M, A)]
                use = [o if mask >> i & 1 else None for i, o in enumerate(outs)]
                rec.stress_raw(mc, X, ldx, use[0], lds, use[1], use[2], lde, use[3], use[4], use[5])
                torch.cuda.synchronize()
                for i, (o, ref, k) in enumerate(zip(outs, (S, V, W, T, M, A), (6 * ne, ne, ne, mc, mc, mc))):
                    if mask >> i & 1:
                        assert torch.equal(o[..., :k], ref[..., :k]) and (o[..., k:] == 9).all(), (mc, mask, i)
                    else:
                        assert (o == 9).all(), (mc, mask, i)
        X = torch.zeros(n, dtype=torch.float64, device=DEV)
        S = torch.zeros(6 * ne, dtype=torch.float64, device=DEV)
        E6 = torch.zeros((ne, 9), dtype=torch.float64, device=DEV)
        N6 = torch.zeros((len(m.points), 9), dtype=torch.float64, device=DEV)
        for bad, msg in (((0, X, n, S, 6 * ne), "m = 0"), ((17, X, n, S, 6 * ne), "m = 17"),
                         ((1, X, n - 1, S, 6 * ne), "ldx"), ((1, X, n, S, 6 * ne - 1), "ld_sigma")):
            with pytest.raises(_lib.SaaError, match=msg) as ei:
                rec.stress_raw(*bad)
            assert ei.value.code == _lib.SAA_E_ARG
        with pytest.raises(_lib.SaaError, match="ld_elem") as ei:
            rec.stress_raw(1, X, n, None, 0, S, None, ne - 1)
        assert ei.value.code == _lib.SAA_E_ARG
        for bad, msg in (((1, 0, E6, 9 * ne, N6, 9 * len(m.points)), "k = 0"), ((1, 9, E6, 9 * ne, N6, 9 * len(m.points)), "k = 9"),
                         ((0, 6, E6, 6 * ne, N6, 6 * len(m.points)), "m = 0"), ((17, 6, E6, 6 * ne, N6, 6 * len(m.points)), "m = 17"),
                         ((1, 6, E6, 6 * ne - 1, N6, 6 * len(m.points)), "ld_elem"),
                         ((1, 6, E6, 6 * ne, N6, 6 * len(m.points) - 1), "ld_node")):
            with pytest.raises(_lib.SaaError, match=msg) as ei:
                rec.nodal_raw(*bad)
            assert ei.value.code == _lib.SAA_E_ARG


def test_repeatable_bits_and_nodal_average(meshes):
    import torch

    m = meshes["delaunay_beam(2)"]
    rng = np.random.default_rng(13)
    X = _t(rng.normal(size=(20, 3 * len(m.points))))
    ns = NumpyStress(m.points, m.tets, LMD, MU)
    with _rec(m.points, m.tets) as rec:
        a, b = rec.element(X), rec.element(X)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(rec.nodal(a["sigma"]), rec.nodal(a["sigma"]))
        for k in (1, 6, 8, 11):
            E = _t(rng.normal(size=(17, len(m.tets), k)))
            got = rec.nodal(E).cpu().numpy()
            want = ns.nodal(E.cpu().numpy())
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), k
        one = rec.nodal(a["sigma"][3])
        assert torch.equal(one, rec.nodal(a["sigma"])[3])


def test_driver_on_the_reference_two_rank_snapshots(tmp_path, beam_coarse):
    from synchronization_avoiding_algorithms_amd import drivers

    g = write_tworank_tree(str(tmp_path))
    steps = [int(s) for s in g["steps"]]
    rep = drivers.stress(beam_coarse, str(tmp_path), columns=range(len(steps)), history=True)
    want = serial_element_stress(beam_coarse.points, beam_coarse.tets, LMD, MU)
    for j, step in enumerate(steps):
        f = parse_vtk(os.path.join(tmp_path, "Results", "Stress", f"Stress-col-{j}.vtk"))
        got = np.stack([f["cell_data"][f"sigma-{c}"] for c in VOIGT], axis=1)
        if step == 1:
            assert not got.any()
            continue
        assert np.abs(got - want[step]).max() <= 1e-10 * np.abs(want[step]).max(), step
    # the same tree through the NumPy stand-in
    ref = drivers.stress(beam_coarse, str(tmp_path), columns=range(len(steps)), vtk=False, recovery=NumpyStress)
    for c, r in zip(rep["columns"], ref["columns"]):
        assert c["element"] == r["element"] or c["von_mises_max"] == 0.0
        assert abs(c["strain_energy"] - r["strain_energy"]) <= 1e-12 * abs(r["strain_energy"])


def test_driver_modeled_on_the_hybrid_run(tmp_path, beam_coarse):
    from synchronization_avoiding_algorithms_amd import drivers

    h = load_golden("hybrid_tworank.npz")
    g = load_golden("tworank_trajectory.npz")
    assert np.array_equal(h["epart"], g["epart"])
    truth = [h[f"r{r}_truth_last"].reshape(-1, 1) for r in range(2)]
    modeled = [h[f"r{r}_modeled"][:, -1:] for r in range(2)]
    write_tworank_tree(str(tmp_path))
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.drivers import PATHS

    for r in range(2):
        rio.save_displacement(os.path.join(tmp_path, PATHS["truth"].format(r=r)), truth[r])
        rio.save_displacement(os.path.join(tmp_path, PATHS["modeled"].format(r=r)), modeled[r])
    rep = drivers.stress(beam_coarse, str(tmp_path), columns=[0], modeled=True, vtk=False)["columns"][0]
    ne = len(beam_coarse.tets)
    vm = {}
    for key, runs in (("truth", truth), ("modeled", modeled)):
        v = np.zeros(ne)
        for r in range(2):
            nodes, elems = g[f"r{r}_local_nodes"], g[f"r{r}_local_elements"]
            pos = {int(x): i for i, x in enumerate(nodes)}
            cells = np.vectorize(pos.get)(beam_coarse.tets[elems])
            v[elems] = NumpyStress(beam_coarse.points[nodes], cells, LMD, MU).element(runs[r].T)["von_mises"][0]
        vm[key] = v
    dvm = np.abs(vm["modeled"] - vm["truth"])
    iface = np.isin(beam_coarse.tets, g["Global_shared"]).any(axis=1)
    assert abs(rep["von_mises_rel_l2"] - np.linalg.norm(vm["modeled"] - vm["truth"]) / np.linalg.norm(vm["truth"])) <= 1e-10
    assert rep["dvm_element"] == int(np.argmax(dvm)) and abs(rep["dvm_max"] - dvm.max()) <= 1e-10 * dvm.max()
    assert abs(rep["dvm_max_interface"] - dvm[iface].max()) <= 1e-10 * dvm.max()
    assert abs(rep["dvm_max_interior"] - dvm[~iface].max()) <= 1e-10 * dvm.max()
    assert rep["modeled"]["element"] == int(np.argmax(vm["modeled"])) and rep["element"] == int(np.argmax(vm["truth"]))
    # identical files: every difference exactly 0
    for r in range(2):
        rio.save_displacement(os.path.join(tmp_path, PATHS["modeled"].format(r=r)), truth[r])
    same = drivers.stress(beam_coarse, str(tmp_path), columns=[0], modeled=True, vtk=False)["columns"][0]
    assert same["von_mises_rel_l2"] == 0.0 and same["dvm_max"] == 0.0
    assert same["dvm_max_interface"] == 0.0 and same["dvm_max_interior"] == 0.0


def test_cli_data_prepare_then_stress(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    base = [sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers"]
    r = subprocess.run(base + ["data_prepare", "--synthetic", "2", "--steps", "40", "--out", str(tmp_path)], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["stress", "--synthetic", "2", "--columns", "0,-1", "--history", "--out", str(tmp_path)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    rep = json.loads(lines[0])
    assert [c["column"] for c in rep["columns"]] == [0, 39]
    for c in rep["columns"]:
        assert {"strain_energy", "von_mises_max", "element", "centroid"} <= set(c)
    assert rep["columns"][1]["strain_energy"] > 0
    for path in rep["files"]:
        f = parse_vtk(path)
        assert len(f["cell_data"]["von-mises"]) == rep["n_elems"] and len(f["point_data"]["von-mises"]) == rep["n_nodes"]
        assert np.isclose(f["cell_data"]["von-mises"].max(), [c["von_mises_max"] for c in rep["columns"]
                                                               if path.endswith(f"-{c['column']}.vtk")][0], rtol=1e-15)
    h = np.load(rep["history"])
    assert len(h["strain_energy"]) == 40 and len(h["von_mises_max"]) == 40
    assert h["strain_energy"][-1] == rep["columns"][1]["strain_energy"]
    assert np.array_equal(von_mises(np.zeros((2, 6))), np.zeros(2))
