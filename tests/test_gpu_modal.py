"""Modal analysis on the MI355X: the element stable-frequency kernel, the block apply of K and the consistent M, the stable
time step (checked against the explicit solver itself), the lowest modes, the drop-in Eigen_mode and the driver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

from conftest import REPO
from oracle import fem_oracle as fo
from test_modal import E, GAMMA, LMD, MU, NU, RHO, TABLE, Dense, _meshes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def meshes():
    return _meshes()


@pytest.fixture(scope="module")
def dense(meshes):
    return {name: Dense(m) for name, m in meshes.items()}


def _op(m, **kw):
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(m.points, m.tets, fo.node_to_dof(clamp_nodes(m)), LMD, MU, RHO, device=0, **kw)


def test_element_kernel_matches_the_host_formula(meshes):
    from synchronization_avoiding_algorithms_amd import modal
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    for name, m in meshes.items():
        with _op(m) as op:
            b = op.element_bound(return_omega=True)
            b2 = op.element_bound()
        got = b["omega_e"].cpu().numpy()
        want, _ = modal.element_omega(m.points, m.tets, LMD, MU, RHO)
        assert np.abs(got / want - 1.0).max() <= 1e-12, name
        assert b["certified"] and b["n_nonpositive"] == 0
        assert b["omega_max"] == got.max() and b["element"] == int(np.argmax(got)), name  # first maximum, exact
        assert want[b["element"]] >= want.max() * (1 - 1e-12), name  # lattices have exact ties up to round-off
        if name == "delaunay_beam(2)":
            assert b["element"] == int(np.argmax(want))
        assert (b2["omega_max"], b2["element"]) == (b["omega_max"], b["element"])  # repeatable
    m = structured_beam(19)
    with _op(m) as op:
        got = op.element_bound(return_omega=True)["omega_e"]
        idx = np.random.default_rng(0).choice(len(m.tets), 10_000, replace=False)
        got = got.cpu().numpy()[idx]
    want, _ = modal.element_omega(m.points, m.tets[idx], LMD, MU, RHO)
    assert np.abs(got / want - 1.0).max() <= 1e-12


def test_element_kernel_refuses_to_certify_inverted_elements(meshes):
    from synchronization_avoiding_algorithms_amd.mesh import Mesh

    m = meshes["structured_beam(2)"]
    tets = m.tets.copy()
    tets[[3, 50]] = tets[[3, 50]][:, [0, 2, 1, 3]]
    with _op(Mesh(m.points, {"tetra": tets, "triangle": m.triangles})) as op:
        b = op.element_bound()
    assert not b["certified"] and b["n_nonpositive"] == 2


def _consistent_mass(m):
    from scipy.sparse import coo_matrix

    Me, _ = fo.element_mass_force(m.points[m.tets], RHO, 0.0)
    dof = fo.node_to_dof(m.tets.ravel()).reshape(-1, 12)
    n3 = 3 * len(m.points)
    return coo_matrix((Me.ravel(), (np.repeat(dof, 12, axis=1).ravel(), np.tile(dof, (1, 12)).ravel())), shape=(n3, n3)).tocsr()


def test_block_apply_matches_the_step_kernel_and_the_assembled_mass(meshes):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes
    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver

    dev = torch.device("cuda", 0)
    for name in ("beam_coarse", "structured_beam(2)"):
        m = meshes[name]
        dd = fo.node_to_dof(clamp_nodes(m))
        lumped, load, _ = fs.device_setup_fields(m.points, m.tets, RHO, 0.5, 0)
        sol = HipExplicitSolver(m.points, m.tets, lumped, load, dd, LMD, MU, 1e-4, 0.5, device=0)
        sol.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        M = _consistent_mass(m)
        n = 3 * len(m.points)
        free = np.ones(n)
        free[dd] = 0.0
        ft = torch.as_tensor(free, device=dev)
        with _op(m) as op:
            for mcols in (1, 5, 16):
                ld = n + (7 if mcols == 5 else 0)  # a leading dimension above 3 * n_nodes
                X = torch.rand((mcols, ld), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(mcols)) - 0.5
                KX = torch.full((mcols, ld), 7.0, dtype=torch.float64, device=dev)
                MX = torch.full((mcols, ld), 7.0, dtype=torch.float64, device=dev)
                op.apply_raw(mcols, X, ld, KX, MX)
                torch.cuda.synchronize()
                for j in range(mcols):
                    xj = (X[j, :n] * ft).contiguous()
                    want_k = torch.empty(n, dtype=torch.float64, device=dev)
                    sol.internal_force_device(xj, want_k)
                    want_k = (want_k * ft).cpu().numpy()
                    want_m = free * (M @ xj.cpu().numpy())
                    gk, gm = KX[j, :n].cpu().numpy(), MX[j, :n].cpu().numpy()
                    assert np.linalg.norm(gk - want_k) <= 1e-13 * np.linalg.norm(want_k), (name, mcols, j)
                    assert np.linalg.norm(gm - want_m) <= 1e-13 * np.linalg.norm(want_m), (name, mcols, j)
                    assert not gk[dd].any() and not gm[dd].any()
                if ld > n:
                    assert (KX[:, n:] == 7.0).all() and (MX[:, n:] == 7.0).all()  # nothing written past the columns
                KX2, MX2 = torch.empty_like(KX), torch.empty_like(MX)
                op.apply_raw(mcols, X, ld, KX2, MX2)
                torch.cuda.synchronize()
                assert torch.equal(KX2[:, :n], KX[:, :n]) and torch.equal(MX2[:, :n], MX[:, :n])  # bitwise repeatable
            X = torch.zeros((17, n), dtype=torch.float64, device=dev)
            with pytest.raises(_lib.SaaError, match="1 <= m <= 16") as ei:
                op.apply_raw(17, X, n, torch.empty_like(X))
            assert ei.value.code == _lib.SAA_E_ARG
            KX, MX = op.apply(X, k=True, m=True)  # the Python face splits 17 columns into 16 + 1
            assert KX.shape == (17, n) and not KX.any() and not MX.any()
        sol.close()


def test_stable_time_step_reproduces_the_table(meshes, dense):
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes
    from synchronization_avoiding_algorithms_amd.modal import stable_time_step

    for name, m in meshes.items():
        r = stable_time_step(m.points, m.tets, clamp_nodes(m), E, NU, RHO, GAMMA, device=0)
        dt_ref, dt_crit, dt_bound = TABLE[name][:3]
        assert r["dt_reference"] == fo.cfl_dt(m.tets, m.points, E, NU, RHO, GAMMA)  # the reference's rule, bit for bit
        assert r["dt_reference"] == pytest.approx(dt_ref, rel=2e-3)
        assert r["dt_crit"] == pytest.approx(dt_crit, rel=2e-3) and r["dt_bound"] == pytest.approx(dt_bound, rel=2e-3)
        assert abs(r["omega_max"] / dense[name].omega_max() - 1.0) <= 1e-10
        assert r["certified"] and r["dt_bound"] <= r["dt_crit"] and r["lanczos_residual"] <= 1e-8
        assert r["ratio"] == pytest.approx(r["dt_reference"] / r["dt_crit"])


def test_dt_crit_is_the_limit_of_the_explicit_solver(meshes, dense):
    """d0 = dn = the top eigenvector of M_L^-1 K, no load, the reference's alpha = 0.5: bounded just below dt_crit,
    exponential growth just above it."""
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes
    from synchronization_avoiding_algorithms_amd.modal import stable_time_step
    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver

    m, d = meshes["structured_beam(2)"], dense["structured_beam(2)"]
    dt_crit = stable_time_step(m.points, m.tets, clamp_nodes(m), E, NU, RHO, GAMMA, device=0)["dt_crit"]
    s = 1.0 / np.sqrt(d.lumped[d.free])
    _, vec = np.linalg.eigh(s[:, None] * d.Kf * s[None, :])
    v = np.zeros(len(d.free))
    v[d.free] = s * vec[:, -1]
    lumped, _, _ = fs.device_setup_fields(m.points, m.tets, RHO, 0.5, 0)
    amps = {}
    for factor in (0.99, 1.01):
        sol = HipExplicitSolver(m.points, m.tets, lumped, np.zeros(len(v)), d.dirichlet, LMD, MU, factor * dt_crit, 0.5,
                                device=0)
        sol.set_state(v, v)
        a = [np.abs(v).max()]
        for _ in range(200):
            sol.step(1)
            a.append(float(np.abs(sol.get_state()[0]).max()))
        sol.close()
        amps[factor] = np.array(a)
    a = amps[0.99]
    assert a[100:].max() <= 1.01 * a[:101].max(), (a[:101].max(), a[100:].max())
    b = amps[1.01]
    assert np.isfinite(b).all() and b[100] > 1e6 * b[0], b[100] / b[0]


def test_lowest_modes_on_the_gpu(meshes, dense):
    from scipy.sparse.linalg import eigsh

    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes, structured_beam
    from synchronization_avoiding_algorithms_amd.modal import device_lowest_modes
    from synchronization_avoiding_algorithms_amd.Tools import Mat_construction as MC
    from synchronization_avoiding_algorithms_amd.Tools import commons as CM

    for name in ("beam_coarse", "delaunay_beam(2)"):
        m = meshes[name]
        with _op(m) as op:
            r = device_lowest_modes(op, m.points, m.tets, LMD, MU, 10)
        want = np.sqrt(dense[name].lowest_omega2(10)) / (2 * np.pi)
        assert r["converged"] and np.abs(r["frequencies_hz"] / want - 1.0).max() <= 1e-9, (name, r["frequencies_hz"], want)
    m = structured_beam(4)
    dd = fo.node_to_dof(clamp_nodes(m))
    free = np.ones(3 * len(m.points), dtype=bool)
    free[dd] = False
    M, K, _ = MC.Global_Assembly(1, m.tets, m.points, dd, CM.elasticity(LMD, MU, RHO, 0.5, False), None, sparse=True)
    w2 = np.sort(eigsh(K[free][:, free].tocsc(), 10, M[free][:, free].tocsc(), sigma=0, which="LM", tol=1e-13)[0])
    with _op(m) as op:
        r = device_lowest_modes(op, m.points, m.tets, LMD, MU, 10)
    assert np.abs(r["frequencies_hz"] / (np.sqrt(w2) / (2 * np.pi)) - 1.0).max() <= 1e-7, (r["residuals"], r["omega2"], w2)


def test_eigen_mode_prints_the_reference_spectrum(meshes, capsys):
    from synchronization_avoiding_algorithms_amd.Tools import Mat_construction as MC
    from synchronization_avoiding_algorithms_amd.Tools import commons as CM
    from synchronization_avoiding_algorithms_amd.Tools.Steady_solvers import Eigen_mode

    m = meshes["beam_coarse"]
    d = Dense(m)
    elas = CM.elasticity(LMD, MU, RHO, 0.5, False)
    assert Eigen_mode(1, m.tets, m.points, d.dirichlet.tolist(), elas) == 0
    out = capsys.readouterr().out
    got = np.array(out.strip().lstrip("[").rstrip("]").split(), dtype=np.float64)
    # the reference's pair (Steady_solvers.py:27-33): Global_Assembly, then M[d, d] = 1
    M, K, _ = MC.Global_Assembly(1, m.tets, m.points, d.dirichlet.tolist(), elas, None, steady=False)
    for dof in d.dirichlet:
        M[dof, dof] = 1
    w2 = sl.eigh(K, M, eigvals_only=True)
    want = np.sqrt(np.clip(w2, 0.0, None)) / (2 * np.pi)
    assert len(got) == 50 and len(d.dirichlet) == 15
    assert (got[:15] == 0.0).all()
    assert np.abs(got[15:] / want[15:50] - 1.0).max() <= 1e-8


def test_drivers_modal_prints_one_json_object():
    env = {k: v for k, v in os.environ.items()}
    out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "modal", "--synthetic", "2",
                          "--k", "4"], cwd=REPO, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["n_elems"] == 1200 and res["certified"] and len(res["frequencies_hz"]) == 4
    assert res["dt_crit"] == pytest.approx(TABLE["structured_beam(2)"][1], rel=2e-3)
    assert max(res["residuals"]) <= 1e-8 and res["dt_bound"] <= res["dt_crit"]
