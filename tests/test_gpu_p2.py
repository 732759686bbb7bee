"""Quadratic (10-node) tetrahedra on the GPU: the order-2 ``saa_operator`` handle against the reference's own results
(tests/golden/p2_beam.npz: straight and curved elements) and the NumPy double (tests/p2_double.py), the steady and modal
drop-ins and the drivers' ``--order 2``.

Bars: rel-L2 < 1e-13 per column for ``K X``, ``M X``, the load and the diagonals (the project's ``K d`` bar, DESIGN.md
section 2); < 1e-9 for the steady solution (tests/test_steady.py); frequencies to 1e-9 with residuals <= 1e-8 and the printed
spectrum to 1e-8 (tests/test_gpu_modal.py).  Tip deflection: Euler-Bernoulli gives q L^4 / (8 E I) = 0.5 * 6^4 / (8e6 / 12)
= 9.72e-4 per axis for the 6 x 1 x 1 cantilever; the reference's p = 2 result on 288 tets is within 1 % of it and its p = 1
result on the same vertices is 0.44 of it (linear tetrahedra lock in bending), so the bars are |ratio - 1| <= 0.02 and
|ratio - 0.44| <= 0.02."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden, rel_l2

import p2_double as p2

pytestmark = pytest.mark.gpu

SETS = ("straight", "curved")
THEORY_TIP = 0.5 * 6.0 ** 4 / (8.0 * 1e6 / 12.0)


@pytest.fixture(scope="module")
def gold():
    g = load_golden("p2_beam.npz")
    g["mat"] = tuple(float(g[k]) for k in ("lmd", "mu", "rho", "fz"))
    return g


def _op(points, cells, dirichlet, lmd, mu, rho):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(points, cells, dirichlet, lmd, mu, rho)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


@pytest.mark.parametrize("name", SETS)
def test_apply_load_and_diagonal_match_the_reference_and_the_double(gold, name):
    pts, c10, dd = gold[f"points_{name}"], gold["cells10"], gold["dirichlet_dofs"]
    lmd, mu, rho, fz = gold["mat"]
    X = gold["X"].T.copy()                                                           # (3, n_dof)
    with _op(pts, c10, dd, lmd, mu, rho) as op:
        assert op.order == 2 and op.n_elems == 288 and op.n_nodes == 625
        KX, MX = op.apply(_dev(X), k=True, m=True)
        KX, MX = KX.cpu().numpy(), MX.cpu().numpy()
        F = op.load((0.0, -fz, -fz)).cpu().numpy()
        dk, dm = (t.cpu().numpy() for t in op.diagonal())
    want_m = p2.apply_m(pts, c10, dd, rho, X)
    want_dk, want_dm = p2.diagonals(pts, c10, dd, lmd, mu, rho)
    ek = [rel_l2(KX[j], gold[f"KX_{name}"][:, j]) for j in range(3)]
    em = [rel_l2(MX[j], want_m[j]) for j in range(3)]
    ef, edk = rel_l2(F, gold[f"F_{name}"]), rel_l2(dk, gold[f"diagK_{name}"])
    edk2, edm = rel_l2(dk, want_dk), rel_l2(dm, want_dm)
    print(name, "K X", ek, "M X", em, "F", ef, "diag K", edk, edk2, "diag M", edm)
    assert max(ek) < 1e-13 and max(em) < 1e-13 and ef < 1e-13 and edk < 1e-13 and edk2 < 1e-13 and edm < 1e-13
    for out in (KX, MX):
        assert not out[:, dd].any()
    assert not F[dd].any() and not dk[dd].any() and not dm[dd].any()


def test_order_one_load_and_diagonal(gold):
    from synchronization_avoiding_algorithms_amd.steady import stiffness_diagonal

    lmd, mu, rho, fz = gold["mat"]
    nv = int(gold["n_vertices"])
    pts, tets = gold["points_straight"][:nv], gold["cells10"][:, :4]
    dd = np.nonzero(np.repeat(np.abs(pts[:, 0]) < 1e-9, 3))[0]
    want = stiffness_diagonal(pts, tets, lmd, mu)
    p = pts[tets]
    vol = np.einsum("ei,ei->e", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])) / 6.0
    node_vol = np.bincount(tets.ravel(), weights=np.repeat(vol, 4), minlength=nv)
    for dofs in (np.zeros(0, dtype=np.int64), dd):
        free = np.ones(3 * nv)
        free[dofs] = 0.0
        with _op(pts, tets, dofs, lmd, mu, rho) as op:
            assert op.order == 1
            dk, dm = (t.cpu().numpy() for t in op.diagonal())
            F = op.load((0.0, -fz, -fz)).cpu().numpy()
        e1, e2 = rel_l2(dk, want * free), rel_l2(dm, np.repeat(rho * node_vol / 10.0, 3) * free)
        e3 = rel_l2(F, (np.repeat(node_vol / 4.0, 3) * np.tile([0.0, -fz, -fz], nv)) * free)
        print("order 1: diag K", e1, "diag M", e2, "load", e3)
        assert e1 < 1e-13 and e2 < 1e-13 and e3 < 1e-13
        assert not dk[dofs].any() and not dm[dofs].any() and not F[dofs].any()


def test_masks_and_repeatability(gold):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    pts, c10, dd = gold["points_curved"], gold["cells10"], gold["dirichlet_dofs"]
    lmd, mu, rho, _ = gold["mat"]
    n = 3 * len(pts)
    g = torch.Generator().manual_seed(5)
    X = (torch.rand((16, n), generator=g, dtype=torch.float64) - 0.5).cuda()
    with _op(pts, c10, dd, lmd, mu, rho) as op:
        KX, MX = op.apply(X, k=True, m=True)
        assert not KX[:, dd].any() and not MX[:, dd].any()
        # garbage on Dirichlet inputs changes no output bit
        Xg = X.clone()
        Xg[:, dd[0::3]] = float("nan")
        Xg[:, dd[1::3]] = float("inf")
        Xg[:, dd[2::3]] = 1e300
        KXg, MXg = op.apply(Xg, k=True, m=True)
        assert torch.equal(KXg, KX) and torch.equal(MXg, MX)
        # two identical calls, K and M alone or together
        KX2, MX2 = op.apply(X, k=True, m=True)
        assert torch.equal(KX2, KX) and torch.equal(MX2, MX)
        assert torch.equal(op.apply(X)[0], KX) and torch.equal(op.apply(X, k=False, m=True)[1], MX)
        # a column does not depend on the others in the call
        for j in (0, 7, 15):
            kj, mj = op.apply(X[j].clone(), k=True, m=True)
            assert torch.equal(kj, KX[j]) and torch.equal(mj, MX[j]), j
        k5, _ = op.apply(X[3:8].contiguous())
        assert torch.equal(k5, KX[3:8])
        # column counts outside 1..16
        big = torch.zeros((17, n), dtype=torch.float64, device="cuda")
        out = torch.zeros_like(big)
        for m in (0, 17):
            with pytest.raises(_lib.SaaError) as ei:
                op.apply_raw(m, big, n, out, None)
            assert ei.value.code == _lib.SAA_E_ARG
        assert not out.any()


@pytest.mark.parametrize("name", SETS)
def test_rigid_body_modes_and_symmetry(gold, name):
    import torch

    pts, c10 = gold[f"points_{name}"], gold["cells10"]
    lmd, mu, rho, _ = gold["mat"]
    n = len(pts)
    R = np.zeros((6, n, 3))
    for c in range(3):
        R[c, :, c] = 1.0
        axis = np.zeros(3)
        axis[c] = 1.0
        R[3 + c] = np.cross(axis, pts)
    R = R.reshape(6, 3 * n)
    g = torch.Generator().manual_seed(9)
    XY = (torch.rand((2, 3 * n), generator=g, dtype=torch.float64) - 0.5).cuda()
    with _op(pts, c10, np.zeros(0, dtype=np.int32), lmd, mu, rho) as op:
        KR = op.apply(_dev(R))[0].cpu().numpy()
        knorm = float(op.diagonal(m=False)[0].max())                                  # <= |K|_2
        KXY, MXY = op.apply(XY, k=True, m=True)
    ratios = np.linalg.norm(KR, axis=1) / (knorm * np.linalg.norm(R, axis=1))
    print(name, "|K r| / (|K| |r|)", ratios)
    assert ratios.max() <= 1e-12
    x, y = XY[0], XY[1]
    for A in (KXY, MXY):
        a, b = float(x @ A[1]), float(y @ A[0])
        scale = float(torch.linalg.vector_norm(x) * torch.linalg.vector_norm(A[1]))
        print(name, "x.Ay - y.Ax", a - b, "scale", scale)
        assert abs(a - b) <= 1e-12 * scale


def test_linear_element_entry_points_refuse_an_order_two_handle(gold):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    lmd, mu, rho, _ = gold["mat"]
    lib = _lib.load()
    buf = torch.zeros(16 * 3 * 625, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    with _op(gold["points_straight"], gold["cells10"], gold["dirichlet_dofs"], lmd, mu, rho) as op:
        with pytest.raises(_lib.SaaError, match="order-2"):
            op.element_bound()
        calls = {
            "saa_operator_element_bound": lambda: lib.saa_operator_element_bound(op._h, None, None, None, None),
            "saa_operator_stress": lambda: lib.saa_operator_stress(op._h, 1, p, 1875, p, 6 * 288, None, None, 288, None, None, None),
            "saa_operator_nodal_average": lambda: lib.saa_operator_nodal_average(op._h, 1, 6, p, 6 * 288, p, 6 * 625),
            "saa_operator_stress_error": lambda: lib.saa_operator_stress_error(op._h, 1, p, 6 * 288, p, 6 * 625, None, 0, p, 288,
                                                                               None, None, None),
        }
        for name, call in calls.items():
            assert call() == _lib.SAA_E_ARG, name
            msg = lib.saa_last_error().decode()
            assert name in msg and "order-2" in msg, msg
        torch.cuda.synchronize()
    assert not buf.any()


def test_apply_and_load_beyond_the_dense_route():
    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic

    mesh = to_quadratic(structured_beam(8))
    lmd, mu = lame(1e6, 0.3)
    rho = 1.3
    dd = node_to_dof(plane_nodes(mesh.points))
    rng = np.random.default_rng(8)
    # mid-edge nodes off the clamp plane moved by up to 2.5 % of the cell size: curved elements at this size too
    pts = mesh.points.copy()
    nv = len(structured_beam(8).points)
    move = (np.arange(len(pts)) >= nv) & (np.abs(pts[:, 0]) > 1e-9)
    pts[move] += rng.uniform(-0.003125, 0.003125, size=(int(move.sum()), 3))
    X = rng.uniform(-1e-2, 1e-2, size=(2, 3 * len(pts)))
    with _op(pts, mesh.tets10, dd, lmd, mu, rho) as op:
        assert op.n_elems == 76800
        KX, MX = (t.cpu().numpy() for t in op.apply(_dev(X), k=True, m=True))
        F = op.load((0.1, -0.5, -0.5)).cpu().numpy()
        dk, dm = (t.cpu().numpy() for t in op.diagonal())
    want_k, want_m = p2.apply_k(pts, mesh.tets10, dd, lmd, mu, X), p2.apply_m(pts, mesh.tets10, dd, rho, X)
    want_dk, want_dm = p2.diagonals(pts, mesh.tets10, dd, lmd, mu, rho)
    errs = [rel_l2(KX[j], want_k[j]) for j in range(2)] + [rel_l2(MX[j], want_m[j]) for j in range(2)]
    ef = rel_l2(F, p2.load(pts, mesh.tets10, dd, (0.1, -0.5, -0.5)))
    ed = (rel_l2(dk, want_dk), rel_l2(dm, want_dm))
    print("structured_beam(8) elevated: K X, M X", errs, "load", ef, "diagonals", ed)
    assert max(errs) < 1e-13 and ef < 1e-13 and max(ed) < 1e-13


def _tip(d, pts, n_vert):
    tip = np.nonzero(np.abs(pts[:n_vert, 0] - 6.0) < 1e-9)[0]
    return -np.asarray(d).reshape(-1, 3)[tip, 1].mean()


def test_steady_drop_in(gold):
    from synchronization_avoiding_algorithms_amd.steady import steady_solve_operator
    from synchronization_avoiding_algorithms_amd.Tools import commons as CM
    from synchronization_avoiding_algorithms_amd.Tools.Steady_solvers import Steady_Elasticity_solver

    lmd, mu, rho, fz = gold["mat"]
    c10, dd, nv = gold["cells10"], gold["dirichlet_dofs"], int(gold["n_vertices"])
    elas = CM.elasticity(lmd, mu, rho, fz, False)
    for name in SETS:
        pts = gold[f"points_{name}"]
        d = Steady_Elasticity_solver(2, c10, pts, dd.tolist(), elas)
        assert d.shape == (3 * len(pts), 1)
        err = rel_l2(d, gold[f"d_steady_{name}"])
        with _op(pts, c10, dd, lmd, mu, rho) as op:
            b = op.load((0.0, -fz, -fz))
            d2, its, rel = steady_solve_operator(op, b, tol=1e-12)
            d3, _, rel3 = steady_solve_operator(op, b.repeat(3, 1) * _dev([[1.0], [2.0], [-0.5]]), tol=1e-12)
        print(name, "rel-L2 to d_steady", err, "iterations", its, "reported residual", rel, rel3)
        assert err < 1e-9 and rel <= 1e-12 and rel3 <= 1e-12
        assert rel_l2(d2, gold[f"d_steady_{name}"]) < 1e-9 and not d[dd].any() and not d2[dd].any()
        assert rel_l2(d3[1], 2.0 * d2) < 1e-9 and rel_l2(d3[2], -0.5 * d2) < 1e-9
    pts = gold["points_straight"]
    d = Steady_Elasticity_solver(2, c10, pts, dd.tolist(), elas)
    tip2, tip_ref = _tip(d, pts, nv), _tip(gold["d_steady_straight"], pts, nv)
    dd1 = np.nonzero(np.repeat(np.abs(pts[:nv, 0]) < 1e-9, 3))[0]
    tip1 = _tip(Steady_Elasticity_solver(1, c10[:, :4], pts[:nv], dd1.tolist(), elas), pts, nv)
    print("tip deflection / beam theory: p = 2", tip2 / THEORY_TIP, "reference p = 2", tip_ref / THEORY_TIP, "p = 1",
          tip1 / THEORY_TIP)
    assert abs(tip2 / tip_ref - 1.0) < 1e-9
    assert abs(tip2 / THEORY_TIP - 1.0) <= 0.02 and abs(tip1 / THEORY_TIP - 0.44) <= 0.02


def test_modes_of_the_quadratic_beam(capsys):
    import scipy.linalg as sl

    from synchronization_avoiding_algorithms_amd.fem_setup import lame, node_to_dof
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import device_lowest_modes
    from synchronization_avoiding_algorithms_amd.Tools import commons as CM
    from synchronization_avoiding_algorithms_amd.Tools.Steady_solvers import Eigen_mode

    mesh = to_quadratic(structured_beam(1, length=6.0))
    lmd, mu = lame(1e6, 0.3)
    rho = 1.0
    dd = node_to_dof(plane_nodes(mesh.points))
    assert len(mesh.tets10) == 36 and len(dd) == 27
    K, M = p2.assemble(mesh.points, mesh.tets10, dd, lmd, mu, rho)
    free = np.ones(3 * len(mesh.points), dtype=bool)
    free[dd] = False
    w2 = sl.eigh(K[np.ix_(free, free)], M[np.ix_(free, free)], eigvals_only=True)
    want = np.sqrt(w2) / (2 * np.pi)
    with _op(mesh.points, mesh.tets10, dd, lmd, mu, rho) as op:
        r = device_lowest_modes(op, mesh.points, mesh.tets10, lmd, mu, 6)
    print("frequencies", r["frequencies_hz"], "dense", want[:6], "residuals", r["residuals"])
    assert r["converged"] and r["residuals"].max() <= 1e-8
    assert np.abs(r["frequencies_hz"] / want[:6] - 1.0).max() <= 1e-9
    assert abs(want[0] / 4.49 - 1.0) < 0.01                                         # beam theory, first bending frequency
    capsys.readouterr()
    assert Eigen_mode(2, mesh.tets10, mesh.points, dd.tolist(), CM.elasticity(lmd, mu, rho, 0.5, False)) == 0
    out = capsys.readouterr().out
    got = np.array(out.strip().lstrip("[").rstrip("]").split(), dtype=np.float64)
    assert len(got) == 50 and (got[:27] == 0.0).all()
    assert np.abs(got[27:] / want[:23] - 1.0).max() <= 1e-8


MODAL_KEYS_ORDER_1 = {"n_nodes", "n_elems", "n_free_dofs", "dt_reference", "dt_crit", "dt_bound", "ratio", "certified",
                      "critical_element", "n_nonpositive", "omega_max", "omega_bound", "lanczos_residual", "lanczos_iterations",
                      "frequencies_hz", "residuals", "modes_converged", "outer_iterations", "inner_iterations", "seconds"}


def _driver(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=cwd,
                          capture_output=True, text=True, timeout=300, env=env)


def test_drivers_order_two(tmp_path):
    from synchronization_avoiding_algorithms_amd.mesh import read_vtk

    out = _driver(["steady_state", "--order", "2", "--synthetic", "2", "--out", str(tmp_path / "q")], str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"steady solve \(order 2\): (\d+) CG iterations, relative residual (\S+), max\|d\| = (\S+)", out.stdout)
    assert m and float(m.group(2)) <= 1e-12, out.stdout
    path = tmp_path / "q" / "Results" / "Static" / "steady_distributed.vtk"
    back = read_vtk(str(path))
    assert set(back.cells_dict) == {"tetra10"} and back.tets10.shape == (1200, 10)
    text = path.read_text()
    assert "displacement-x" in text and "displacement-z" in text and "CELL_TYPES 1200\n24\n" in text
    assert np.array_equal(back.points[back.tets10[:, 4]], 0.5 * (back.points[back.tets10[:, 0]] + back.points[back.tets10[:, 1]]))

    out = _driver(["modal", "--order", "2", "--synthetic", "2", "--k", "4"], str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert set(res) == {"order", "n_nodes", "n_elems", "n_free_dofs", "frequencies_hz", "residuals", "modes_converged",
                        "outer_iterations", "inner_iterations", "seconds"}
    assert res["order"] == 2 and res["n_elems"] == 1200 and res["n_nodes"] == len(back.points)
    assert len(res["frequencies_hz"]) == 4 and max(res["residuals"]) <= 1e-8 and res["modes_converged"]

    # The default invocations compute what they did before --order existed: the p = 1 route, restated here the way
    # drivers.steady_state and drivers.modal took it on the parent commit.  Floats to 1e-9 (the steady bar of
    # tests/test_steady.py and the frequency bar of tests/test_gpu_modal.py; the FORCE_ONLY kernel sums with LDS atomics, so
    # two runs need not be bit-equal), dt_reference, integers and flags exactly.
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.drivers import DEFAULTS
    from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes, structured_beam
    from synchronization_avoiding_algorithms_amd.modal import modal_report
    from synchronization_avoiding_algorithms_amd.solver import HipExplicitSolver
    from synchronization_avoiding_algorithms_amd.steady import steady_solve, stiffness_diagonal

    out = _driver(["steady_state", "--synthetic", "2", "--out", str(tmp_path / "l")], str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    assert re.search(r"^steady solve: \d+ CG iterations, relative residual \S+, max\|d\| = \S+$", out.stdout, re.M), out.stdout
    lin_path = tmp_path / "l" / "Results" / "Static" / "steady_distributed.vtk"
    lin = read_vtk(str(lin_path))
    mesh = structured_beam(2)
    assert set(lin.cells_dict) == {"tetra"} and np.array_equal(lin.tets, mesh.tets) and np.array_equal(lin.points, mesh.points)
    assert "CELL_TYPES 1200\n10\n" in lin_path.read_text()
    tok = lin_path.read_text().split()
    got = np.stack([np.array(tok[i + 6: i + 6 + 459], dtype=np.float64)
                    for i in (tok.index(f"displacement-{c}") - 1 for c in "xyz")], axis=1)
    E, nu, rho, fz = (DEFAULTS[k] for k in ("E", "nu", "rho", "fz"))
    lmd, mu = fs.lame(E, nu)
    lumped, fpre, min_edge = fs.device_setup_fields(mesh.points, mesh.tets, rho, fz, 0)
    dd = fs.node_to_dof(clamp_nodes(mesh))
    sol = HipExplicitSolver(mesh.points, mesh.tets, lumped, fpre, dd, lmd, mu,
                            fs.dt_from_min_edge(min_edge, E, nu, rho, DEFAULTS["gamma"]), DEFAULTS["alpha"], device=0)
    want, _, _ = steady_solve(sol, fpre, dd, diag=stiffness_diagonal(mesh.points, mesh.tets, lmd, mu), tol=1e-12)
    sol.close()
    err = rel_l2(got, want.reshape(-1, 3))
    print("default steady_state against steady_solve", err)
    assert err < 1e-9
    out = _driver(["modal", "--synthetic", "2", "--k", "4"], str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    res1 = json.loads(out.stdout.strip().splitlines()[-1])
    assert set(res1) == MODAL_KEYS_ORDER_1
    ref1 = modal_report(mesh.points, mesh.tets, clamp_nodes(mesh), E=E, nu=nu, rho=rho, gamma=DEFAULTS["gamma"], k=4, device=0)
    for key in ("n_nodes", "n_elems", "n_free_dofs", "certified", "critical_element", "n_nonpositive", "dt_reference",
                "modes_converged"):
        assert res1[key] == ref1[key], key
    for key in ("dt_crit", "dt_bound", "ratio", "omega_max", "omega_bound"):
        assert res1[key] == pytest.approx(ref1[key], rel=1e-9), key
    assert res1["frequencies_hz"] == pytest.approx(ref1["frequencies_hz"], rel=1e-9)
    assert res1["n_elems"] == 1200 and res1["n_nodes"] == 459
    # the quadratic beam is softer in bending than the locking linear one
    assert res["frequencies_hz"][0] < res1["frequencies_hz"][0]
