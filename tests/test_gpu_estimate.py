"""Stress error estimate on the MI355X: both forms of ``saa_operator_stress_error`` against the NumPy double, the
Zienkiewicz-Zhu estimate of a quadratic field against its true error, vertex order, repeatability, column grouping,
strides, validation, and the ``drivers estimate`` command on a two-rank tree of the product's own ``data_prepare``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, free_port
from estimate_double import NumpyEstimate, interior_elements, quadratic_field
from oracle import fem_oracle as fo
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


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_both_forms_match_the_double(meshes):
    for name, m in meshes.items():
        rng = np.random.default_rng(3)
        nn, ne = len(m.points), len(m.tets)
        S, N, O = rng.normal(size=(3, ne, 6)), rng.normal(size=(3, nn, 6)), rng.normal(size=(3, ne, 6))
        dbl = NumpyEstimate(m.points, m.tets, LMD, MU)
        with _rec(m.points, m.tets) as rec:
            for form, kw in (("nodal", dict(nodal=N)), ("other", dict(other=O))):
                want = dbl.error(S, **kw)
                got = _np(rec.error(_t(S), **{k: _t(v) for k, v in kw.items()}))
                for j in range(3):
                    err = np.abs(got["eta2"][j] - want["eta2"][j]).max() / want["eta2"][j].max()
                    tot = abs(got["eta2_total"][j] - want["eta2_total"][j]) / want["eta2_total"][j]
                    print(f"{name} {form} column {j}: eta2 {err:.2e} of max, total {tot:.2e}")
                    assert err <= 1e-12, (name, form, j)
                    assert tot <= 1e-12, (name, form, j)
                    assert got["eta2_max"][j] == got["eta2"][j].max(), (name, form, j)
                    assert got["eta2_argmax"][j] == int(np.argmax(got["eta2"][j])), (name, form, j)


def test_argmax_is_the_lowest_index_on_ties(meshes):
    import torch

    m = meshes["structured_beam(2)"]  # congruent elements on dyadic coordinates: equal volumes, bit for bit
    ne = len(m.tets)
    S = torch.zeros((ne, 6), dtype=torch.float64, device=DEV)
    O = torch.ones((ne, 6), dtype=torch.float64, device=DEV)
    with _rec(m.points, m.tets) as rec:
        r = rec.error(S, other=O)
    eta2 = r["eta2"].cpu().numpy()
    assert (eta2 == eta2.max()).sum() > 1
    assert int(r["eta2_argmax"]) == int(np.argmax(eta2)) and float(r["eta2_max"]) == eta2.max()


def test_quadratic_field_effectivity_convergence_and_patch_test():
    from synchronization_avoiding_algorithms_amd import mesh as mesh_mod

    D = fo.elasticity_D(LMD, MU)
    rng = np.random.default_rng(7)
    B, b = rng.normal(size=(3, 3)), rng.normal(size=3)
    for family in ("structured_beam", "delaunay_beam"):
        eta = {}
        for n in (4, 8):
            m = getattr(mesh_mod, family)(n)
            u, exact = quadratic_field(m.points, D)
            with _rec(m.points, m.tets) as rec:
                est = _np(rec.estimate(_t(u)))
                sig = rec.element(_t(u), von_mises=False, energy=False)["sigma"]
                # the exact stress is linear, so its nodal interpolant is the exact stress: this is the true error
                true = _np(rec.error(sig, nodal=_t(exact)))
                if n == 4:
                    aff = _np(rec.estimate(_t((m.points @ B.T + b).reshape(-1))))
            eta[n] = np.sqrt(est["eta2_total"])
            theta = eta[n] / np.sqrt(true["eta2_total"])
            print(f"{family}({n}): eta = {eta[n]:.6f}, theta = {theta:.6f}, relative = {est['relative']:.6f}")
            assert 0.95 <= theta <= 1.05, (family, n)
            assert abs(est["relative"] - np.sqrt(est["eta2_total"] / (2 * est["energy_total"] + est["eta2_total"]))) <= 1e-15
            if family == "structured_beam":
                inner = interior_elements(m.points, m.tets)
                ti = np.sqrt(est["eta2"][inner].sum() / true["eta2"][inner].sum())
                print(f"  interior theta - 1 = {ti - 1:.2e}")
                assert abs(ti - 1) <= 1e-10, n
        print(f"{family}: eta(4) / eta(8) = {eta[4] / eta[8]:.6f}")
        assert 1.9 <= eta[4] / eta[8] <= 2.1, family
        print(f"{family}(4) affine: eta2_total / (2 energy_total) = {aff['eta2_total'] / (2 * aff['energy_total']):.2e}")
        assert aff["energy_total"] > 0 and aff["eta2_total"] <= 1e-22 * 2 * aff["energy_total"], family


def test_vertex_order_does_not_matter(meshes):
    m = meshes["delaunay_beam(2)"]
    rng = np.random.default_rng(11)
    tets = m.tets.copy()
    pick = rng.choice(len(tets), len(tets) // 10, replace=False)
    perms = np.array([[1, 0, 2, 3], [0, 2, 1, 3], [1, 2, 0, 3], [3, 2, 1, 0], [2, 0, 3, 1]])  # odd and even
    for k, e in enumerate(pick):
        tets[e] = tets[e][perms[k % len(perms)]]
    S, N, O = (_t(rng.normal(size=(2, k, 6))) for k in (len(tets), len(m.points), len(tets)))
    out = []
    for cells in (m.tets, tets):
        with _rec(m.points, cells) as rec:
            out.append((_np(rec.error(S, nodal=N)), _np(rec.error(S, other=O))))
    for form in range(2):
        a, b = out[0][form], out[1][form]
        assert np.abs(a["eta2"] - b["eta2"]).max() <= 1e-13 * a["eta2"].max(), form
        assert np.abs(a["eta2_total"] - b["eta2_total"]).max() <= 1e-13 * a["eta2_total"].max(), form
        assert np.array_equal(a["eta2_argmax"], b["eta2_argmax"]), form


def test_repeatable_bits_column_independence_and_grouping(meshes):
    import torch

    m = meshes["delaunay_beam(2)"]
    rng = np.random.default_rng(13)
    nn, ne = len(m.points), len(m.tets)
    S, N, O = _t(rng.normal(size=(37, ne, 6))), _t(rng.normal(size=(37, nn, 6))), _t(rng.normal(size=(37, ne, 6)))
    dbl = NumpyEstimate(m.points, m.tets, LMD, MU)
    with _rec(m.points, m.tets) as rec:
        for kw in (dict(nodal=N), dict(other=O)):
            a, b = rec.error(S, **kw), rec.error(S, **kw)
            assert a["eta2"].shape == (37, ne) and a["eta2_argmax"].dtype == torch.int32
            for k in a:
                assert torch.equal(a[k], b[k]), k
            want = dbl.error(S.cpu().numpy(), **{k: v.cpu().numpy() for k, v in kw.items()})  # 37 columns: 16 + 16 + 5
            assert np.abs(a["eta2"].cpu().numpy() - want["eta2"]).max() <= 1e-12 * want["eta2"].max()
            assert np.array_equal(a["eta2_argmax"].cpu().numpy(), want["eta2_argmax"])
            for j in (0, 7, 15, 16, 36):  # alone or among 16 (or among the last 5): the same bits
                one = rec.error(S[j], **{k: v[j] for k, v in kw.items()})
                for k in a:
                    assert one[k].shape == a[k][j].shape and torch.equal(one[k], a[k][j]), (j, k)
            first16 = rec.error(S[:16], **{k: v[:16] for k, v in kw.items()})
            for k in a:
                assert torch.equal(first16[k], a[k][:16]), k
        # estimate() = element -> nodal -> error
        X = _t(rng.normal(size=(3, 3 * nn)))
        est = rec.estimate(X)
        el = rec.element(X)
        ref = rec.error(el["sigma"], nodal=rec.nodal(el["sigma"]))
        assert torch.equal(est["eta2"], ref["eta2"]) and torch.equal(est["eta2_total"], ref["eta2_total"])
        assert torch.equal(est["energy_total"], el["energy_total"])
        one = rec.estimate(X[1])
        assert one["eta2"].shape == (ne,) and torch.equal(one["eta2"], est["eta2"][1]) and one["relative"] == est["relative"][1]


def test_padded_and_unaligned_leading_dimensions(meshes):
    import torch

    m = meshes["structured_beam(2)"]
    nn, ne = len(m.points), len(m.tets)
    g = torch.Generator(DEV).manual_seed(5)
    with _rec(m.points, m.tets) as rec:
        for mc in (1, 5, 16):
            for pad_s, pad_o, pad_e, shift in ((7, 5, 3, 0), (8, 6, 4, 0), (8, 6, 4, 1)):  # odd, even, even off 16 bytes
                for nodal in (True, False):
                    rows = nn if nodal else ne
                    lds, ldo, lde = 6 * ne + pad_s, 6 * rows + pad_o, ne + pad_e
                    Sb = torch.rand(mc * lds + shift, dtype=torch.float64, device=DEV, generator=g) - 0.5
                    Ob = torch.rand(mc * ldo + shift, dtype=torch.float64, device=DEV, generator=g) - 0.5
                    S, Ot = Sb[shift:].view(mc, lds), Ob[shift:].view(mc, ldo)
                    Et = torch.full((mc, lde), 7.0, dtype=torch.float64, device=DEV)
                    T, M = (torch.full((mc,), 7.0, dtype=torch.float64, device=DEV) for _ in range(2))
                    A = torch.full((mc,), 7, dtype=torch.int32, device=DEV)
                    rec.error_raw(mc, S, lds, Ot if nodal else None, ldo, None if nodal else Ot, ldo, Et, lde, T, M, A)
                    torch.cuda.synchronize()
                    assert (Et[:, ne:] == 7.0).all()
                    Sc = S[:, :6 * ne].reshape(mc, ne, 6).contiguous()
                    Oc = Ot[:, :6 * rows].reshape(mc, rows, 6).contiguous()
                    ref = rec.error(Sc, nodal=Oc) if nodal else rec.error(Sc, other=Oc)
                    case = (mc, pad_s, shift, nodal)
                    assert torch.equal(Et[:, :ne], ref["eta2"]) and torch.equal(T, ref["eta2_total"]), case
                    assert torch.equal(M, ref["eta2_max"]) and torch.equal(A, ref["eta2_argmax"]), case
                    # every combination of NULL outputs
                    for mask in range(16):
                        outs = [torch.full_like(t, 9) for t in (Et, T, M, A)]
                        use = [o if mask >> i & 1 else None for i, o in enumerate(outs)]
                        rec.error_raw(mc, S, lds, Ot if nodal else None, ldo, None if nodal else Ot, ldo, use[0], lde, *use[1:])
                        torch.cuda.synchronize()
                        for i, (o, want, k) in enumerate(zip(outs, (Et, T, M, A), (ne, mc, mc, mc))):
                            if mask >> i & 1:
                                assert torch.equal(o[..., :k], want[..., :k]) and (o[..., k:] == 9).all(), (case, mask, i)
                            else:
                                assert (o == 9).all(), (case, mask, i)


def test_validation(meshes):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    m = meshes["structured_beam(2)"]
    nn, ne = len(m.points), len(m.tets)
    S = torch.zeros(6 * ne, dtype=torch.float64, device=DEV)
    N = torch.zeros(6 * nn, dtype=torch.float64, device=DEV)
    O = torch.zeros(6 * ne, dtype=torch.float64, device=DEV)
    Et = torch.full((ne,), 9.0, dtype=torch.float64, device=DEV)
    with _rec(m.points, m.tets) as rec:
        ok = dict(m=1, sigma_elem=S, ld_sigma=6 * ne, sigma_node=N, ld_node=6 * nn, eta2=Et, ld_eta=ne)
        other = dict(m=1, sigma_elem=S, ld_sigma=6 * ne, sigma_other=O, ld_other=6 * ne, eta2=Et, ld_eta=ne)
        for bad, msg in ((dict(ok, m=0), "m = 0"), (dict(ok, m=17), "m = 17"),
                         (dict(ok, sigma_other=O, ld_other=6 * ne), "both"),
                         (dict(ok, sigma_node=None), "neither"), (dict(ok, sigma_elem=None), "sigma_elem_dev"),
                         (dict(ok, ld_sigma=6 * ne - 1), "ld_sigma"), (dict(ok, ld_node=6 * nn - 1), "ld_node"),
                         (dict(other, ld_other=6 * ne - 1), "ld_other"), (dict(ok, ld_eta=ne - 1), "ld_eta"),
                         (dict(other, ld_eta=ne - 1), "ld_eta"),
                         # refused with every output NULL too: the checks come before the no-op
                         (dict(m=0, sigma_elem=S, ld_sigma=6 * ne, sigma_node=N, ld_node=6 * nn), "m = 0"),
                         (dict(m=1, sigma_elem=S, ld_sigma=6 * ne), "neither")):
            with pytest.raises(_lib.SaaError, match=msg) as ei:
                rec.error_raw(**bad)
            assert ei.value.code == _lib.SAA_E_ARG, msg
        torch.cuda.synchronize()
        assert (Et == 9.0).all()  # nothing was launched
        # all outputs NULL: a no-op; a leading dimension that goes with a NULL pointer is not looked at
        rec.error_raw(1, S, 6 * ne, N, 6 * nn)
        rec.error_raw(16, S, 6 * ne, None, 0, O, 6 * ne)
        rec.error_raw(**dict(ok, eta2=None, ld_eta=0))
        torch.cuda.synchronize()
        assert (Et == 9.0).all()
        with pytest.raises(ValueError, match="exactly one"):
            rec.error(S.view(ne, 6))
        with pytest.raises(ValueError, match="exactly one"):
            rec.error(S.view(ne, 6), nodal=N.view(nn, 6), other=O.view(ne, 6))
        with pytest.raises(ValueError, match="expected nodal"):
            rec.error(S.view(ne, 6), nodal=O.view(ne, 6))
        with pytest.raises(ValueError, match="element stresses"):
            rec.error(N.view(nn, 6), other=O.view(ne, 6))


def _prepare_worker(rank, world, port, out_dir, n, steps):
    import torch
    import torch.distributed as dist

    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    drivers.data_prepare(structured_beam(n), steps, 1, out_dir, rank, world)
    dist.barrier()
    dist.destroy_process_group()


def _close(a, b, path="report"):
    """Two reports agree: same structure, integers and strings equal, floats to 1e-11 relative."""
    if isinstance(b, dict):
        assert isinstance(a, dict) and set(a) == set(b), path
        for k in b:
            _close(a[k], b[k], f"{path}.{k}")
    elif isinstance(b, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _close(x, y, f"{path}[{i}]")
    elif isinstance(b, float):
        assert abs(a - b) <= 1e-11 * abs(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_cli_estimate_on_a_two_rank_tree_of_data_prepare(tmp_path):
    """400 steps, so that the stress wave from the clamp has crossed the slab interface.  Before it arrives the body there
    moves almost rigidly: its strain is a difference of nearly equal displacements, and round-off of the displacement
    alone (relative 2e-16) moves the interface sums by 2e-6 relative after 40 steps, against 4e-14 after 200 or 400
    (NumPy double on the oracle's trajectory), which is what a comparison to 1e-11 needs."""
    import torch.multiprocessing as mp

    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam
    from stress_double import parse_vtk

    n, steps = 2, 400
    mp.spawn(_prepare_worker, args=(2, free_port(), str(tmp_path), n, steps), nprocs=2, join=True)
    rng = np.random.default_rng(9)
    for r in range(2):  # a modelled run: the synchronised one, disturbed
        truth = np.asarray(rio.load_displacement(os.path.join(tmp_path, drivers.PATHS["truth"].format(r=r))))
        assert truth.shape[1] == steps
        rio.save_displacement(os.path.join(tmp_path, drivers.PATHS["modeled"].format(r=r)),
                              truth * (1.0 + 1e-3 * rng.normal(size=truth.shape)))
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", "estimate", "--synthetic", str(n),
           "--columns", "0,-1", "--modeled", "--out", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    rep = json.loads(lines[0])
    ref = drivers.estimate(structured_beam(n), str(tmp_path), [0, -1], modeled=True, vtk=False, recovery=NumpyEstimate)
    assert rep["n_ranks"] == 2 and [c["column"] for c in rep["columns"]] == [0, steps - 1]
    last = rep["columns"][1]
    assert last["eta"] > 0 and 0 < last["relative"] < 1 and last["model_error"] > 0
    assert len(rep["files"]) == 2
    for path, c in zip(rep["files"], rep["columns"]):
        f = parse_vtk(path)
        assert list(f["cell_data"]) == ["eta2", "error-density", "model-error2"] and len(f["cell_data"]["eta2"]) == rep["n_elems"]
        assert np.isclose(np.sqrt(f["cell_data"]["eta2"].sum()), c["eta"], rtol=1e-12)
        assert f["cell_data"]["eta2"].max() == c["eta2_max"] and int(np.argmax(f["cell_data"]["eta2"])) == c["element"]
    rep["files"] = []
    _close(rep, json.loads(json.dumps(ref)))
