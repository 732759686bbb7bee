"""The block tangent apply ``saa_operator_tangent_apply_block`` (``csrc/saa_optan_block.hip``) and what is built on it - the
natural frequencies of a loaded structure about its equilibrium, ``modal.prestressed_modes`` / ``prestressed_report`` / ``drivers
modal --material`` - on the MI355X, against the doubles of tests/tangent_double.py (longdouble element pass) and
tests/prestress_double.py (dense ``K_T``, dense mass, ``eigh``; tests/test_prestress.py qualifies it on the CPU).

The bar of the block is that of the one-column tangent: ``err = max|y - r| / max|r| <= 1e-12 + 8 env``.  The meshes have at most
288 elements, except that of the driver run, which the driver builds itself."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import operator_extended as ox
import prestress_double as pd
import tangent_double as td

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMD, MU = fd.lame(fd.E, fd.NU)
SENTINEL = -7.25e300
# what `drivers modal --order 2` printed before it knew a material, key for key (modal.modal_report_p2)
P2_KEYS = {"order", "n_nodes", "n_elems", "n_free_dofs", "frequencies_hz", "residuals", "modes_converged", "outer_iterations",
           "inner_iterations", "seconds"}
REPORT_KEYS = {"order", "n_nodes", "n_elems", "n_free_dofs", "material", "load", "newton", "stable", "lowest_ritz", "n_inverted",
               "frequencies_hz", "residuals", "modes_converged", "frequencies_hz_unstressed", "residuals_unstressed", "omega2_ratio",
               "outer_iterations", "inner_iterations", "outer_iterations_unstressed", "inner_iterations_unstressed", "seconds"}
NEWTON_KEYS = {"converged", "residual", "newton_iterations", "cg_iterations", "load_steps", "n_inverted", "tip_deflection",
               "min_det_f"}


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(t):
    return t.cpu().numpy()


def _operator(case):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(case["points"], np.asarray(case["cells"]).astype(np.int32), np.asarray(case["dd"]).astype(np.int32),
                         case["lmd"], case["mu"], fd.RHO)


def _mesh_operator(name):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    pts, cells, dd = fd.mesh(name)
    return ModalOperator(pts, cells.astype(np.int32), dd.astype(np.int32), LMD, MU, fd.RHO)


def _raw_block(op, material, u, V, pad=7, tail=64):
    """One library call on the ``(m, n)`` block ``V`` with leading dimensions ``n + pad``: ``(KV (m, n), padding intact)``."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    m, n = V.shape
    ld = n + pad
    vin = torch.zeros((m, ld), dtype=torch.float64, device="cuda")
    vin[:, :n] = V
    out = torch.full((m * ld + tail,), SENTINEL, dtype=torch.float64, device="cuda")
    n_inv = C.c_int64(-1)
    _lib.check(op._lib.saa_operator_tangent_apply_block(op._h, _lib.material_id(material), C.c_void_p(u.data_ptr()), m,
                                                        C.c_void_p(vin.data_ptr()), ld, C.c_void_p(out.data_ptr()), ld,
                                                        C.byref(n_inv)))
    body = out[:m * ld].reshape(m, ld)
    intact = bool((body[:, n:] == SENTINEL).all()) and bool((out[m * ld:] == SENTINEL).all())
    return body[:, :n].clone(), intact, int(n_inv.value)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", td.case_ids(), ids=fx.case_name)
def test_block_is_within_the_bar(cid, material):
    case, _, _ = td.reference(cid)
    with _operator(case) as op:
        V = _dev(np.stack([case["v_" + d] for d in td.DIRECTIONS]))
        KV, n_inv = op.tangent_apply_block(_dev(case["u"]), V, material, count=True)
        got = {d: _host(KV[j]) for j, d in enumerate(td.DIRECTIONS)}
    assert n_inv == 0
    _, bad = td.check(got, cid, material, ox.KERNEL_FACTOR)
    assert not bad, bad
    for d in td.DIRECTIONS:
        assert not got[d][case["dd"]].any()


# ---- 2. column independence and shapes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_a_column_does_not_depend_on_its_call(name, material):
    import torch

    cid = (name, "strain", 0, 0.3)
    case, _, env = td.reference(cid)
    bar = ox.TOL + ox.KERNEL_FACTOR * float(max(e.max() for e in env[material].values()))
    n = 3 * len(case["points"])
    V = _dev(np.random.default_rng(11).uniform(-1.0, 1.0, size=(16, n)))
    with _operator(case) as op:
        u = _dev(case["u"])
        runs = {}
        for m in (1, 5, 16):
            runs[m], intact, n_inv = _raw_block(op, material, u, V[:m])
            assert intact and n_inv == 0, (m, intact, n_inv)
        assert torch.equal(runs[1][0], runs[16][0]) and torch.equal(runs[5], runs[16][:5])
        perm = torch.as_tensor(np.random.default_rng(12).permutation(16), device="cuda")
        shuffled, intact, _ = _raw_block(op, material, u, V[perm])
        assert intact and torch.equal(shuffled, runs[16][perm])
        again, intact, _ = _raw_block(op, material, u, V)
        assert intact and torch.equal(again, runs[16])
        assert not _host(runs[16])[:, case["dd"]].any()
        worst = 0.0
        for j in range(16):
            one = op.tangent_apply(u, V[j].contiguous(), material)
            worst = max(worst, float((runs[16][j] - one).abs().max() / one.abs().max()))
    print(f"{name} {material}: block against the one-column entry, worst {worst:.2e}, allowed {bar:.2e}")
    assert worst <= bar


# ---- 3. launch edges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_elems", (1, 255, 256, 257))
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_launch_edges_with_sixteen_columns(name, n_elems):
    import torch

    case = td.sub_case(td.build_case((name, "strain", 0, 0.3)), n_elems)
    assert len(case["cells"]) == n_elems
    for material in fd.MATERIALS:
        ref, inv, _ = td.outputs(case, material)
        assert not inv.any()
        env = td.envelope(case, ref, lambda c: td.outputs(c, material)[0])
        V = _dev(np.stack([case["v_" + td.DIRECTIONS[j % 2]] for j in range(16)]))
        with _operator(case) as op:
            KV, intact, n_inv = _raw_block(op, material, _dev(case["u"]), V)
        assert intact and n_inv == 0
        for j in range(2, 16):
            assert torch.equal(KV[j], KV[j % 2]), (material, j)
        got = {d: _host(KV[j])[None] for j, d in enumerate(td.DIRECTIONS)}
        _, bad = ox.check(got, ref, env, ox.KERNEL_FACTOR, f"{name}[:{n_elems}] {material}", names=list(td.DIRECTIONS))
        assert not bad, bad


@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_more_rows_than_a_call_takes(name):
    import torch

    case = td.build_case((name, "strain", 0, 0.3))
    n = 3 * len(case["points"])
    V = _dev(np.random.default_rng(13).uniform(-1.0, 1.0, size=(33, n)))
    with _operator(case) as op:
        u = _dev(case["u"])
        for material in fd.MATERIALS:
            rows = torch.stack([op.tangent_apply_block(u, V[j], material) for j in range(33)])
            for m in (17, 33):
                assert torch.equal(op.tangent_apply_block(u, V[:m], material), rows[:m]), (material, m)


# ---- 4. the linear material -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fd.MESHES)
def test_linear_material_is_the_apply_bit_for_bit(name):
    import torch

    case = td.build_case((name, "strain", 0, 0.3))
    n = 3 * len(case["points"])
    V = _dev(np.random.default_rng(14).uniform(-1.0, 1.0, size=(19, n)))
    with _operator(case) as op:
        want = op.apply(V)[0]
        assert torch.equal(op.tangent_apply_block(None, V, "linear"), want)
        KV, n_inv = op.tangent_apply_block(_dev(case["u"]), V, "linear", count=True)
        assert torch.equal(KV, want) and n_inv == 0
        assert torch.equal(op.tangent_apply_block(None, V[3], "linear"), want[3])
        for material in fd.MATERIALS:
            with pytest.raises(ValueError):
                op.tangent_apply_block(None, V, material)


# ---- 5. inversion ---------------------------------------------------------------------------------------------------------------

def test_inverted_elements_are_dropped_from_every_column_and_counted_once():
    import torch

    pts, cells, dd = fd.mesh("curved288")
    fs = td.Tangent(pts, cells, LMD, MU, dd)
    _, u, star = fd.inversion_state(fs, pts, 0.02 * fd.smooth_random_field(pts, 3))
    case = {"points": pts, "cells": cells, "dd": dd, "lmd": LMD, "mu": MU, "u": u,
            "v_random": np.random.default_rng(5).uniform(-1.0, 1.0, size=u.size), "v_smooth": fd.smooth_random_field(pts, 6)}
    ref, inv, _ = td.outputs(case, "neo_hookean")
    assert inv[star].all() and 0 < inv.sum() < len(cells)

    def outputs_of(c):
        out, alt_inv, _ = td.outputs(c, "neo_hookean")
        assert (alt_inv == inv).all()
        return out

    env = td.envelope(case, ref, outputs_of)
    V = _dev(np.stack([case["v_random"], case["v_smooth"], case["v_random"]]))
    with _operator(case) as op:
        ud = _dev(u)
        KV, n_inv = op.tangent_apply_block(ud, V, "neo_hookean", count=True)
        n_one = op.tangent_apply(ud, V[0].contiguous(), "neo_hookean", count=True)[1]
        n_svk = op.tangent_apply_block(ud, V, "svk", count=True)[1]
    print("inverted in the double", int(inv.sum()), "block", n_inv, "one column", n_one)
    assert n_inv == n_one == int(inv.sum()) and n_svk == 0
    assert bool(torch.isfinite(KV).all()) and torch.equal(KV[2], KV[0])
    _, bad = ox.check({d: _host(KV[j])[None] for j, d in enumerate(td.DIRECTIONS)}, ref, env, ox.KERNEL_FACTOR,
                      "curved288 inversion, block", names=list(td.DIRECTIONS))
    assert not bad, bad


# ---- 6. symmetry ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_block_tangent_is_symmetric(name, material):
    import torch

    cid = (name, "strain", 0, 0.3)
    case, _, env = td.reference(cid)
    bar = ox.TOL + ox.KERNEL_FACTOR * float(max(e.max() for e in env[material].values()))
    n = 3 * len(case["points"])
    rng = np.random.default_rng(15)
    with _operator(case) as op:
        u = _dev(case["u"])
        V, W = _dev(rng.uniform(-1.0, 1.0, size=(4, n))) * op.free, _dev(rng.uniform(-1.0, 1.0, size=(4, n))) * op.free
        KV, KW = op.tangent_apply_block(u, V, material), op.tangent_apply_block(u, W, material)
        A, B = V @ KW.T, (W @ KV.T).T                                   # V K_T W^T, formed from either side
        scale = torch.linalg.vector_norm(V, dim=1)[:, None] * torch.linalg.vector_norm(KW, dim=1)[None, :]
        worst = float(((A - B).abs() / scale).max())
    print(name, material, f"|v.Kw - w.Kv| / (|v| |Kw|) <= {worst:.2e}, allowed {2 * bar:.2e}")
    assert worst <= 2.0 * bar


# ---- 7. prestressed modes against the dense double ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gpu_unstressed(name):
    from synchronization_avoiding_algorithms_amd.modal import device_lowest_modes

    pts, cells, _ = fd.mesh(name)
    with _mesh_operator(name) as op:
        out = device_lowest_modes(op, pts, cells.astype(np.int32), LMD, MU, 4)
    assert out["converged"]
    return out["omega2"]


@pytest.mark.parametrize("fx_load", pd.FX, ids=("compression", "tension"))
@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", pd.MESHES)
def test_prestressed_modes_against_the_dense_double(name, material, fx_load):
    from synchronization_avoiding_algorithms_amd.modal import prestressed_modes

    u = pd.equilibrium(name, material, fx_load)[0]
    want, w0 = pd.prestressed(name, material, fx_load)[:4], pd.unstressed(name)
    with _mesh_operator(name) as op:
        got = prestressed_modes(op, u, material, k=4)
    assert got["stable"] is True and got["converged"] and got["n_inverted"] == 0 and got["material"] == material
    err = float(np.abs(got["omega2"] / want - 1.0).max())
    ratio, dense = float(got["omega2"][0] / _gpu_unstressed(name)[0]), float(want[0] / w0[0])
    print(f"{name} {material} fx {fx_load:+.0f}: {got['outer_iterations']} sweeps, {got['inner_iterations']} inner iterations, "
          f"residuals {got['residuals'].max():.1e}, omega^2 against eigh {err:.1e}, ratio {ratio:.6f} (dense {dense:.6f})")
    assert got["residuals"].max() <= 1e-8 and err <= 1e-8
    assert (ratio < 1.0) == (fx_load < 0) and abs(ratio - dense) <= 1e-6
    assert np.allclose(got["frequencies_hz"], np.sqrt(got["omega2"]) / (2.0 * np.pi), rtol=1e-15)


# ---- 8. the unstable state ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", pd.MESHES)
def test_an_unstable_state_is_answered_not_raised(name, material):
    """``3 u*(fx = -2000)``: finite, uninverted (``det F >= 0.97``), and the tangent has negative eigenvalues."""
    from synchronization_avoiding_algorithms_amd.modal import prestressed_modes

    u, w = pd.unstable(name, material)
    with _mesh_operator(name) as op:
        got = prestressed_modes(op, u, material, k=4)
    print(f"{name} {material}: lowest_ritz {got['lowest_ritz']:.3f} (dense lowest {w[0]:.3f}) after {got['outer_iterations']} sweeps, "
          f"{got['inner_iterations']} inner iterations")
    assert got["stable"] is False and got["converged"] is False and got["frequencies_hz"] is None and got["n_inverted"] == 0
    assert np.isfinite(got["lowest_ritz"]) and got["lowest_ritz"] < 0 and got["lowest_ritz"] >= w[0] - 1e-8 * abs(w[0])


# ---- 9. the whole path ----------------------------------------------------------------------------------------------------------

def test_prestressed_report_on_the_compressed_beam():
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes
    from synchronization_avoiding_algorithms_amd.modal import prestressed_report

    pts, cells, _ = fd.mesh("beam36")
    rep = prestressed_report(pts, cells.astype(np.int32), plane_nodes(pts), "svk", load=(-2000.0, 0.0, 0.0), k=4, load_steps=4,
                             E=fd.E, nu=fd.NU, rho=fd.RHO)
    assert set(rep) == REPORT_KEYS and set(rep["newton"]) == NEWTON_KEYS
    dense = float(pd.prestressed("beam36", "svk", -2000.0)[0] / pd.unstressed("beam36")[0])
    diff = abs(rep["omega2_ratio"][0] - dense)
    print(rep["newton"], f"ratio {rep['omega2_ratio'][0]:.8f}, dense {dense:.8f}, difference {diff:.2e}")
    assert rep["order"] == 2 and rep["newton"]["converged"] and rep["newton"]["residual"] <= 1e-8 and rep["newton"]["load_steps"] == 4
    assert rep["newton"]["min_det_f"] >= 0.99 and rep["stable"] is True and rep["modes_converged"]
    assert diff <= 1e-5 and len(rep["frequencies_hz"]) == 4 and max(rep["residuals"]) <= 1e-8


# ---- 10. the driver -------------------------------------------------------------------------------------------------------------

def _driver(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=str(cwd),
                          capture_output=True, text=True, timeout=300, env=env)


def test_driver_modal_with_a_material_and_without(tmp_path):
    """``--fx 200`` on the 25 : 1 beam is tension at a root strain of 200 * 25 / E = 0.5 %; the double's Newton on the 25 x 1 x 1
    stand-in of that beam converges there to 1e-12 in one load step."""
    base = ["modal", "--synthetic", "2", "--order", "2", "--k", "3"]
    out = _driver(base + ["--material", "svk", "--fx", "200"], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print({k: v for k, v in res.items() if k != "seconds"})
    assert set(res) == REPORT_KEYS and set(res["newton"]) == NEWTON_KEYS
    assert res["order"] == 2 and res["material"] == "svk" and res["load"] == [200.0, -0.5, -0.5]
    assert res["newton"]["converged"] is True and res["stable"] is True
    assert len(res["omega2_ratio"]) == 3 and all(r > 1.0 for r in res["omega2_ratio"])
    plain = _driver(base, tmp_path)
    assert plain.returncode == 0, plain.stderr[-3000:]
    old = json.loads(plain.stdout.strip().splitlines()[-1])
    assert set(old) == P2_KEYS and set(old["seconds"]) == {"operator_create", "lowest_modes"}
    assert np.allclose(old["frequencies_hz"], res["frequencies_hz_unstressed"], rtol=1e-7)
