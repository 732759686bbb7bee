"""The extended-precision reference of the operator kernels (tests/operator_extended.py) checked on the CPU:

* the longdouble run against the same statements in mpmath at 50 digits, on four elements per family and order, to 2^-58 of
  each field's maximum (NumPy routines that accept longdouble are not trusted until checked);
* its float64 run against the older NumPy doubles at ``nu = 0.3`` (other formulas: ``inv(D)``, ``einsum``, ``np.linalg``);
* the two conditions under which the bar ``err <= 1e-12 + 8 env`` of tests/test_gpu_operator_extended.py means something,
  on every case: the stable float64 restatement stays within ``1e-12 + 2 env``, and ``env <= 1e-6``;
* that the bar has teeth: the float64 restatement with the two forms the kernels used to have FAILS it for von Mises and
  for ``eta^2`` at ``nu = 0.499999``, and passes at ``nu = 0.3``."""
import numpy as np
import pytest

import operator_extended as ox

MP_CASES = [("structured2", "nu", 0.499999), ("curved288", "nu", 0.499999), ("delaunay2", "shift", 20),
            ("curved288", "shift", 20), ("delaunay2", "needle", 1e-3), ("beam36", "needle", 1e-3),
            ("structured2", "sliver", 1e-6), ("straight288", "sliver", 1e-6), ("beam36", "curved", 0.2)]


@pytest.mark.parametrize("cid", MP_CASES, ids=ox.case_name)
def test_longdouble_matches_mpmath_at_50_digits(cid):
    import mpmath

    case = ox.sub_case(ox.build_case(cid), 4, 2)
    with mpmath.workdps(50):
        want = ox.outputs(case, ox.MP)
        got = ox.outputs(case, np.longdouble)
        worst = {}
        for name, w in want.items():
            if name in ox.ARG_OF:
                assert (np.asarray(w, dtype=np.int64) == got[name]).all(), name
                continue
            diff = np.abs(ox.conv(got[name], ox.MP) - w)
            worst[name] = float(diff.max() / np.abs(w).max())
    print(ox.case_name(cid), {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= 2.0 ** -58, worst


def test_stable_restatement_matches_the_older_doubles_at_order_2():
    import p2_double as p2
    import p2_stress_double as psd

    case = ox.build_case(("curved288", "nu", 0.3))
    pts, cells, lmd, mu, rho = (case[k] for k in ("points", "cells", "lmd", "mu", "rho"))
    got = ox.outputs(case, np.float64)
    ns = psd.NumpyQuadraticStress(pts, cells, lmd, mu)
    want = dict(ns.element(case["X"]))
    want["kx"], want["mx"] = p2.apply_k(pts, cells, (), lmd, mu, case["X"]), p2.apply_m(pts, cells, (), rho, case["X"])
    want["load"] = p2.load(pts, cells, (), case["force"])
    want["diag_k"], want["diag_m"] = p2.diagonals(pts, cells, (), lmd, mu, rho)
    want["nodal"] = ns.nodal(case["sig"])
    for tag, res in (("zz", ns.error(case["sig"], nodal=case["nod"])), ("other", ns.error(case["sig"], other=case["sig_other"])),
                     ("press", ns.error(case["psig"], nodal=case["pnod"]))):
        want.update({f"{tag}.{k}": v for k, v in res.items()})
    _compare(got, want)


def test_stable_restatement_matches_the_older_doubles_at_order_1():
    from estimate_double import NumpyEstimate

    case = ox.build_case(("delaunay2", "nu", 0.3))
    pts, cells, lmd, mu, rho = (case[k] for k in ("points", "cells", "lmd", "mu", "rho"))
    got = ox.outputs(case, np.float64)
    ns = NumpyEstimate(pts, cells, lmd, mu)
    want = dict(ns.element(case["X"]))
    want["nodal"] = ns.nodal(case["sig"])
    for tag, res in (("zz", ns.error(case["sig"], nodal=case["nod"])), ("other", ns.error(case["sig"], other=case["sig_other"])),
                     ("press", ns.error(case["psig"], nodal=case["pnod"]))):
        want.update({f"{tag}.{k}": v for k, v in res.items()})
    # consistent mass rho V / 20 (1 + delta_ab), load f V / 4, diag M rho V / 10 (the closed forms of the linear element)
    n = len(pts)
    U = case["X"].reshape(len(case["X"]), n, 3)[:, cells]
    mx, load, dm = np.zeros((len(U), n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for a in range(4):
        np.add.at(mx, (slice(None), cells[:, a]), rho * ns.vol[None, :, None] / 20.0 * (U[:, :, a] + U.sum(axis=2)))
        np.add.at(load, cells[:, a], ns.vol[:, None] / 4.0 * case["force"][None, :])
        np.add.at(dm, cells[:, a], rho * ns.vol[:, None] / 10.0 * np.ones(3))
    want["mx"], want["load"], want["diag_m"] = mx.reshape(len(U), -1), load.reshape(-1), dm.reshape(-1)
    _compare(got, want)
    # K through the energy: x . K x / 2 = sum_e W_e, and its diagonal through unit vectors of three nodes
    half = 0.5 * (case["X"] * got["kx"]).sum(axis=1)
    assert np.abs(half / got["energy_total"] - 1.0).max() < 1e-12
    sub = dict(case)
    sub["X"] = np.eye(3 * n)[[0, 3 * (n // 2) + 1, 3 * n - 1]]
    kx = ox.Extended(pts, cells, lmd, mu, rho, np.float64).apply_k(sub["X"])
    for row, d in zip(kx, (0, 3 * (n // 2) + 1, 3 * n - 1)):
        assert abs(row[d] / got["diag_k"][d] - 1.0) < 1e-12


def _compare(got, want):
    errs = {}
    for name, w in want.items():
        if name in ox.ARG_OF:
            f = ox.ARG_OF[name]
            flat = np.asarray(want[f]).reshape(len(w), -1)
            assert (flat[np.arange(len(w)), np.asarray(got[name])] >= flat.max(axis=1) * (1 - 1e-12)).all(), name
            continue
        errs[name] = float(ox.errors(name, got[name], np.asarray(w, dtype=np.longdouble)).max())
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-12, errs


@pytest.mark.parametrize("cid", ox.case_ids(), ids=ox.case_name)
def test_the_bar_is_meaningful_on_this_case(cid):
    case, ref, env = ox.reference(cid)
    worst, bad = ox.check(ox.outputs(case, np.float64), ref, env, ox.STABLE_FACTOR, ox.case_name(cid))
    assert not bad, bad                                               # the stable restatement: 1e-12 + 2 env
    top = {k: float(v.max()) for k, v in env.items()}
    assert max(top.values()) <= ox.ENV_MAX, top


@pytest.mark.parametrize("cid", ox.bound_case_ids(), ids=ox.case_name)
def test_the_element_bound_reference(cid):
    case, ref, env = ox.bound_reference(cid)
    err = float(np.abs(ox.element_omega(case, np.float64) - ref).max() / ref.max())
    true = ox.omega_true(case)
    print(ox.case_name(cid), f"err {err:.2e} env {env:.2e} omega_true / max omega_e {true / ref.max():.6f}")
    assert err <= ox.TOL + ox.STABLE_FACTOR * env and env <= ox.ENV_MAX
    assert ref.max() >= (1 - 1e-12) * true                            # Irons-Treharne holds for the reference itself


@pytest.mark.parametrize("mesh", ox.MESHES)
def test_the_bar_has_teeth(mesh):
    """The forms the kernels had before fail at nu = 0.499999 and pass at nu = 0.3: the tests can fail, and for that reason."""
    names = ["von_mises", "zz.eta2", "other.eta2", "press.eta2"]
    case, ref, env = ox.reference((mesh, "nu", 0.499999))
    worst, bad = ox.check(ox.outputs(case, np.float64, kernel_order=True), ref, env, ox.KERNEL_FACTOR, f"{mesh} kernel order",
                          names=names)
    assert sorted(b[0] for b in bad) == sorted(names), bad
    for name in names:
        assert worst[name][0] > 10.0 * (ox.TOL + ox.KERNEL_FACTOR * worst[name][1]), (name, worst[name])  # and not narrowly
    case, ref, env = ox.reference((mesh, "nu", 0.3))
    _, bad = ox.check(ox.outputs(case, np.float64, kernel_order=True), ref, env, ox.KERNEL_FACTOR, f"{mesh} kernel order",
                      names=names)
    assert not bad, bad
