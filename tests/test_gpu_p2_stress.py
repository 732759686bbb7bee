"""Stress recovery and error estimate of quadratic tetrahedra on the GPU (csrc/saa_stress_p2.hip) against the NumPy double
(tests/p2_stress_double.py).

Meshes: the reference's 288-element / 625-node fixture, straight and curved (two workgroups, the second partial); the
36-element beam (one partial workgroup); ``to_quadratic(delaunay_beam(2))`` (node valences into the forties: long CSR rows);
``to_quadratic(structured_beam(8))`` (76 800 elements: more than 256 partials into the final reduction; totals, maxima and
argmaxima only).

Bars: every output to 1e-12 of its field's maximum (fp64 with sums of at most some tens of terms; the double orders its sums
differently).  ``energy_total`` against ``x . K x / 2`` of the same handle to 1e-12.  Patch test and cubic-field rates as in
tests/test_p2_stress.py.  Repeatability, column independence and grouping are bitwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden

import p2_stress_double as psd
from estimate_double import quadratic_field

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-12


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _rec(points, cells10, lmd, mu, **kw):
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery

    return QuadraticStressRecovery(points, cells10, lmd, mu, **kw)


def _err(got, want):
    want = np.asarray(want, dtype=np.float64)
    top = np.abs(want).max()
    return np.abs(np.asarray(got.cpu() if hasattr(got, "cpu") else got, dtype=np.float64) - want).max() / (top if top > 0 else 1.0)


@pytest.fixture(scope="module")
def cases():
    """name -> (points, cells10, lmd, mu, the double, X (16, n_dof), the double's element fields of X), made once."""
    from synchronization_avoiding_algorithms_amd.fem_setup import lame
    from synchronization_avoiding_algorithms_amd.mesh import delaunay_beam, structured_beam, to_quadratic

    g = load_golden("p2_beam.npz")
    lmd, mu = float(g["lmd"]), float(g["mu"])
    b36, dl = to_quadratic(structured_beam(1, length=6.0)), to_quadratic(delaunay_beam(2))
    meshes = {"straight288": (g["points_straight"], g["cells10"]), "curved288": (g["points_curved"], g["cells10"]),
              "beam36": (b36.points, b36.tets10), "delaunay2": (dl.points, dl.tets10)}
    out = {}
    for i, (name, (pts, c10)) in enumerate(meshes.items()):
        ns = psd.NumpyQuadraticStress(pts, c10, lmd, mu)
        X = np.random.default_rng(40 + i).uniform(-0.5, 0.5, size=(16, 3 * len(pts))) * 1e-3
        out[name] = (pts, c10, lmd, mu, ns, X, ns.element(X))
    out["lame"] = lame(1e6, 0.3)
    return out


NAMES = ("straight288", "curved288", "beam36", "delaunay2")


@pytest.mark.parametrize("m", (1, 5, 16))
@pytest.mark.parametrize("name", NAMES)
def test_every_output_matches_the_double(cases, name, m):
    pts, c10, lmd, mu, ns, X, want = cases[name]
    ne = len(c10)
    with _rec(pts, c10, lmd, mu) as rec:
        el = rec.element(_dev(X[:m]))
        nodal = rec.nodal(el["sigma"])
        zz = rec.error(el["sigma"], nodal=nodal)
        other = rec.element(_dev(X[::-1][:m].copy()))["sigma"]
        df = rec.error(el["sigma"], other=other)
        same = rec.error(el["sigma"], other=el["sigma"].clone())
    errs = {k: _err(el[k], want[k][:m]) for k in ("sigma", "von_mises", "energy", "energy_total", "von_mises_max")}
    assert el["sigma"].shape == (m, ne, 4, 6) and el["von_mises"].shape == (m, ne, 4) and el["energy"].shape == (m, ne)
    # the argmax is a point index 4 e + q; the double's value there is its maximum (last-bit ties aside)
    arg = el["von_mises_argmax"].cpu().numpy().astype(np.int64)
    flat = want["von_mises"][:m].reshape(m, -1)
    assert ((0 <= arg) & (arg < 4 * ne)).all()
    assert (flat[np.arange(m), arg] >= flat.max(axis=1) * (1.0 - TOL)).all()
    sig = want["sigma"][:m]
    want_nodal = ns.nodal(sig)
    errs["nodal"] = _err(nodal, want_nodal)
    want_zz = ns.error(sig, nodal=want_nodal)
    want_df = ns.error(sig, other=ns.element(X[::-1][:m])["sigma"])
    for tag, got, ref in (("zz", zz, want_zz), ("other", df, want_df)):
        for k in ("eta2", "eta2_total", "eta2_max"):
            errs[f"{tag}.{k}"] = _err(got[k], ref[k])
        a = got["eta2_argmax"].cpu().numpy().astype(np.int64)
        assert (ref["eta2"][np.arange(m), a] >= ref["eta2_max"] * (1.0 - 1e-10)).all(), tag
    print(name, m, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs
    for k in ("eta2", "eta2_total", "eta2_max"):
        assert not same[k].any(), k                                   # a field against itself: exactly 0
    assert not same["eta2_argmax"].any()


@pytest.mark.parametrize("name", ("curved288", "delaunay2"))
def test_energy_total_is_half_x_k_x_of_the_same_handle(cases, name):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    pts, c10, lmd, mu, _, X, _ = cases[name]
    with ModalOperator(pts, c10, (), lmd, mu, 1.0) as op:
        rec = _rec(None, None, None, None, operator=op)
        Xd = _dev(X[:5])
        W = rec.element(Xd, sigma=False, von_mises=False, energy=False)["energy_total"].cpu().numpy()
        KX, _ = op.apply(Xd)
        want = 0.5 * (Xd * KX).sum(dim=1).cpu().numpy()
        rec.close()
        assert op._h.value                                             # a borrowed operator is not closed
    print(name, "W / (x.Kx/2) - 1", W / want - 1.0)
    assert np.abs(W / want - 1.0).max() < 1e-12


@pytest.mark.parametrize("n", (1, 2))
def test_patch_test(cases, n):
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic

    lmd, mu = cases["lame"]
    quad = to_quadratic(structured_beam(n, length=6.0))
    ns = psd.NumpyQuadraticStress(quad.points, quad.tets10, lmd, mu)
    u, exact = quadratic_field(quad.points, ns.D)
    _, at_gauss = quadratic_field(ns.gauss_positions().reshape(-1, 3), ns.D)
    with _rec(quad.points, quad.tets10, lmd, mu) as rec:
        el = rec.element(_dev(u))
        nodal = rec.nodal(el["sigma"])
        est = rec.estimate(_dev(u))
    top = np.abs(exact).max()
    e_gauss = np.abs(el["sigma"].cpu().numpy().reshape(-1, 6) - at_gauss).max() / top
    e_nodal = np.abs(nodal.cpu().numpy() - exact).max() / top
    eta2, W = float(est["eta2_total"]), float(est["energy_total"])
    print(f"n = {n}: Gauss {e_gauss:.2e} nodal {e_nodal:.2e} eta2 / 2W {eta2 / (2 * W):.2e}")
    assert el["sigma"].shape == (len(quad.tets10), 4, 6) and nodal.shape == (len(quad.points), 6)   # a vector drops m
    assert e_gauss < TOL and e_nodal < TOL
    assert eta2 <= 1e-22 * 2.0 * W


def test_cubic_field_eta_falls_like_h_squared(cases):
    lmd, mu = cases["lame"]

    def make(points, cells10, u):
        with _rec(points, cells10, lmd, mu) as rec:
            est = rec.estimate(_dev(u))
            sigma = rec.element(_dev(u), von_mises=False, energy=False)["sigma"]
            return sigma.cpu().numpy(), float(est["eta2_total"])

    psd.check_cubic_series(*psd.cubic_series(make, lmd, mu))


def test_reductions_over_more_than_256_partials(cases):
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic

    lmd, mu = cases["lame"]
    quad = to_quadratic(structured_beam(8))
    ne = len(quad.tets10)
    assert ne == 76800 and (ne + 255) // 256 > 256
    X = np.random.default_rng(77).uniform(-0.5, 0.5, size=(2, 3 * len(quad.points))) * 1e-3
    ns = psd.NumpyQuadraticStress(quad.points, quad.tets10, lmd, mu)
    want = ns.element(X)
    want_zz = ns.error(want["sigma"], nodal=ns.nodal(want["sigma"]))
    with _rec(quad.points, quad.tets10, lmd, mu) as rec:
        el = rec.element(_dev(X), von_mises=False, energy=False)
        zz = rec.error(el["sigma"], nodal=rec.nodal(el["sigma"]))
    errs = {k: _err(el[k], want[k]) for k in ("energy_total", "von_mises_max")}
    errs.update({k: _err(zz[k], want_zz[k]) for k in ("eta2_total", "eta2_max")})
    print(errs)
    assert max(errs.values()) < TOL, errs
    assert np.array_equal(el["von_mises_argmax"].cpu().numpy(), want["von_mises_argmax"])
    assert np.array_equal(zz["eta2_argmax"].cpu().numpy(), want_zz["eta2_argmax"])


def test_repeatable_bits_column_independence_grouping_and_no_mask(cases):
    import torch

    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    pts, c10, lmd, mu, _, X, _ = cases["curved288"]
    rng = np.random.default_rng(9)
    X33 = _dev(rng.uniform(-0.5, 0.5, size=(33, X.shape[1])) * 1e-3)

    def run(rec, Xb):
        el = rec.element(Xb)
        nodal = rec.nodal(el["sigma"])
        return {**el, "nodal": nodal, **rec.error(el["sigma"], nodal=nodal)}

    with _rec(pts, c10, lmd, mu) as rec:
        a, b = run(rec, X33[:16]), run(rec, X33[:16])
        for k in a:
            assert torch.equal(a[k], b[k]), k
        for j in (0, 7, 15):
            one = run(rec, X33[j])
            for k in a:
                assert torch.equal(one[k], a[k][j]), (j, k)
        for mc in (17, 33):
            whole = run(rec, X33[:mc])
            for lo in range(0, mc, 16):
                part = run(rec, X33[lo:min(lo + 16, mc)])
                for k in whole:
                    assert torch.equal(whole[k][lo:lo + 16], part[k]), (mc, lo, k)
        hist = rec.history(X33[:17].T.contiguous())
        whole = rec.element(X33[:17])
        for k in hist:
            assert torch.equal(hist[k], whole[k]), k
    # the Dirichlet mask of the handle is not applied: a NaN on a clamped dof reaches the stress
    dd = np.arange(0, 9)
    with ModalOperator(pts, c10, dd, lmd, mu, 1.0) as op, _rec(None, None, None, None, operator=op) as rec:
        Xn = X33[:2].clone()
        Xn[1, dd] = float("nan")
        el = rec.element(Xn)
        assert torch.isfinite(el["energy_total"][0]) and torch.isnan(el["energy_total"][1])
        assert torch.isnan(el["sigma"][1]).any() and not torch.isnan(el["sigma"][0]).any()


def test_padded_and_odd_leading_dimensions(cases):
    import torch

    pts, c10, lmd, mu, _, X, _ = cases["curved288"]
    ne, nn, ndof = len(c10), len(pts), 3 * len(pts)
    with _rec(pts, c10, lmd, mu) as rec:
        for mc in (1, 5, 16):
            for pad, shift in ((7, 0), (8, 0), (8, 1)):               # odd, even, even off 16 bytes
                ldx, lds, ldv, lde, ldn = ndof + pad, 24 * ne + pad, 4 * ne + pad, ne + pad, 6 * nn + pad
                Xb = torch.full((mc * ldx + shift,), 3.0, dtype=torch.float64, device=DEV)
                Xp = Xb[shift:].view(mc, ldx)
                Xp[:, :ndof] = _dev(X[:mc])
                full = lambda ld: torch.full((mc * ld + shift,), 7.0, dtype=torch.float64, device=DEV)  # noqa: E731
                Sb, Vb, Eb, Nb, Hb = full(lds), full(ldv), full(lde), full(ldn), full(lde)
                S, V, E, N, H = (t[shift:].view(mc, -1) for t in (Sb, Vb, Eb, Nb, Hb))
                T, M, T2, M2 = (torch.full((mc,), 7.0, dtype=torch.float64, device=DEV) for _ in range(4))
                A, A2 = (torch.full((mc,), 7, dtype=torch.int32, device=DEV) for _ in range(2))
                rec.stress_raw(mc, Xp, ldx, S, lds, V, ldv, E, lde, T, M, A)
                rec.nodal_raw(mc, S, lds, N, ldn)
                rec.error_raw(mc, S, lds, N, ldn, None, 0, H, lde, T2, M2, A2)
                torch.cuda.synchronize()
                case = (mc, pad, shift)
                for t, k in ((S, 24 * ne), (V, 4 * ne), (E, ne), (N, 6 * nn), (H, ne)):
                    assert (t[:, k:] == 7.0).all(), case
                for t in (Sb, Vb, Eb, Nb, Hb):
                    assert (t[:shift] == 7.0).all(), case
                assert (Xp[:, ndof:] == 3.0).all()
                ref = rec.element(_dev(X[:mc]))
                rn = rec.nodal(ref["sigma"])
                rz = rec.error(ref["sigma"], nodal=rn)
                assert torch.equal(S[:, :24 * ne].reshape(mc, ne, 4, 6), ref["sigma"]), case
                assert torch.equal(V[:, :4 * ne].reshape(mc, ne, 4), ref["von_mises"]) and torch.equal(E[:, :ne], ref["energy"]), case
                assert torch.equal(T, ref["energy_total"]) and torch.equal(M, ref["von_mises_max"]), case
                assert torch.equal(A, ref["von_mises_argmax"]), case
                assert torch.equal(N[:, :6 * nn].reshape(mc, nn, 6), rn) and torch.equal(H[:, :ne], rz["eta2"]), case
                assert torch.equal(T2, rz["eta2_total"]) and torch.equal(M2, rz["eta2_max"]) and torch.equal(A2, rz["eta2_argmax"]), case
                # the element form on padded rows
                H2 = full(lde)[shift:].view(mc, lde)
                rec.error_raw(mc, S, lds, None, 0, S, lds, H2, lde)
                torch.cuda.synchronize()
                assert not H2[:, :ne].any() and (H2[:, ne:] == 7.0).all(), case


def test_zero_displacement(cases):
    import torch

    pts, c10, lmd, mu, _, X, _ = cases["beam36"]
    with _rec(pts, c10, lmd, mu) as rec:
        est_in = torch.zeros((3, X.shape[1]), dtype=torch.float64, device=DEV)
        el = rec.element(est_in)
        est = rec.estimate(est_in)
    assert not el["von_mises_max"].any() and not el["von_mises_argmax"].any() and not el["energy_total"].any()
    assert not est["eta2_max"].any() and not est["eta2_argmax"].any() and not est["relative"].any()


def test_validation_writes_nothing(cases):
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery

    pts, c10, lmd, mu, _, X, _ = cases["curved288"]
    ne, nn, ndof = len(c10), len(pts), 3 * len(pts)
    Xd = _dev(X[:1]).reshape(-1)
    nine = lambda k: torch.full((k,), 9.0, dtype=torch.float64, device=DEV)  # noqa: E731
    S, V, E, N, H, T = nine(24 * ne), nine(4 * ne), nine(ne), nine(6 * nn), nine(ne), nine(1)
    A = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    outs = (S, V, E, N, H, T, A)
    with _rec(pts, c10, lmd, mu) as rec:
        st = dict(m=1, x=Xd, ldx=ndof, sigma=S, ld_sigma=24 * ne, von_mises=V, ld_vm=4 * ne, energy=E, ld_elem=ne, energy_total=T,
                  von_mises_max=T, von_mises_argmax=A)
        no = dict(m=1, sigma=S, ld_sigma=24 * ne, sigma_node=N, ld_node=6 * nn)
        er = dict(m=1, sigma=S, ld_sigma=24 * ne, sigma_node=N, ld_node=6 * nn, eta2=H, ld_eta=ne, eta2_total=T, eta2_max=T,
                  eta2_argmax=A)
        bad = [(rec.stress_raw, dict(st, m=0), "m = 0"), (rec.stress_raw, dict(st, m=17), "m = 17"),
               (rec.stress_raw, dict(st, ldx=ndof - 1), "ldx"), (rec.stress_raw, dict(st, ld_sigma=24 * ne - 1), "ld_sigma"),
               (rec.stress_raw, dict(st, ld_vm=4 * ne - 1), "ld_vm"), (rec.stress_raw, dict(st, ld_elem=ne - 1), "ld_elem"),
               (rec.stress_raw, dict(st, x=None), "x_dev"),
               (rec.nodal_raw, dict(no, m=0), "m = 0"), (rec.nodal_raw, dict(no, m=17), "m = 17"),
               (rec.nodal_raw, dict(no, ld_sigma=24 * ne - 1), "ld_sigma"), (rec.nodal_raw, dict(no, ld_node=6 * nn - 1), "ld_node"),
               (rec.error_raw, dict(er, m=0), "m = 0"), (rec.error_raw, dict(er, m=17), "m = 17"),
               (rec.error_raw, dict(er, ld_sigma=24 * ne - 1), "ld_sigma"), (rec.error_raw, dict(er, ld_node=6 * nn - 1), "ld_node"),
               (rec.error_raw, dict(er, ld_eta=ne - 1), "ld_eta"),
               (rec.error_raw, dict(er, sigma_node=None, sigma_other=S, ld_other=24 * ne - 1), "ld_other"),
               (rec.error_raw, dict(er, sigma_other=S, ld_other=24 * ne), "both"),
               (rec.error_raw, dict(er, sigma_node=None), "neither")]
        for call, kw, msg in bad:
            with pytest.raises(_lib.SaaError, match=msg) as ei:
                call(**kw)
            assert ei.value.code == _lib.SAA_E_ARG, msg
        # every output NULL: a no-op
        rec.stress_raw(1, Xd, ndof)
        rec.nodal_raw(1, S, 24 * ne, None, 0)
        rec.error_raw(1, S, 24 * ne, N, 6 * nn)
        torch.cuda.synchronize()
        for t in outs:
            assert (t == 9).all()
        with pytest.raises(ValueError, match="exactly one"):
            rec.error(S.view(ne, 4, 6))
        with pytest.raises(ValueError, match="expected nodal"):
            rec.error(S.view(ne, 4, 6), nodal=H.view(1, ne))
    # an order-1 handle is refused by name, as the linear entry points refuse an order-2 one
    lib = _lib.load()
    with ModalOperator(pts[:int(c10[:, :4].max()) + 1], c10[:, :4], (), lmd, mu, 1.0) as op1:
        assert op1.order == 1
        p = lambda t: t.data_ptr()  # noqa: E731
        calls = {"saa_operator_stress_p2": lambda: lib.saa_operator_stress_p2(op1._h, 1, p(Xd), ndof, p(S), 24 * ne, p(V), 4 * ne, p(E),
                                                                              ne, p(T), p(T), p(A)),
                 "saa_operator_nodal_stress_p2": lambda: lib.saa_operator_nodal_stress_p2(op1._h, 1, p(S), 24 * ne, p(N), 6 * nn),
                 "saa_operator_stress_error_p2": lambda: lib.saa_operator_stress_error_p2(op1._h, 1, p(S), 24 * ne, p(N), 6 * nn, None,
                                                                                          0, p(H), ne, p(T), p(T), p(A))}
        for name, call in calls.items():
            assert call() == _lib.SAA_E_ARG, name
            msg = lib.saa_last_error().decode()
            assert name in msg and "order-1" in msg, msg
        with pytest.raises(ValueError, match="order-2"):
            QuadraticStressRecovery(None, None, None, None, operator=op1)
        torch.cuda.synchronize()
    for t in outs:
        assert (t == 9).all()
    # a material without compliance (mu > 0 and 3 lambda + 2 mu > 0 fail) never gets a handle: D is not positive definite
    for bad_lmd, bad_mu in ((1.0, 0.0), (-1.0, 1.0)):
        with pytest.raises(_lib.SaaError, match="not positive definite") as ei:
            _rec(pts, c10, bad_lmd, bad_mu)
        assert ei.value.code == _lib.SAA_E_ARG
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 9).all()


def test_cli_dynamics_then_stress_and_estimate(tmp_path):
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd.fem_setup import lame
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.results_io import load_displacement

    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")

    def run(*args):
        out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args, "--synthetic", "1",
                              "--order", "2", "--out", str(tmp_path)], cwd=str(tmp_path), capture_output=True, text=True,
                             timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    run("dynamics", "--steps", "200", "--save-every", "50")
    st = run("stress", "--columns", "0,-1", "--history")
    es = run("estimate")
    traj = load_displacement(str(tmp_path / drivers.PATHS["dynamics"].format(p=2)))
    quad = to_quadratic(structured_beam(1))
    lmd, mu = lame(drivers.DEFAULTS["E"], drivers.DEFAULTS["nu"])
    n_cols = traj.shape[1]
    assert st["order"] == 2 and st["n_saved"] == n_cols and st["n_elems"] == len(quad.tets10) and st["n_nodes"] == len(quad.points)
    assert [c["column"] for c in st["columns"]] == [0, n_cols - 1] and [c["column"] for c in es["columns"]] == [n_cols - 1]
    with _rec(quad.points, quad.tets10, lmd, mu) as rec:
        X = _dev(traj[:, [0, n_cols - 1]].T)
        el = rec.element(X)
        est = rec.estimate(X[1])
        hist = rec.history(traj)
    close = lambda a, b: abs(a - b) <= 1e-11 * abs(b)  # noqa: E731
    for i, col in enumerate(st["columns"]):
        assert set(col) == {"column", "strain_energy", "von_mises_max", "element", "gauss_point", "position", "centroid"}
        assert close(col["strain_energy"], float(el["energy_total"][i])) and close(col["von_mises_max"], float(el["von_mises_max"][i]))
        assert 4 * col["element"] + col["gauss_point"] == int(el["von_mises_argmax"][i])
        assert len(col["position"]) == 3 and len(col["centroid"]) == 3
    col = es["columns"][0]
    assert set(col) == {"column", "eta", "energy_norm", "relative", "element", "eta2_max", "centroid"}
    assert close(col["eta"], float(est["eta2_total"]) ** 0.5) and close(col["energy_norm"], (2.0 * float(est["energy_total"])) ** 0.5)
    assert close(col["relative"], float(est["relative"])) and 0.0 < col["relative"] < 1.0
    assert col["element"] == int(est["eta2_argmax"]) and close(col["eta2_max"], float(est["eta2_max"]))
    with np.load(st["history"]) as h:
        assert np.allclose(h["strain_energy"], hist["energy_total"].cpu().numpy(), rtol=1e-11, atol=0.0)
        assert np.array_equal(4 * h["von_mises_element"] + h["von_mises_gauss_point"], hist["von_mises_argmax"].cpu().numpy())
    files = st["files"] + es["files"]
    assert [os.path.basename(f) for f in files] == ["Stress-order2-col-0.vtk", f"Stress-order2-col-{n_cols - 1}.vtk",
                                                    f"Estimate-order2-col-{n_cols - 1}.vtk"]
    for f in files:
        text = open(f).read()
        ne = len(quad.tets10)
        assert f"CELLS {ne} {11 * ne}" in text
        assert set(text[text.index(f"CELL_TYPES {ne}"):].split("\n")[1:ne + 1]) == {"24"}
        assert "SCALARS sigma-xx double 1" in text and "SCALARS von-mises-max double 1" in text and "SCALARS energy double 1" in text
    assert "SCALARS eta2 double 1" in open(files[-1]).read()
