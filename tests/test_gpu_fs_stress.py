"""Finite-strain stress recovery on the GPU: ``saa_operator_stress_finite`` and everything above it (``stress.StressRecovery``
/ ``QuadraticStressRecovery`` with ``material=``, ``drivers stress`` / ``estimate`` / ``steady_state --material``), against the
longdouble NumPy double of tests/fs_stress_double.py.

Shapes: the four meshes of ``finite_strain_double.MESHES`` - 288 tets cross a block edge of the 256-lane passes, the 36-tet
beam stays within one block.  Bars: 1e-12 of the largest entry for one evaluation against the longdouble double (the
project's bar for operator outputs), bitwise wherever the same kernel runs on the same data."""
import json
import os

import numpy as np
import pytest

import finite_strain_double as fd
import fs_stress_double as sd

pytestmark = pytest.mark.gpu

LMD, MU = fd.lame(fd.E, fd.NU)
TOL = 1e-12
COMBOS = [(material, measure) for material in fd.MATERIALS for measure in sd.MEASURES]
FIELDS = ("sigma", "von_mises", "det_f", "energy", "energy_total", "von_mises_max", "von_mises_argmax")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _np(t):
    return t.cpu().numpy()


def _err(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble).reshape(want.shape) - want).max() / np.abs(want).max())


def _recovery(pts, cells, dd=()):
    """The recovery of the mesh's order on its own handle (``dd``: Dirichlet dofs of the handle, which the stress ignores)."""
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery, StressRecovery

    op = ModalOperator(pts, cells.astype(np.int32), np.asarray(dd, dtype=np.int32), LMD, MU, fd.RHO)
    rec = (QuadraticStressRecovery if cells.shape[1] == 10 else StressRecovery)(None, None, None, None, operator=op)
    rec._own = True                                                   # close() closes the handle too
    return rec


class Mesh:
    """One mesh of the tests: points, cells, the longdouble double, the ``max|H| = 0.3`` field of its seed, and the
    double's results on it, computed once per (material, measure)."""

    def __init__(self, k, name):
        self.name = name
        self.pts, self.cells, self.dd = fd.mesh(name)
        self.ld = sd.FsStress(self.pts, self.cells, LMD, MU)
        self.u, self.det, self.hmax = fd.scale_to_strain(self.ld.fs, fd.smooth_random_field(self.pts, 40 + k))
        self.nq, self.ne = self.ld.nq, self.ld.n_elems
        self._want, self._bad = {}, None

    def want(self, material, measure):
        if (material, measure) not in self._want:
            self._want[material, measure] = self.ld.recover(self.u, material, measure)
        return self._want[material, measure]

    def bad(self):
        """``(u, elements)`` of ``finite_strain_double.inversion_state`` over a tenth of the field."""
        if self._bad is None:
            f64 = fd.FiniteStrain(self.pts, self.cells, LMD, MU, (), T=np.float64)
            _, u, elements = fd.inversion_state(f64, self.pts, 0.1 * self.u)
            self._bad = (u, np.asarray(elements))
        return self._bad

    def recovery(self, dd=()):
        return _recovery(self.pts, self.cells, dd)


@pytest.fixture(scope="module")
def meshes():
    return {name: Mesh(k, name) for k, name in enumerate(fd.MESHES)}


def _compare(res, want, label):
    """Every field of one column against the double; returns the errors after printing them."""
    errs = {"stress": _err(_np(res["sigma"]), want["stress"]), "von_mises": _err(_np(res["von_mises"]), want["von_mises"]),
            "det_f": _err(_np(res["det_f"]), want["det_f"]), "energy": _err(_np(res["energy"]), want["energy"]),
            "energy_total": abs(float(res["energy_total"]) - float(want["energy_total"])) / abs(float(want["energy_total"])),
            "von_mises_max": abs(float(res["von_mises_max"]) - float(want["von_mises_max"])) / abs(float(want["von_mises_max"]))}
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    return errs


# ---- 1. one evaluation against the double ---------------------------------------------------------------------------------

@pytest.mark.parametrize("material,measure", COMBOS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_against_the_double(meshes, name, material, measure):
    """The seeded field at ``max|H| = 0.3``.  Measured on the MI355X, of the largest entry: stress 1.6e-16 .. 4.9e-15 (svk), 2.3e-16 ..
    3.0e-15 (neo_hookean); von Mises up to 3.7e-15; ``det_f`` 9.4e-17 .. 1.7e-15; energy 2.1e-16 .. 1.8e-15; ``energy_total`` and
    ``von_mises_max`` 0 .. 6.2e-16."""
    m = meshes[name]
    want = m.want(material, measure)
    with m.recovery(m.dd) as rec:                                     # (a clamped handle: the mask is not applied)
        res = rec.element(_dev(m.u), material=material, measure=measure)
    errs = _compare(res, want, f"{name} {material} {measure}")
    assert max(errs.values()) <= TOL
    assert res["n_inverted"] == 0 and res["measure"] == measure
    top = np.sort(np.asarray(want["von_mises"], dtype=np.float64).reshape(-1))[-2:]
    if top[1] - top[0] > 1e-9 * top[1]:
        assert int(res["von_mises_argmax"]) == want["von_mises_argmax"]


# ---- 2. rigid motion --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_rigid_motion_gives_no_stress_where_the_linear_entry_reports_one(meshes, name, material):
    """The test that cannot pass without the feature: ``u = (R - I) X + c``, 0.5 rad.  Measured on the MI355X:
    ``max|stress| / max|sigma_linear|`` 4.5e-15 .. 7.2e-14 over the four meshes, both materials and both measures, with
    ``max|sigma_linear|`` 2.2e5; the energy 2e-30 .. 9e-29 of the linear one; ``|det F - 1|`` 1.1e-15 .. 1.0e-14."""
    m = meshes[name]
    u = _dev(np.asarray(fd.rigid_motion(m.pts, 0.5), dtype=np.float64))
    with m.recovery() as rec:
        lin = rec.element(u)
        scale = float(lin["sigma"].abs().max())
        assert scale > 1e5                                            # what a user of the linear entries gets today
        for measure in sd.MEASURES:
            res = rec.element(u, material=material, measure=measure)
            worst = max(float(res["sigma"].abs().max()), float(res["von_mises"].abs().max()), float(res["von_mises_max"]))
            en = float(res["energy_total"]) / float(lin["energy_total"])
            print(name, material, measure, f"max|stress| / max|sigma_linear| = {worst / scale:.2e} (linear {scale:.3e}),",
                  f"energy / linear energy = {en:.2e}, max|det F - 1| = {float((res['det_f'] - 1).abs().max()):.2e}")
            assert worst <= TOL * scale and abs(en) <= TOL and res["n_inverted"] == 0
            assert float((res["det_f"] - 1).abs().max()) <= TOL


# ---- 3. objectivity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_objectivity(meshes, name, material):
    """``u' = R (X + u) - X``: PK2, the energy and ``det F`` are those of ``u``; Cauchy turns into ``R sigma R^T``.  Measured on
    the MI355X: PK2 2.5e-15 .. 5.3e-14, energy 1.1e-15 .. 5.9e-14, ``det F`` 8.8e-16 .. 8.7e-15, Cauchy 2.7e-15 .. 4.2e-14 (the largest on
    ``delaunay2``: rounding ``u'`` to float64 costs ``eps |x| / h``)."""
    m = meshes[name]
    T = np.longdouble
    X = np.asarray(m.pts, dtype=T)
    rot = np.asarray(fd.rigid_motion(np.eye(3), 0.5, shift=(0, 0, 0)), dtype=T).reshape(3, 3).T + np.eye(3, dtype=T)   # R
    x = X + np.asarray(m.u, dtype=T).reshape(-1, 3)
    turned = np.zeros_like(x)
    for i in range(3):
        for k in range(3):
            turned[:, i] = turned[:, i] + rot[i, k] * x[:, k]
    u2 = np.asarray((turned - X).reshape(-1), dtype=np.float64)
    with m.recovery() as rec:
        a = {ms: rec.element(_dev(m.u), material=material, measure=ms) for ms in sd.MEASURES}
        b = {ms: rec.element(_dev(u2), material=material, measure=ms) for ms in sd.MEASURES}
    errs = {k: _err(_np(b["pk2"][k]), _np(a["pk2"][k])) for k in ("sigma", "energy", "det_f")}
    sg = sd.tensor(np.asarray(_np(a["cauchy"]["sigma"]), dtype=T))
    want = np.zeros_like(sg)
    for i in range(3):
        for k in range(3):
            for p in range(3):
                for q in range(3):
                    want[..., i, k] = want[..., i, k] + rot[i, p] * sg[..., p, q] * rot[k, q]
    errs["cauchy"] = _err(_np(b["cauchy"]["sigma"]), sd.voigt(want))
    print(name, material, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL


# ---- 4. tie to the force pass -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", fd.MESHES)
def test_energy_and_pk2_are_those_of_the_internal_force(meshes, name, material):
    """On a handle without Dirichlet dofs: ``energy`` against ``internal_force(..., energy=True)``, and ``f_int`` rebuilt on the
    host from the returned PK2 (``P = F S`` with the double's gradients and weights, longdouble).  Measured on the MI355X:
    energy 0 .. 5.1e-16 (neo_hookean at order 1 and on ``curved288``: 0), ``f_int`` 1.5e-16 .. 2.2e-15 of ``max|f|``."""
    m = meshes[name]
    with m.recovery() as rec:
        res = rec.element(_dev(m.u), material=material, measure="pk2")
        f, en, n_inv = rec.op.internal_force(_dev(m.u), material, energy=True)
    rebuilt = m.ld.force_from_pk2(m.u, _np(res["sigma"]).reshape(m.ne, m.nq, 6))
    e_en, e_f = _err(_np(res["energy"]), _np(en)), _err(rebuilt, _np(f))
    print(name, material, f"energy against the force pass {e_en:.2e}, f_int from PK2 {e_f:.2e}")
    assert n_inv == 0 and e_en <= TOL and e_f <= TOL


# ---- 5. homogeneous deformation ----------------------------------------------------------------------------------------------

F0 = np.array([[0.95, 0.12, -0.05], [-0.08, 0.9, 0.1], [0.06, -0.04, 0.93]])


def _closed_form(material, measure):
    """The stress of ``F0`` in longdouble from the textbook formulas, through ``C = F^T F`` and its inverse."""
    T = np.longdouble
    F = np.asarray(F0, dtype=T)
    cof, J = fd.FiniteStrain._cofactors(F)
    Cm = np.zeros((3, 3), dtype=T)
    for i in range(3):
        for k in range(3):
            for l in range(3):
                Cm[i, k] = Cm[i, k] + F[l, i] * F[l, k]
    eye = np.eye(3, dtype=T)
    if material == "svk":
        Em = (Cm - eye) / 2
        S = T(LMD) * (Em[0, 0] + Em[1, 1] + Em[2, 2]) * eye + 2 * T(MU) * Em
    else:
        ccof, cdet = fd.FiniteStrain._cofactors(Cm)
        Cinv = ccof.T / cdet
        S = T(MU) * (eye - Cinv) + T(LMD) * np.log(J) * Cinv
    if measure == "pk2":
        return sd.voigt(S), J
    sg = np.zeros((3, 3), dtype=T)
    for i in range(3):
        for k in range(3):
            for a in range(3):
                for b in range(3):
                    sg[i, k] = sg[i, k] + F[i, a] * S[a, b] * F[k, b]
    return sd.voigt(sg / J), J


@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("name", ("curved288", "delaunay2"))
def test_homogeneous_deformation_is_reproduced(meshes, name, material):
    """``u = (F0 - I) X``, ``det F0 = 0.81``, not symmetric: every point's stress is the closed form, so is the recovered nodal
    stress, and the estimate vanishes.  Measured on the MI355X: points 8.3e-15 .. 2.2e-14, nodal 5.8e-15 .. 1.1e-14, ``det F``
    1.8e-15 .. 3.3e-15, ``eta2_total / (2 energy_total)`` 3.1e-30 .. 2.5e-29."""
    m = meshes[name]
    u = _dev((m.pts @ (F0 - np.eye(3)).T).reshape(-1))
    with m.recovery() as rec:
        for measure in sd.MEASURES:
            want, J = _closed_form(material, measure)
            res = rec.element(u, material=material, measure=measure)
            nodal = rec.nodal(res["sigma"])
            e_pt = _err(_np(res["sigma"]).reshape(-1, 6), np.broadcast_to(want, (m.ne * m.nq, 6)))
            e_nd = _err(_np(nodal), np.broadcast_to(want, (len(m.pts), 6)))
            e_j = float((res["det_f"] - float(J)).abs().max()) / float(J)
            print(name, material, measure, f"points {e_pt:.2e}, nodal {e_nd:.2e}, det F {e_j:.2e} (det F0 = {float(J):.4f})")
            assert e_pt <= TOL and e_nd <= TOL and e_j <= TOL and res["n_inverted"] == 0
        est = rec.estimate(u, material=material)
        print(name, material, "eta2_total / (2 energy_total) =", float(est["eta2_total"]) / (2 * float(est["energy_total"])))
        assert float(est["eta2_total"]) <= 1e-20 * 2 * float(est["energy_total"]) and est["n_inverted"] == 0


# ---- 6. columns and layout ---------------------------------------------------------------------------------------------------

def _columns(m, n):
    """``n`` distinct columns: the field scaled between a tenth and all of it."""
    return np.stack([m.u * (0.1 + 0.9 * j / max(n - 1, 1)) for j in range(n)])


def _same(a, b):
    import torch

    return all(torch.equal(a[k], b[k]) for k in FIELDS)


@pytest.mark.parametrize("material,measure", COMBOS)
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_columns_are_independent_and_repeatable(meshes, name, material, measure):
    """16 columns in one call against 16 calls of one, 17 through the chunking, and the same call twice: bit-equal."""
    import torch

    m = meshes[name]
    X = _dev(_columns(m, 17))
    with m.recovery() as rec:
        all17 = rec.element(X, material=material, measure=measure)
        again = rec.element(X, material=material, measure=measure)
        assert _same(all17, again) and torch.equal(all17["n_inverted"], again["n_inverted"])
        assert tuple(all17["sigma"].shape) == (17, m.ne, *rec._ROW, 6) and tuple(all17["det_f"].shape) == (17, m.ne, *rec._ROW)
        block = rec.element(X[:16], material=material, measure=measure)
        for j in range(17):
            one = rec.element(X[j], material=material, measure=measure)
            assert all(torch.equal(one[k], all17[k][j]) for k in FIELDS), (j, "of 17")
            if j < 16:
                assert all(torch.equal(one[k], block[k][j]) for k in FIELDS), (j, "of 16")
        assert not all17["n_inverted"].any()


@pytest.mark.parametrize("material,measure", (("neo_hookean", "pk2"), ("svk", "cauchy")))
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_leading_dimensions_offsets_and_null_outputs(meshes, name, material, measure):
    """Leading dimensions above the minimum and bases that are not 16-byte aligned give the same bits and leave the padding
    alone; any subset of outputs may be NULL; a leading dimension below its minimum is refused."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    m = meshes[name]
    mat, meas = _lib.material_id(material), _lib.MEASURES[measure]
    nc, ne, nq = 3, m.ne, m.nq
    X = _dev(_columns(m, nc))
    mins = {"stress": 6 * nq * ne, "von_mises": nq * ne, "det_f": nq * ne, "energy": ne}
    with m.recovery() as rec:
        ref = rec.element(X, material=material, measure=measure)
        ref = {"stress": ref["sigma"], **{k: ref[k] for k in FIELDS[1:]}}
        pad, fill = {"stress": 3, "von_mises": 1, "det_f": 5, "energy": 7}, -7.25
        buf = {k: torch.full((1 + nc * (mins[k] + pad[k]),), fill, dtype=torch.float64, device="cuda") for k in mins}
        red = {"energy_total": torch.empty(nc, dtype=torch.float64, device="cuda"),
               "von_mises_max": torch.empty(nc, dtype=torch.float64, device="cuda"),
               "von_mises_argmax": torch.empty(nc, dtype=torch.int32, device="cuda")}
        xbuf = torch.full((1 + nc * (rec.n_dof + 3),), np.nan, dtype=torch.float64, device="cuda")
        xv = xbuf[1:].view(nc, rec.n_dof + 3)
        xv[:, :rec.n_dof] = X
        assert xv.data_ptr() % 16 == 8 and all(b[1:].data_ptr() % 16 == 8 for b in buf.values())
        inv = rec.stress_finite_raw(mat, meas, nc, xv, rec.n_dof + 3, buf["stress"][1:], mins["stress"] + 3, buf["von_mises"][1:],
                                    mins["von_mises"] + 1, buf["det_f"][1:], mins["det_f"] + 5, buf["energy"][1:],
                                    mins["energy"] + 7, **red, n_inverted=True)
        assert inv == [0] * nc
        for k in mins:
            rows = buf[k][1:].view(nc, mins[k] + pad[k])
            assert torch.equal(rows[:, :mins[k]].reshape(ref[k].shape), ref[k]), k
            assert bool((rows[:, mins[k]:] == fill).all()) and float(buf[k][0]) == fill, k
        assert all(torch.equal(red[k], ref[k]) for k in red)
        # subsets of the outputs
        for keep in (("stress",), ("det_f",), ("von_mises", "energy"), ("energy_total",), ("von_mises_argmax", "stress"),
                     ("stress", "von_mises", "det_f", "energy")):
            out = {k: torch.full((nc, mins[k]), fill, dtype=torch.float64, device="cuda") for k in mins if k in keep}
            r2 = {k: torch.zeros_like(v) for k, v in red.items() if k in keep}
            rec.stress_finite_raw(mat, meas, nc, X, rec.n_dof, out.get("stress"), mins["stress"], out.get("von_mises"),
                                  mins["von_mises"], out.get("det_f"), mins["det_f"], out.get("energy"), mins["energy"], **r2)
            for k, v in {**out, **r2}.items():
                assert torch.equal(v.reshape(ref[k].shape), ref[k]), (keep, k)
        rec.stress_finite_raw(mat, meas, nc, X, rec.n_dof)                # every output NULL: nothing to do, no error
        # refusals that need the handle
        for k, args in (("ldx", dict(ldx=rec.n_dof - 1)), ("ld_stress", dict(stress=buf["stress"], ld_stress=mins["stress"] - 1)),
                        ("ld_vm", dict(von_mises=buf["von_mises"], ld_vm=mins["von_mises"] - 1)),
                        ("ld_det", dict(det_f=buf["det_f"], ld_det=mins["det_f"] - 1)),
                        ("ld_elem", dict(energy=buf["energy"], ld_elem=ne - 1))):
            with pytest.raises(_lib.SaaError) as exc:
                rec.stress_finite_raw(mat, meas, nc, X, **{"ldx": rec.n_dof, **args})
            assert exc.value.code == _lib.SAA_E_ARG and f"saa_operator_stress_finite: {k} = " in str(exc.value)


# ---- 7. inversion ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_inversion(meshes, name):
    """``inversion_state`` as one column among healthy ones, and a column of NaN.  Measured on the MI355X: the inverted column against
    the double 0 .. 5.0e-15 in every field; everything else is exact."""
    import torch

    m = meshes[name]
    bad, elements = m.bad()
    healthy = _columns(m, 2)
    X = _dev(np.stack([healthy[0], bad, healthy[1], np.full_like(bad, np.nan)]))
    with m.recovery() as rec:
        for material, measure in COMBOS:
            res = rec.element(X, material=material, measure=measure)
            two = rec.element(_dev(healthy), material=material, measure=measure)
            for j, i in ((0, 0), (1, 2)):
                assert all(torch.equal(two[k][j], res[k][i]) for k in FIELDS), (material, measure, i)
            want = m.ld.recover(bad, material, measure)
            got = {k: v[1] for k, v in res.items() if k not in ("n_inverted", "measure")}
            errs = _compare(got, want, f"{name} {material} {measure} inverted column")
            assert max(errs.values()) <= TOL
            counts = res["n_inverted"].tolist()
            if (material, measure) == ("svk", "pk2"):
                assert counts == [0, 0, 0, 0] and want["n_inverted"] == 0
                continue
            gone = np.nonzero(want["inverted"])[0]
            assert sorted(gone) == sorted(elements) and counts == [0, len(elements), 0, m.ne]
            sig, vm, en, det = (_np(res[k][1]).reshape(m.ne, -1) for k in ("sigma", "von_mises", "energy", "det_f"))
            zero = np.nonzero(~sig.any(axis=1) & ~vm.any(axis=1) & ~en.any(axis=1))[0]
            assert sorted(zero) == sorted(elements) and (det[elements].min(axis=1) <= 0).all() and (det[np.setdiff1d(np.arange(m.ne), elements)] > 0).all()
            assert int(res["von_mises_argmax"][1]) // m.nq not in elements
            # the column of NaN: every element inverted, nothing in the total or the maximum, det F kept
            assert not _np(res["sigma"][3]).any() and not _np(res["von_mises"][3]).any() and not _np(res["energy"][3]).any()
            assert float(res["energy_total"][3]) == 0.0 and float(res["von_mises_max"][3]) == 0.0 and int(res["von_mises_argmax"][3]) == -1
            assert bool(torch.isnan(res["det_f"][3]).all())


# ---- 8. the drivers end to end ------------------------------------------------------------------------------------------------

def _parse_arrays(path):
    text = open(path).read()
    point = text[text.index("POINT_DATA"):text.index("CELL_DATA")] if "CELL_DATA" in text else text[text.index("POINT_DATA"):]
    cell = text[text.index("CELL_DATA"):] if "CELL_DATA" in text else ""
    names = lambda part: [ln.split()[1] for ln in part.splitlines() if ln.startswith("SCALARS")]  # noqa: E731
    return names(point), names(cell)


POINT_ARRAYS = ["displacement-x", "displacement-y", "displacement-z", "sigma-xx", "sigma-yy", "sigma-zz", "sigma-yz", "sigma-xz",
                "sigma-xy", "von-mises"]


@pytest.mark.parametrize("order", (2, 1))
def test_drivers_end_to_end(tmp_path, order, capsys):
    """50 steps of ``dynamics --material svk --fz 50`` on ``--synthetic 2``, then ``stress`` and ``estimate --material svk`` on
    the last column: the report against the double on the saved column.  Measured on the MI355X: ``strain_energy`` 1.8e-16,
    ``von_mises_max`` 1.6e-16 .. 2.1e-16 (after 50 steps the load has hardly acted: ``max|u|`` 6e-7 and 1e-5)."""
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd import results_io as rio
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    out = str(tmp_path)
    base = ["--synthetic", "2", "--order", str(order), "--material", "svk", "--out", out]
    drivers.main(["dynamics", *base, "--fz", "50", "--steps", "50", "--save-every", "10"])
    capsys.readouterr()
    drivers.main(["stress", *base, "--history"])
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    drivers.main(["estimate", *base])
    est = json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    mesh = structured_beam(2)
    if order == 2:
        mesh = drivers._quadratic(mesh)
    cells = np.asarray(mesh.tets10 if order == 2 else mesh.tets, dtype=np.int64)
    traj = np.asarray(rio.load_displacement(os.path.join(out, drivers.PATHS["dynamics"].format(p=order))))
    ld = sd.FsStress(mesh.points, cells, LMD, MU)
    want = ld.recover(traj[:, -1], "svk", "cauchy")
    col = rep["columns"][0]
    e_w = abs(col["strain_energy"] - float(want["energy_total"])) / float(want["energy_total"])
    e_v = abs(col["von_mises_max"] - float(want["von_mises_max"])) / float(want["von_mises_max"])
    print(f"order {order}: strain_energy {col['strain_energy']:.6e} ({e_w:.2e}), von_mises_max {col['von_mises_max']:.6e} ({e_v:.2e}),",
          f"min det F {col['min_det_f']:.4f}, max|u| {np.abs(traj[:, -1]).max():.3e}; estimate relative {est['columns'][0]['relative']:.3f}")
    assert rep["material"] == "svk" and rep["measure"] == "cauchy" and rep["order"] == order
    assert e_w <= TOL and e_v <= TOL and col["n_inverted"] == 0
    assert abs(col["min_det_f"] - float(want["det_f"].min())) <= TOL
    # (the reported element holds the double's maximum to the bar: 50 steps into the run the largest values of the structured
    # beam lie in elements that the load treats alike, and the last bit decides between them)
    vm = np.asarray(want["von_mises"], dtype=np.float64)
    print(f"order {order}: element {col['element']} holds {vm[col['element']].max():.17e}, the double's element",
          f"{want['von_mises_argmax'] // ld.nq} holds {vm.max():.17e}")
    assert vm[col["element"]].max() >= vm.max() * (1.0 - TOL)
    pk2 = ld.recover(traj[:, -1], "svk", "pk2")
    ecol = est["columns"][0]
    assert est["measure"] == "pk2" and abs(ecol["energy_norm"] ** 2 / 2 - float(pk2["energy_total"])) <= TOL * float(pk2["energy_total"])
    assert 0 < ecol["relative"] < 1 and ecol["n_inverted"] == 0
    j = traj.shape[1] - 1
    assert [os.path.relpath(f, out) for f in rep["files"]] == [f"Results/Stress/Stress-svk-order{order}-col-{j}.vtk"]
    assert [os.path.relpath(f, out) for f in est["files"]] == [f"Results/Stress/Estimate-svk-order{order}-col-{j}.vtk"]
    assert os.path.relpath(rep["history"], out) == f"Results/Stress/history-svk-order{order}.npz"
    assert _parse_arrays(rep["files"][0]) == (POINT_ARRAYS, ["von-mises-max", "energy", "det-f-min"])
    assert _parse_arrays(est["files"][0]) == (POINT_ARRAYS, ["von-mises-max", "energy", "det-f-min", "eta2"])
    with np.load(rep["history"]) as h:
        assert len(h["strain_energy"]) == traj.shape[1] and h["strain_energy"][-1] == col["strain_energy"]
        assert h["von_mises_max"][-1] == col["von_mises_max"] and h["min_det_f"][-1] == col["min_det_f"] and not h["n_inverted"].any()


def test_driver_steady_state_reports_the_stress_of_the_converged_state(tmp_path):
    """``steady_state --material svk``: the new report keys, ``strain_energy`` against the stored energy ``Pi(d)`` of the double
    at the returned ``d``, and the Cauchy stress in the file after the untouched displacement.  Measured on the MI355X:
    ``strain_energy`` against ``Pi(d)`` 0, ``von_mises_max`` 2.6e-16, ``min det F`` 0.988."""
    from synchronization_avoiding_algorithms_amd import drivers
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam

    mesh = structured_beam(2)
    path, d, rep = drivers.steady_state_nonlinear(mesh, str(tmp_path), material="svk", order=1, fz=10.0)
    cells = np.asarray(mesh.tets, dtype=np.int64)
    ld = sd.FsStress(mesh.points, cells, LMD, MU)
    want = ld.recover(d.reshape(-1), "svk", "cauchy")
    pi = ld.fs.total_energy(d.reshape(-1), "svk")
    e_w = abs(rep["strain_energy"] - float(pi)) / float(pi)
    e_v = abs(rep["von_mises_max"] - float(want["von_mises_max"])) / float(want["von_mises_max"])
    print(f"strain_energy {rep['strain_energy']:.6e} against Pi(d) {e_w:.2e}, von_mises_max {rep['von_mises_max']:.6e} ({e_v:.2e}),",
          f"min det F {rep['min_det_f']:.4f}")
    assert {"von_mises_max", "element", "strain_energy", "min_det_f"} <= set(rep)
    assert e_w <= TOL and e_v <= TOL and rep["element"] == want["von_mises_argmax"]
    assert abs(rep["min_det_f"] - float(want["det_f"].min())) <= TOL
    point, cell = _parse_arrays(path)
    assert point == POINT_ARRAYS and cell == []
    text = open(path).read()
    first = text[text.index("SCALARS displacement-x"):text.index("SCALARS displacement-y")].splitlines()[2:]
    assert np.array_equal(np.array([float(v) for v in first]), d.reshape(-1, 3)[:, 0])
