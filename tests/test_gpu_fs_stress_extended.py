"""The finite-strain stress recovery of ``csrc/saa_stress_fs.hip`` (``saa_operator_stress_finite``) off the moderate-strain
beam, against the longdouble reference of tests/fs_stress_double.py on the cases of tests/fs_stress_extended.py.

Families (tests/fs_stress_extended.py builds them, tests/test_fs_stress_extended.py qualifies every one on the CPU): ``max|H|``
1e-4 and 1e-8; ``nu`` 0.499999 at 0.3 and 1e-6 and 0.4999 at 1e-6; ``min det F`` 1e-2 and 1e-3; a rigid rotation of 0.5 rad
next to a strain of 1e-6; a dilation; coordinates shifted by 2^20; needles, slivers and strongly curved elements; on the four
meshes of ``finite_strain_double.MESHES`` (<= 288 elements, three of them cross a 256-lane block edge), for both materials and
both measures.

The bar, per output (``stress``, ``von_mises``, ``det_f``, ``energy``, ``energy_total``, ``von_mises_max``,
``von_mises_argmax``): ``err = max|y - r| / max|r| <= 1e-12 + 8 env``, as tests/test_gpu_operator_extended.py.  Each test prints
``err``, ``env`` and ``err / env``.  Units: no bar, bitwise.  The pass as it was first written formed the Cauchy stress of St.
Venant-Kirchhoff as ``F S F^T / J`` in one piece and took the von Mises differences from it; its float64 restatement
(``kernel_order=True``) fails this file's bar for ``von_mises`` on the ``nu = 0.499999``, ``max|H| = 1e-6`` case of every mesh by
28 to 60 times (tests/test_fs_stress_extended.py).  So did the kernel on the MI355X: 2.2e-11, 2.8e-11, 3.0e-11 and 4.4e-11 on
``structured288``, ``delaunay2``, ``beam36`` and ``curved288`` at envelopes of 1.1e-15 to 7.2e-15, everything else within the bar.
With the differences taken before the pressure goes in it gives 1.8e-16, 2.9e-16, 1.7e-15 and 3.2e-15 there (``err / env`` 0.16,
0.04, 1.1, 0.68), and over the whole file at most 0.24 of the bar (slivers, ``energy_total``; the chain 0.37, slivers,
``eta2_total``); the largest errors as such are the rotation family's, 2.2e-8 at an envelope of 2.1e-8.

Also here: the launch edges (1, 255, 256 and 257 elements through the raw entry with sentinels behind every row), whole
workgroups without a value (a reflected part of the mesh: ``det F = -1`` at every point), and the chain element stress ->
nodal recovery -> Zienkiewicz-Zhu estimate on the PK2 field of the nearly incompressible and the sliver cases."""
import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import fs_stress_extended as sx
import operator_extended as ox

pytestmark = pytest.mark.gpu

FLOAT_OUTPUTS = tuple(k for k in sx.OUTPUTS if k not in ox.ARG_OF)
SENTINEL, N_SENTINEL = -7.25, 64


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(t):
    return t.cpu().numpy()


def _recovery(case):
    """The recovery of the case's order on a handle of its own, built with the case's Dirichlet dofs (which the stress passes
    ignore); ``close()`` closes the handle too."""
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery, StressRecovery

    op = ModalOperator(case["points"], case["cells"].astype(np.int32), np.asarray(case["dd"], dtype=np.int32), case["lmd"],
                       case["mu"], fd.RHO)
    rec = (QuadraticStressRecovery if case["cells"].shape[1] == 10 else StressRecovery)(None, None, None, None, operator=op)
    rec._own = True
    return rec


def _fields(res, j=None):
    """The outputs of ``rec.element`` under the names of ``sx.OUTPUTS``, on the host (``j``: one column of a block)."""
    pick = (lambda v: v) if j is None else (lambda v: v[j])
    out = {k: _host(pick(res[k])) for k in FLOAT_OUTPUTS if k != "stress"}
    out["stress"] = _host(pick(res["sigma"]))
    out["von_mises_argmax"] = _host(pick(res["von_mises_argmax"]))
    return out


# ---- 1. parity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material,measure", sx.COMBOS)
@pytest.mark.parametrize("cid", sx.case_ids(), ids=sx.case_name)
def test_every_output_is_within_the_bar(cid, material, measure):
    case, ref, env, info = sx.reference(cid)
    key = (material, measure)
    assert info["n_inverted"][key] == 0
    with _recovery(case) as rec:
        res = rec.element(_dev(case["u"]), material=material, measure=measure)
    assert res["n_inverted"] == 0 and res["measure"] == measure
    _, bad = sx.check(_fields(res), cid, key, ox.KERNEL_FACTOR)
    assert not bad, bad


# ---- 2. units -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("material,measure", sx.COMBOS)
@pytest.mark.parametrize("cid", fx.unit_cases(), ids=sx.case_name)
def test_power_of_two_units_commute_bitwise(cid, material, measure, u):
    case = sx.build_case(cid)
    scaled = fx.scaled_case(case, u)
    key = (material, measure)
    ref = sx.outputs(scaled, combos=[key])[0][key]                    # no overflow or underflow in the reference first
    for name in FLOAT_OUTPUTS:
        r = np.asarray(ref[name], dtype=np.float64)
        assert np.isfinite(r).all() and (np.abs(r[r != 0]) > 1e-290).all() and np.abs(r).max() < 1e290, name
    got = []
    for c in (case, scaled):
        with _recovery(c) as rec:
            res = rec.element(_dev(c["u"]), material=material, measure=measure)
            assert res["n_inverted"] == 0
            got.append(_fields(res))
    differ = [(name, int((got[1][name] != got[0][name] * 2.0 ** (u * sx.UNIT_EXPONENT[name])).sum())) for name in FLOAT_OUTPUTS
              if not np.array_equal(got[1][name], got[0][name] * 2.0 ** (u * sx.UNIT_EXPONENT[name]))]
    print(sx.case_name(cid), material, measure, u, "outputs that differ:", differ)
    assert not differ, differ
    assert int(got[1]["von_mises_argmax"]) == int(got[0]["von_mises_argmax"])


# ---- 3. launch edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material,measure", sx.COMBOS)
@pytest.mark.parametrize("n_elems", (1, 255, 256, 257))
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_launch_edges_through_the_raw_entry(name, n_elems, material, measure):
    """The first ``n_elems`` elements as a mesh of their own, two equal columns through ``stress_finite_raw`` with 64 sentinel
    doubles behind every row of every output: column 0 to the bar, column 1 bit-equal to it, every sentinel intact."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib

    case, ref, env, info = sx.edge_reference(name, n_elems)
    key = (material, measure)
    assert info["n_inverted"][key] == 0 and len(case["cells"]) == n_elems
    nq, m = (4 if case["cells"].shape[1] == 10 else 1), 2
    width = {"stress": 6 * nq * n_elems, "von_mises": nq * n_elems, "det_f": nq * n_elems, "energy": n_elems}
    with _recovery(case) as rec:
        X = _dev(np.stack([case["u"], case["u"]]))
        buf = {k: torch.full((m, w + N_SENTINEL), SENTINEL, dtype=torch.float64, device="cuda") for k, w in width.items()}
        red = {k: torch.full((m + N_SENTINEL,), SENTINEL, dtype=torch.float64, device="cuda") for k in ("energy_total", "von_mises_max")}
        arg = torch.full((m + N_SENTINEL,), -77, dtype=torch.int32, device="cuda")
        inv = rec.stress_finite_raw(_lib.material_id(material), _lib.MEASURES[measure], m, X, rec.n_dof,
                                    buf["stress"], width["stress"] + N_SENTINEL, buf["von_mises"], width["von_mises"] + N_SENTINEL,
                                    buf["det_f"], width["det_f"] + N_SENTINEL, buf["energy"], width["energy"] + N_SENTINEL,
                                    red["energy_total"], red["von_mises_max"], arg, n_inverted=True)
        torch.cuda.synchronize()
    assert inv == [0, 0]
    got = {k: _host(buf[k][:, :w]) for k, w in width.items()}
    got.update({k: _host(v[:m]) for k, v in red.items()})
    got["von_mises_argmax"] = _host(arg[:m])
    for k, w in width.items():
        assert bool((buf[k][:, w:] == SENTINEL).all()), k
    assert all(bool((v[m:] == SENTINEL).all()) for v in red.values()) and bool((arg[m:] == -77).all())
    _, bad = sx.check_fields({k: v[0] for k, v in got.items()}, ref, env, key, ox.KERNEL_FACTOR,
                             f"{name} first {n_elems} {material} {measure}")
    assert not bad, bad
    assert all(np.array_equal(v[0], v[1]) for v in got.values())


# ---- 4. whole workgroups without a value ----------------------------------------------------------------------------------

@pytest.mark.parametrize("material,measure", sx.COMBOS)
@pytest.mark.parametrize("name", ("structured288", "curved288"))
def test_whole_workgroups_without_a_value(name, material, measure):
    """``sx.with_copy``: the mesh, cut behind element 255 so that its two parts share no node, followed by a copy of its first
    32 elements on nodes of their own (elements 288 to 319; 320 elements, two workgroups).  Three columns in one call: healthy
    everywhere; the copy reflected through its centroid (``u = -2 (X - c)``: ``det F = -1`` at every point, no rounding decides
    a sign) - the second workgroup then ends in 32 lanes without a value; the first 256 elements reflected - the whole first
    workgroup has none, and the maximum and its index come from the second.  ``svk`` with ``pk2`` does not look at ``J`` (and
    a reflection has ``E = 0``)."""
    import torch

    case, columns, ref, env, count = sx.copy_reference(name)
    key = (material, measure)
    ne, nq = len(case["cells"]), 4 if case["cells"].shape[1] == 10 else 1
    assert ne == 320
    looks = key != ("svk", "pk2")
    gone = [np.zeros(ne, dtype=bool), np.arange(ne) >= 288, np.arange(ne) < 256]
    with _recovery(case) as rec:
        res = rec.element(_dev(columns), material=material, measure=measure)
        alone = [rec.element(_dev(col), material=material, measure=measure) for col in columns]
    assert res["n_inverted"].tolist() == ([0, 32, 256] if looks else [0, 0, 0])
    for j in range(3):
        assert count[j][key] == (int(gone[j].sum()) if looks else 0)
        got = _fields(res, j)
        _, bad = sx.check_fields(got, ref[j], env[j], key, ox.KERNEL_FACTOR, f"{name} + copy column {j} {material} {measure}")
        assert not bad, (j, bad)                                      # (det_f among them: the computed value is kept)
        one = _fields(alone[j])
        assert all(np.array_equal(one[k], got[k]) for k in sx.OUTPUTS), j
        assert alone[j]["n_inverted"] == int(res["n_inverted"][j])
        det = got["det_f"].reshape(ne, nq)
        if j:
            assert np.abs(det[gone[j]] + 1.0).max() <= 1e-12 and (det[~gone[j]] > 0).all()
        if looks:
            rows = np.concatenate([got["stress"].reshape(ne, -1), got["von_mises"].reshape(ne, -1), got["energy"].reshape(ne, -1)],
                                  axis=1)
            assert not rows[gone[j]].any() and rows[~gone[j]].any(axis=1).all()
            assert not gone[j][int(got["von_mises_argmax"]) // nq]
    if looks:
        assert int(res["von_mises_argmax"][2]) // nq >= 256           # the maximum of column 2 lies in the second workgroup
    assert bool(torch.isfinite(res["energy_total"]).all()) and bool((res["energy_total"] > 0).all())


# ---- 5. the chain to the estimate (secondary) -----------------------------------------------------------------------------

@pytest.mark.parametrize("material", fd.MATERIALS)
@pytest.mark.parametrize("cid", sx.composite_ids(), ids=sx.case_name)
def test_nodal_recovery_and_estimate_of_the_pk2_field(cid, material):
    """``rec.nodal`` of the kernel's own PK2 field and ``rec.estimate(u, material=)`` against ``Extended.nodal`` / ``.error``
    applied to the longdouble PK2 field; the envelope is that of the whole chain from the inputs."""
    case, ref, env, info = sx.reference(cid)
    key = (material, "pk2")
    with _recovery(case) as rec:
        u = _dev(case["u"])
        sigma = rec.element(u, von_mises=False, energy=False, material=material, measure="pk2")["sigma"]
        nodal = rec.nodal(sigma)
        est = rec.estimate(u, material=material)
    assert est["n_inverted"] == 0
    got = {"nodal": _host(nodal), "eta2": _host(est["eta2"]), "eta2_total": _host(est["eta2_total"])}
    _, bad = sx.check(got, cid, key, ox.KERNEL_FACTOR, f"{sx.case_name(cid)} {material} chain", names=sx.COMPOSITE)
    assert not bad, bad
