"""The cases of tests/fs_stress_extended.py qualified on the CPU, before any of them is given to a kernel:

* the unmasked state of every case is the nominal one: nothing inverted, ``min det F > 0``, and ``max|H|`` of the strain part
  (``min det F`` in the ``mindet`` family) within 1 % of the case's value;
* the two conditions under which the bar ``err <= 1e-12 + 8 env`` of tests/test_gpu_fs_stress_extended.py means something, on
  every case, output and ``(material, measure)``: the stable float64 restatement of ``fs_stress_double.FsStress`` stays within
  ``1e-12 + 2 env``, and ``env <= 1e-6``; on the composite cases also for the nodal recovery and ``eta^2`` of the PK2 field,
  through the whole float64 chain;
* the longdouble run against the same statements in mpmath at 50 digits, on four elements of every family, both orders, to
  2^-58 of the field's maximum.  The rotation family is held as tests/finite_strain_extended.py explains: with ``max|H| =
  0.3`` next to the rotation at 2^-58, and at its own strain of 1e-6 to ``2^-58 + 2^-11 * 8 env``; so is the von Mises value of
  the dilation family, whose deviator is 1/20 of ``H`` and less (see the test);
* that the bar has teeth: ``kernel_order=True`` in float64 (``svk`` with ``cauchy`` as ``F S F^T / J`` in one piece, von Mises
  from the differences of the finished normal stresses - what the kernel did at first) FAILS it for the von Mises field on the
  ``nu = 0.499999``, ``max|H| = 1e-6`` case of every mesh, by 28 to 60 times the bar, and passes everything else there;
* power-of-two units commute bit for bit with the float64 restatement."""
import numpy as np
import pytest

import finite_strain_double as fd
import finite_strain_extended as fx
import fs_stress_extended as sx
import operator_extended as ox

FLOAT_OUTPUTS = tuple(k for k in sx.OUTPUTS if k not in ox.ARG_OF)

MP_CASES = [("structured288", "strain", 0, 1e-8), ("curved288", "strain", 0, 1e-4), ("delaunay2", "nu", 0.499999, 1e-6),
            ("curved288", "nu", 0.499999, 0.3), ("beam36", "nu", 0.4999, 1e-6), ("structured288", "mindet", 1e-3, 0),
            ("beam36", "mindet", 1e-2, 0), ("structured288", "rotation", 0.5, 0.3), ("curved288", "rotation", 0.5, 0.3),
            ("structured288", "shift", 20, 1e-6), ("curved288", "shift", 20, 0.3), ("delaunay2", "needle", 1e-3, 1e-6),
            ("beam36", "needle", 1e-3, 1e-6), ("structured288", "sliver", 1e-6, 0.3), ("curved288", "sliver", 1e-6, 0.3),
            ("beam36", "curved", 0.2, 1e-6)]


def _flat(res):
    """``outputs`` of one key without the leading axis and without the count."""
    return {k: v[0] for k, v in res.items() if k != "n_inverted"}


@pytest.mark.parametrize("cid", sx.case_ids(), ids=sx.case_name)
def test_the_bar_is_meaningful_on_this_case(cid):
    case, ref, env, info = sx.reference(cid)
    assert not any(info["n_inverted"].values()) and info["min_det"] > 0, info
    if cid[1] == "mindet":
        assert cid[2] <= info["min_det"] <= 1.0100001 * cid[2], info
    else:
        assert abs(sx.nominal(case) / cid[3] - 1.0) < 1e-2, (sx.nominal(case), info)
    if cid[1] not in ("rotation", "dilation"):
        assert not case["u"][case["dd"]].any()
    names = {key: sx.OUTPUTS + (sx.COMPOSITE if "nodal" in ref[key] else ()) for key in sx.COMBOS}
    assert ("nodal" in ref["svk", "pk2"]) == (cid in sx.composite_ids())
    got = sx.outputs(case, np.float64, composite=cid in sx.composite_ids())[0]
    for key in sx.COMBOS:
        assert got[key]["n_inverted"] == 0
        _, bad = sx.check(_flat(got[key]), cid, key, ox.STABLE_FACTOR, names=names[key])
        assert not bad, (key, bad)                                    # the stable restatement: 1e-12 + 2 env
        top = {k: float(v.max()) for k, v in env[key].items()}
        assert max(top.values()) <= ox.ENV_MAX, (key, top)


def test_the_case_list_is_the_trimmed_one():
    ids = sx.case_ids()
    assert len(ids) == 54 and len(set(ids)) == 54 and set(ids) <= set(fx.case_ids())
    assert len(sx.composite_ids()) == 12 and set(sx.suspect_ids()) <= set(ids)


@pytest.mark.parametrize("cid", MP_CASES, ids=sx.case_name)
def test_longdouble_matches_mpmath_at_50_digits(cid):
    import mpmath

    case = fx.sub_case(sx.build_case(cid), 4)
    worst = {}
    with mpmath.workdps(50):
        want = sx.outputs(case, ox.MP)[0]
        got = sx.outputs(case, np.longdouble)[0]
        for key in sx.COMBOS:
            assert want[key]["n_inverted"] == got[key]["n_inverted"] == 0
            assert want[key]["von_mises_argmax"] == got[key]["von_mises_argmax"]
            for name in FLOAT_OUTPUTS:
                w = want[key][name]
                diff = np.abs(ox.conv(got[key][name], ox.MP) - w)
                worst[key + (name,)] = float(diff.max() / np.abs(w).max())
    print(sx.case_name(cid), f"largest {max(worst.values()):.1e} at {max(worst, key=worst.get)}")
    assert max(worst.values()) <= 2.0 ** -58, {k: v for k, v in worst.items() if v > 2.0 ** -58}


AMPLIFIED = [("delaunay2", "rotation", 0.5, 1e-6), ("curved288", "rotation", 0.5, 1e-6),
             ("delaunay2", "dilation", fx.DILATION, 1e-3), ("beam36", "dilation", fx.DILATION, 1e-3)]


@pytest.mark.parametrize("cid", AMPLIFIED, ids=sx.case_name)
def test_longdouble_in_the_rotation_and_dilation_families_is_as_far_from_mpmath_as_its_precision_allows(cid):
    """As the test of this name in tests/test_finite_strain_extended.py: at a strain ``s`` next to a rotation every rounding is
    amplified by ``|H| / s`` in any form, so longdouble is held to ``2^-58 + 2^-11 * 8 env`` there, which leaves the reference
    2^-11 of the bar from the truth.  The dilation family is held the same way here, for the von Mises value alone: the
    deviator is what a field of 1e-3 leaves next to ``H = 0.02 I``, whose rounding (``eps |u| |grad N|``, u up to 0.1) it sees
    amplified in any form; measured 2.0e-17 of the largest von Mises value on ``delaunay2`` (env 3e-14), every other output
    of the family within 2^-58."""
    import mpmath

    case = fx.sub_case(sx.build_case(cid), 4)
    rng = np.random.default_rng(77)
    draws = [fx.perturbed(case, rng) for _ in range(ox.N_DRAWS)]
    with mpmath.workdps(50):
        got = sx.outputs(case)[0]
        want = sx.outputs(case, ox.MP)[0]
        alts = [sx.outputs(alt)[0] for alt in draws]
        for key in sx.COMBOS:
            for name in FLOAT_OUTPUTS:
                g = got[key][name]
                env = max(float(np.abs(a[key][name] - g).max() / np.abs(g).max()) for a in alts)
                err = float(np.abs(ox.conv(g, ox.MP) - want[key][name]).max() / np.abs(want[key][name]).max())
                print(sx.case_name(cid), *key, name, f"err {err:.2e} env {env:.2e}")
                held = cid[1] == "rotation" or name in ("von_mises", "von_mises_max")
                assert err <= 2.0 ** -58 + (2.0 ** -11 * ox.KERNEL_FACTOR * env if held else 0.0), (key, name, err, env)


@pytest.mark.parametrize("cid", sx.suspect_ids(), ids=sx.case_name)
def test_the_bar_has_teeth(cid):
    """``kernel_order=True`` in float64: ``svk`` with ``cauchy`` fails in ``von_mises`` - not narrowly: ``lambda / mu = 5e5``
    times the rounding is 5.5e-11, and the bar is 1e-12; measured 2.8e-11 .. 6.0e-11 - and in nothing but that field and its
    maximum; the three combinations whose differences come from the strain in either order pass everything."""
    got = sx.outputs(sx.build_case(cid), np.float64, kernel_order=True)[0]
    for key in sx.COMBOS:
        worst, bad = sx.check(_flat(got[key]), cid, key, ox.KERNEL_FACTOR, f"{sx.case_name(cid)} {key[0]} {key[1]} kernel order")
        bad = sorted(b[0] for b in bad)
        if key != ("svk", "cauchy"):
            assert bad == [], (key, bad)
            continue
        assert "von_mises" in bad and set(bad) <= {"von_mises", "von_mises_max"}, bad
        err, env = worst["von_mises"]
        assert err > 20 * (ox.TOL + ox.KERNEL_FACTOR * env), (err, env)
    stable = sx.outputs(sx.build_case(cid), np.float64, combos=[("svk", "cauchy")])[0]
    _, bad = sx.check(_flat(stable["svk", "cauchy"]), cid, ("svk", "cauchy"), ox.STABLE_FACTOR, verbose=False)
    assert not bad, bad


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("cid", fx.unit_cases(), ids=sx.case_name)
def test_power_of_two_units_commute_bitwise_in_float64(cid, u):
    case = sx.build_case(cid)
    scaled = fx.scaled_case(case, u)
    ref = sx.outputs(scaled)[0]                                       # no overflow or underflow in the reference first
    base, got = sx.outputs(case, np.float64)[0], sx.outputs(scaled, np.float64)[0]
    for key in sx.COMBOS:
        for name in FLOAT_OUTPUTS:
            r = np.asarray(ref[key][name], dtype=np.float64)
            assert np.isfinite(r).all() and (np.abs(r[r != 0]) > 1e-290).all() and np.abs(r).max() < 1e290, (key, name)
            assert np.array_equal(got[key][name], base[key][name] * 2.0 ** (u * sx.UNIT_EXPONENT[name])), (key, name)
        assert got[key]["von_mises_argmax"] == base[key]["von_mises_argmax"] and got[key]["n_inverted"] == 0
