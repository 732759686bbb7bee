"""The extended-precision reference of the production step kernels (tests/step_extended.py) checked on the CPU:

* every case and variant qualifies.  These are conditions, not measurements: ``env <= 1e-6`` on every step, the float64
  restatement (production association) within ``1e-12 + 2 env`` on every one of the 8 steps, and ``max|d| <= 16 max(|d0|,
  |dn|)`` over the 8 steps.  No state was changed for a case to qualify.  Measured: largest ``env`` 8.6e-10 (slivers, shift
  2^20), worst restatement 0.010 of its bar, largest growth 12.4 (``delaunay2``, ``nu = 0.499999``: 8 ballistic steps of the
  random state, whose ``d0 - dn`` is as large as ``d0``);
* the first step of the reference is ``sx.outputs(case)["d1"]`` bit for bit;
* the longdouble run against mpmath at 50 digits on 4-element sub-cases, every step to 1e-17;
* the plans: several blocks, a halo on every block, paired and single items, ``plan_host_check == 0``, the compact forms;
* the restatement commutes bitwise with the power-of-two units of ``sx.scaled_case`` in both directions, on the runs of
  ``step_extended.UNIT_RUNS`` (the unit of time changes and the ramp's 1 does not);
* the bar has teeth: each of the four mutants misses ``1e-12 + 8 env`` on every case it applies to but those that
  ``step_extended.BLIND`` names, and on none of those;
* on a partition a rank's ``d1`` is the whole-mesh step to 1e-17, a clamped shared dof is 0 after a synchronised step and the
  table row after a predicted one, and the mod-3 partitions do have clamped shared dofs;
* the set-up fields qualify the same way, and their reference rounded to float64 is the case's own mass and load."""
import numpy as np
import pytest

import operator_extended as ox
import step_extended as stx
import stepper_extended as sx


@pytest.mark.parametrize("key", stx.case_keys(), ids=stx.key_name)
def test_case_qualifies(key):
    case, ref, env = stx.reference(*key)
    name = stx.key_name(key)
    assert ref.shape == (stx.N_STEPS, 2, 3 * len(case["points"])) and len(case["clamped"]) > 0
    assert not case["d0"][:, case["dirichlet"]].any() and not case["dn"][:, case["dirichlet"]].any()
    assert stx.compact_forms(case) == (True, True)
    got, tns = stx.restatement(case)
    _, _, ratio, bad = stx.hold(got, ref, env, ox.STABLE_FACTOR, name + " restatement")
    g = stx.growth(case, ref)
    print(f"{name}: largest env {env.max():.2e}, restatement at {ratio:.4f} of its bar, growth {g:.2f}")
    assert env.max() <= ox.ENV_MAX
    assert not bad, bad
    assert 0 < g <= stx.GROWTH_MAX
    tn = case["tn"]
    for t in tns:                                                      # the restatement's clock is the repeated sum
        tn = tn + case["dt"]
        assert t == tn
    if key[1] == "cross1":                                             # the ramp reaches 1 inside the launch, half a step off
        assert tns[2] < 1.0 < tns[3] and abs((tns[3] - 1.0) / case["dt"] - 0.5) < 1e-6
    first = sx.outputs(case)["d1"]
    assert np.array_equal(ref[0], first)


MP_KEYS = [(("structured2", "nu", 0.499999), "base"), (("delaunay2", "shift", 20), "base"), (("delaunay2", "needle", 1e-3), "base"),
           (("structured2", "sliver", 1e-6), "base")] + [(("delaunay2", "nu", 0.3), v) for v in stx.VARIANTS[1:]]


@pytest.mark.parametrize("key", MP_KEYS, ids=stx.key_name)
def test_longdouble_matches_mpmath_at_50_digits(key):
    import mpmath

    case = stx.sub_case(*key)
    with mpmath.workdps(50):
        want, _ = stx.trajectory(case, ox.MP)
        got, _ = stx.trajectory(case)
        top = np.abs(want).max(axis=2)
        worst = np.abs(ox.conv(got, ox.MP) - want).max(axis=2) / top
        worst = float(worst.max())
    print(stx.key_name(key), f"longdouble against 50 digits over {stx.N_STEPS} steps: {worst:.1e}")
    assert worst <= 1e-17


@pytest.mark.parametrize("cid", stx.case_ids(), ids=ox.case_name)
def test_plans_are_multi_block_with_halo_pairs_and_singles(cid):
    case = stx.build_case(cid)
    blocks = {"A": (5, 8), "B": (20, 30)}
    for plan in stx.PLANS:
        f = stx.plan_facts(case, plan)
        print(ox.case_name(cid), plan, {k: f[k] for k in ("n_blocks", "n_halo_total", "min_halo", "n_items", "n_pairs", "check")})
        assert stx.plan_is_rich(f), f
        assert blocks[plan][0] <= f["n_blocks"] <= blocks[plan][1]
    if cid == ("structured2", "sliver", 1e-6):
        a, b = stx.plan_facts(case, "A"), stx.plan_facts(case, "B")
        assert (a["n_blocks"], b["n_blocks"], a["n_halo_total"], b["n_halo_total"]) == (8, 30, 225, 842)


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("mesh", ox.MESHES_P1)
def test_power_of_two_units_commute_in_the_restatement(mesh, u):
    for variant, n in stx.UNIT_RUNS:
        case = stx.build_case((mesh, "nu", 0.3), variant)
        base, _ = stx.restatement(case, n)
        got, _ = stx.restatement(sx.scaled_case(case, u), n)
        assert np.isfinite(got).all() and np.array_equal(got, base * 2.0 ** (40 * u))
        r = np.abs(base[base != 0]) * 2.0 ** (40 * u)
        assert (r > 1e-290).all() and (r < 1e290).all()


def _misses(key, mutant):
    case, ref, env = stx.reference(*key)
    got, _ = stx.restatement(case, mutant=mutant)
    _, _, ratio, bad = stx.hold(got, ref, env, ox.KERNEL_FACTOR, f"{stx.key_name(key)} {mutant}")
    return sorted({b[0] for b in bad})


def _applies(key, mutant):
    if mutant == "ramp_late":
        return key[1] not in ("noramp", "tn1.5")
    if mutant == "ramp_unclamped":
        return key[1] in ("cross1", "tn1.5")                            # (tn1.5: the unclamped ramp is 1.5 from the first step)
    return True


@pytest.mark.parametrize("mutant", stx.MUTANTS)
def test_mutant_misses_the_bar(mutant):
    keys = [k for k in stx.case_keys() if _applies(k, mutant)]
    assert keys and set(stx.BLIND[mutant]) <= {stx.key_name(k) for k in keys}
    for key in keys:
        steps = _misses(key, mutant)
        if stx.key_name(key) in stx.BLIND[mutant]:
            assert not steps, (key, steps)
            continue
        assert steps, key
        if mutant == "halo_stale":                                     # nothing before the stale read, everything after it
            assert steps == list(range(stx.STALE_STEP + 1, stx.N_STEPS + 1)), (key, steps)
        if mutant == "ramp_unclamped":
            assert steps == ([5, 6, 7, 8] if key[1] == "cross1" else list(range(1, stx.N_STEPS + 1))), (key, steps)
    for key in stx.case_keys():
        if not _applies(key, mutant):                                  # ramp off or at 1: the mutant is the restatement
            case = stx.build_case(*key)
            assert np.array_equal(stx.restatement(case, mutant=mutant)[0], stx.restatement(case)[0])
    if mutant == "rcp32":
        for name in stx.BLIND[mutant]:
            key = next(k for k in keys if stx.key_name(k) == name)
            c = stx.build_case(*key)
            det = ox.Extended(c["points"], c["cells"], c["lmd"], c["mu"], c["rho"], np.float64).detk
            r32 = np.asarray(np.asarray(1.0 / det, dtype=np.float32), dtype=np.float64)
            assert np.abs(det * r32 - 1.0).max() <= 2.0 ** -50


@pytest.mark.parametrize("key", stx.partition_keys(), ids=stx.key_name)
def test_partition_reference_is_the_whole_mesh_step_on_every_rank(key):
    case, ref, env = stx.partition_reference(*key)
    whole = stx.reference(key[0])[1][0]
    assert sorted(ref) == sorted(stx.rank_names(case))
    worst = 0.0
    for i, lay in enumerate(case["layouts"]):
        mine = whole[:, lay.local_dof]
        worst = max(worst, float(np.abs(ref[f"r{i}.d1"] - mine).max() / np.abs(mine).max()))
        assert np.array_equal(ref[f"r{i}.hist"], ref[f"r{i}.d1"][:, lay.loc_dof_shared])
        assert np.array_equal(ref[f"r{i}.p.hist"], np.asarray(case["tables"][i], dtype=np.longdouble))
        clamped = case["free"][sx._global_shared_dofs(lay)] == 0         # a clamped shared dof: 0, and the table row
        assert not ref[f"r{i}.d1"][:, lay.loc_dof_shared][:, clamped].any() and not ref[f"r{i}.iface"][:, clamped].any()
        assert np.array_equal(ref[f"r{i}.p.d1"][:, lay.loc_dof_shared], ref[f"r{i}.p.hist"])
    top = max(float(v.max()) for v in env.values())
    print(stx.key_name(key), f"rank d1 against the whole-mesh step: {worst:.1e}; largest env {top:.2e}")
    assert worst <= 1e-17 and top <= ox.ENV_MAX
    if key[1] == "mod3":                                               # clamped shared dofs exist: the finish pass has to clamp
        assert any((case["free"][sx._global_shared_dofs(lay)] == 0).any() for lay in case["layouts"])


@pytest.mark.parametrize("cid", stx.case_ids(), ids=ox.case_name)
def test_setup_fields_qualify(cid):
    case, ref, env = stx.setup_reference(cid)
    got = stx.setup_outputs(case, np.float64)
    for name in ref:
        err = float(np.abs(np.asarray(got[name], dtype=np.longdouble) - ref[name]).max() / np.abs(ref[name]).max())
        print(f"{ox.case_name(cid):30s} {name:5s} err {err:.2e} env {env[name][0]:.2e}")
        assert env[name][0] <= ox.ENV_MAX and err <= ox.TOL + ox.STABLE_FACTOR * env[name][0]
    assert np.array_equal(np.asarray(ref["load"][0], dtype=np.float64) * case["free"], case["load"])
    assert np.array_equal(np.asarray(ref["mass"][0], dtype=np.float64), case["mass"])
