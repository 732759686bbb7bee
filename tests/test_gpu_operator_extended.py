"""The operator-handle kernels (csrc/saa_modal.hip, saa_p2.hip, saa_stress.hip, saa_stress_p2.hip, the element bound and the
stress error estimate) off the unit beam, against the extended-precision reference of tests/operator_extended.py.

Families (tests/operator_extended.py builds them): material ``nu`` in {-0.3, 0, 0.3, 0.49, 0.4999, 0.499999}; every
coordinate shifted by (s, -s, s/3), s = 2^10 and 2^20; needles (y times 1e-3); slivers (V / h^3 = 1e-6 in every fifth
element); strongly curved order-2 elements; on ``structured_beam(2)``, ``delaunay_beam(2)`` at order 1 and the 36-element
beam and the 288-element fixture, straight and curved, at order 2 (the fixture spans two workgroups).  Five columns.

The bar, per output and column: ``err = max|y - r| / max|r| <= 1e-12 + 8 env`` with ``env`` what rounding the inputs once costs
the reference (module docstring of operator_extended; tests/test_operator_extended.py shows on the CPU that the bar is
reachable and that the forms the stress kernels had before miss it at ``nu = 0.499999``).  An argmax passes when the
reference's value at the kernel's index is the reference's maximum up to the bar.  Each test prints ``err``, ``env`` and
``err / env`` per output.

Units: no bar.  Coordinates and columns times 2^+-40, ``lambda`` and ``mu`` times 4^+-10, ``rho`` times 2^+-20: every
floating-point output is bitwise the unscaled one times its power of two, every integer output is equal.  Every operation
in these kernels is homogeneous, so any difference is a hidden absolute threshold.

``element_bound`` on the needle, sliver and ``nu`` meshes at order 1: ``omega_e`` under the bar against ``eigvalsh`` of the
longdouble-built element matrix, ``omega_max >= (1 - 1e-12) omega_true`` of the dense generalised eigenproblem with the
lumped mass, certified with no nonpositive volume."""
import numpy as np
import pytest

import operator_extended as ox

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _host(t):
    return t.cpu().numpy()


def _operator(case):
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    return ModalOperator(case["points"], case["cells"].astype(np.int32), (), case["lmd"], case["mu"], case["rho"])


def gpu_outputs(case):
    """The names of ``operator_extended.outputs`` from ``ModalOperator`` and the stress recovery of its order."""
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery, StressRecovery

    out = {}
    with _operator(case) as op:
        X = _dev(case["X"])
        kx, mx = op.apply(X, k=True, m=True)
        out["kx"], out["mx"] = _host(kx), _host(mx)
        out["load"] = _host(op.load(case["force"]))
        dk, dm = op.diagonal()
        out["diag_k"], out["diag_m"] = _host(dk), _host(dm)
        rec = (QuadraticStressRecovery if op.order == 2 else StressRecovery)(None, None, None, None, operator=op)
        out.update({k: _host(v) for k, v in rec.element(X).items()})
        sig, psig = _dev(case["sig"]), _dev(case["psig"])
        out["nodal"] = _host(rec.nodal(sig))
        for tag, res in (("zz", rec.error(sig, nodal=_dev(case["nod"]))), ("other", rec.error(sig, other=_dev(case["sig_other"]))),
                         ("press", rec.error(psig, nodal=_dev(case["pnod"])))):
            out.update({f"{tag}.{k}": _host(v) for k, v in res.items()})
        rec.close()
    return out


@pytest.mark.parametrize("cid", ox.case_ids(), ids=ox.case_name)
def test_every_output_is_within_the_bar(cid):
    case, ref, env = ox.reference(cid)
    got = gpu_outputs(case)
    assert sorted(got) == sorted(ref)
    _, bad = ox.check(got, ref, env, ox.KERNEL_FACTOR, ox.case_name(cid))
    assert not bad, bad


@pytest.mark.parametrize("u", ox.UNITS, ids=("up", "down"))
@pytest.mark.parametrize("mesh", ox.MESHES)
def test_power_of_two_units_commute_bitwise(mesh, u):
    case = ox.build_case((mesh, "nu", 0.3))
    scaled = ox.scaled_case(case, u)
    base, got = gpu_outputs(case), gpu_outputs(scaled)
    if mesh in ox.MESHES_P1:
        for c, o in ((case, base), (scaled, got)):
            with _operator(c) as op:
                b = op.element_bound(return_omega=True)
            o["omega_e"], o["omega_max"], o["element"] = _host(b["omega_e"]), np.float64(b["omega_max"]), np.int64(b["element"])
            assert b["certified"]
    differ = []
    for name, want in base.items():
        if name in ox.UNIT_EXPONENT:
            want = want * 2.0 ** (u * ox.UNIT_EXPONENT[name])            # exact: no result here is near the ends of the range
            assert np.isfinite(got[name]).all() and (np.abs(got[name][got[name] != 0]) > 1e-290).all(), name
        if not np.array_equal(got[name], want):
            differ.append((name, int((got[name] != want).sum())))
    print(mesh, u, "outputs that differ:", differ)
    assert not differ, differ


@pytest.mark.parametrize("cid", ox.bound_case_ids(), ids=ox.case_name)
def test_element_bound_off_the_unit_beam(cid):
    case, ref, env = ox.bound_reference(cid)
    with _operator(case) as op:
        b = op.element_bound(return_omega=True)
    got = _host(b["omega_e"])
    err = float(np.abs(got.astype(np.longdouble) - ref).max() / ref.max())
    true = ox.omega_true(case)
    bar = ox.TOL + ox.KERNEL_FACTOR * env
    print(f"{ox.case_name(cid):34s} omega_e err {err:.2e}  env {env:.2e}  err/env {err / max(env, 1e-300):.2e}  "
          f"omega_max / omega_true {b['omega_max'] / true:.6f}")
    assert err <= bar
    assert b["omega_max"] == got.max() and 0 <= b["element"] < len(got)
    assert ref[b["element"]] >= ref.max() * (1 - bar)
    assert b["omega_max"] >= (1 - 1e-12) * true
    assert b["certified"] and b["n_nonpositive"] == 0
