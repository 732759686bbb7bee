"""The refusals of the operator family of the C API (``saa_operator_*``, ``saa_operator_stepper_*``,
``saa_operator_implicit_*``) that are reached with a null handle or before the handle is looked at, pinned against
``golden/operator_refusals.json``: return code and message, byte for byte (tests/operator_refusals.py has the record).
Where a function tests an argument before its handle the null handle is given together with the bad argument, so the order
of the two checks is pinned too.  ``@hollow`` is a handle without an implementation behind it - eight zero bytes, what the
handle structs are - which separates the checks on the handle from those on what it points to.  The two creates run on a
two-element mesh in host memory; the capacity refusals take an element count that is only a number, since the check
precedes the loop that reads the cells.  Needs the built library, no device.

``python tests/test_operator_refusals.py --write`` regenerates this part of the fixture."""
import ctypes as C
import sys

import numpy as np

import operator_refusals as refusals

MAT = ("saa_operator_internal_force", "saa_operator_tangent_apply", "saa_operator_tangent_bound")


def _cases():
    out = []

    def add(name, *args):
        out.append((name, args))

    # -- the two creates: device, n_nodes, n_elems, xyz, cells, dirichlet_dofs, n_dirichlet, lambda, mu, rho, out
    for name, n, cells, huge in (("saa_operator_create", 5, "tets", 1 << 29), ("saa_operator_create_p2", 14, "cells10", 214748365)):
        good = (0, n, 2, "@xyz", "@" + cells, "@dd", 3, 1.0, 1.0, 1.0, "@out")

        def with_(**kw):
            names = ("device", "n_nodes", "n_elems", "xyz", "cells", "dd", "n_dirichlet", "lmd", "mu", "rho", "out")
            return tuple(kw.get(k, v) for k, v in zip(names, good))

        add(name, *with_(out=None))
        add(name, *with_(n_nodes=0))
        add(name, *with_(n_nodes=-3))
        add(name, *with_(n_elems=-1))
        add(name, *with_(n_dirichlet=-1))
        add(name, *with_(xyz=None))
        add(name, *with_(cells=None))
        add(name, *with_(dd=None))
        add(name, *with_(n_elems=huge))                            # (nothing reads that many cells: refused before the loop)
        add(name, *with_(n_nodes=715827883, n_elems=0, n_dirichlet=0))
        add(name, *with_(lmd="nan"))
        add(name, *with_(mu="inf"))
        add(name, *with_(rho=0.0))
        add(name, *with_(rho="nan"))
        add(name, *with_(cells="@" + cells + "_high"))
        add(name, *with_(cells="@" + cells + "_negative"))
        add(name, *with_(dd="@dd_high" if n == 5 else "@dd_high_p2"))
        add(name, *with_(dd="@dd_negative"))
        add(name, *with_(mu=-1.0))                                 # the implementation's own text, before it touches the device
        add(name, *with_(lmd=-1.0, mu=1.0))

    # -- the operator: a null handle, and what is tested before it
    add("saa_operator_order", None)
    add("saa_operator_order", "@hollow")
    add("saa_operator_load", None, 0.0, 0.0, 1.0, "@p")
    add("saa_operator_diagonal", None, "@p", "@p")
    add("saa_operator_set_stream", None, None)
    add("saa_operator_apply", None, 0, None, -1, None, None, -1)
    add("saa_operator_apply", "@hollow", 1, "@p", 15, "@p", "@p", 15)
    add("saa_operator_element_bound", None, "@p", "@d", "@i", "@i")
    add("saa_operator_lumped_mass", None, "@p")
    for name in MAT:
        tail = ("@d", "@i", "@n") if name == "saa_operator_tangent_bound" else ("@p", "@n")
        for material in (-1, 3):
            add(name, None, material, "@p", "@p", *tail)
        add(name, None, 2, "@p", "@p", *tail)
    for material in (-1, 3):
        add("saa_operator_shifted_apply", None, material, "@p", "@p", None, "@p", None, "@n")
    add("saa_operator_shifted_apply", None, 1, "@p", "@p", None, "@p", None, "@n")
    # op, material, u, m, v, ldv, kv, ldkv, n_inverted: material, then m, then the sign of the leading dimensions, then the handle
    add("saa_operator_tangent_apply_block", None, 3, "@p", 0, "@p", -1, "@p", -1, "@n")
    add("saa_operator_tangent_apply_block", None, 0, "@p", 0, "@p", -1, "@p", -1, "@n")
    add("saa_operator_tangent_apply_block", None, 0, "@p", 17, "@p", 15, "@p", 15, "@n")
    add("saa_operator_tangent_apply_block", None, 1, "@p", 16, "@p", -1, "@p", 15, "@n")
    add("saa_operator_tangent_apply_block", None, 1, "@p", 1, "@p", 15, "@p", -1, "@n")
    add("saa_operator_tangent_apply_block", None, 2, "@p", 1, "@p", 0, "@p", 0, "@n")

    # -- stress recovery: the linear three test the handle first, the order-2 three the column count once op is not null
    add("saa_operator_stress", None, 0, None, 0, None, 0, None, None, 0, None, None, None)
    add("saa_operator_stress", "@hollow", 0, None, 0, None, 0, None, None, 0, None, None, None)
    add("saa_operator_nodal_average", None, 0, 0, None, 0, None, 0)
    add("saa_operator_stress_error", None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
    for m in (0, 1):
        for h in (None, "@hollow"):
            add("saa_operator_stress_p2", h, m, None, 0, None, 0, None, 0, None, 0, None, None, None)
            add("saa_operator_nodal_stress_p2", h, m, None, 0, None, 0)
            add("saa_operator_stress_error_p2", h, m, None, 0, None, 0, None, 0, None, 0, None, None, None)
    # op, material, measure, m, x, ldx, then (pointer, ld) of stress, von Mises, det F and energy, three totals, n_inverted
    rest = (0, None, 0, None, 0, None, 0, None, 0, None, None, None, None)
    for material in (0, 3, -1):
        add("saa_operator_stress_finite", None, material, 7, 0, None, *rest)
    for measure in (-1, 2):
        add("saa_operator_stress_finite", None, 1, measure, 0, None, *rest)
    add("saa_operator_stress_finite", None, 2, 1, 0, None, *rest)
    add("saa_operator_stress_finite", "@hollow", 2, 1, 0, None, *rest)     # x_dev, then m, then what op points to
    add("saa_operator_stress_finite", "@hollow", 2, 1, 17, "@p", *rest)
    add("saa_operator_stress_finite", "@hollow", 2, 1, 16, "@p", *rest)

    # -- the explicit stepper: op, mass, f_ext, dt, alpha, ramp, out
    add("saa_operator_stepper_create", None, "@p", "@p", 0.0, -1.0, 1, None)
    for dt in (0.0, -1e-3, "nan", "inf"):
        add("saa_operator_stepper_create", None, "@p", "@p", dt, -1.0, 1, "@out")
    for alpha in (-0.5, "nan", "inf"):
        add("saa_operator_stepper_create", None, "@p", "@p", 1e-3, alpha, 1, "@out")
    add("saa_operator_stepper_create", None, None, None, 1e-3, 0.0, 1, "@out")
    add("saa_operator_stepper_create", "@hollow", "@p", "@p", 1e-3, 0.5, 0, "@out")
    add("saa_operator_stepper_set_state", None, None, None, "nan")
    add("saa_operator_stepper_get_state", None, None, None, None)
    add("saa_operator_stepper_set_recorder", None, "@p", 0, 0, -1)
    add("saa_operator_stepper_set_option", None, "passes", 3.0)
    add("saa_operator_stepper_set_option", None, None, 3.0)
    add("saa_operator_stepper_set_option", "@hollow", "passes", 3.0)
    add("saa_operator_stepper_step", None, -1)
    add("saa_operator_stepper_set_shared", None, -1, None, None, -2)
    add("saa_operator_stepper_set_interface_buffer", None, None)
    add("saa_operator_stepper_step_begin", None)
    add("saa_operator_stepper_step_finish", None, "@p", -1)
    add("saa_operator_stepper_step_predicted", None, -1, None, -1, "@p", -1)
    add("saa_operator_stepper_halo_gather", None, None)
    add("saa_operator_stepper_halo_scatter", None, None)
    # st, energy, n_rows, every, next_step_index, shared_owned: the three numbers, in that order, then the handle
    add("saa_operator_stepper_set_energy", None, "@p", -1, 0, -1, None)
    add("saa_operator_stepper_set_energy", None, "@p", 0, 0, -1, None)
    add("saa_operator_stepper_set_energy", None, "@p", 4, 1, -1, None)
    add("saa_operator_stepper_set_energy", None, "@p", 4, 1, 0, None)
    for material in (-1, 3):
        add("saa_operator_stepper_set_material", None, material)
    add("saa_operator_stepper_set_material", None, 1)
    add("saa_operator_stepper_inverted", None, "@n", "@n")
    add("saa_operator_stepper_set_dt", None, "nan")

    # -- the implicit stepper: op, mass, f_ext, dt, alpha, ramp, material, out
    add("saa_operator_implicit_create", None, "@p", "@p", 0.0, -1.0, 1, 3, None)
    for dt in (0.0, "nan", "-inf"):
        add("saa_operator_implicit_create", None, "@p", "@p", dt, -1.0, 1, 3, "@out")
    for alpha in (-1.0, "nan"):
        add("saa_operator_implicit_create", None, "@p", "@p", 1e-3, alpha, 1, 3, "@out")
    for material in (3, -1):
        add("saa_operator_implicit_create", None, "@p", "@p", 1e-3, 0.5, 1, material, "@out")
    add("saa_operator_implicit_create", None, None, None, 1e-3, 0.5, 1, 2, "@out")
    add("saa_operator_implicit_set_state", None, None, None, "inf")
    add("saa_operator_implicit_get_state", None, None, None, None, None)
    add("saa_operator_implicit_set_recorder", None, "@p", 0, 0, -1)
    add("saa_operator_implicit_set_option", None, "tol", 1e-8)
    add("saa_operator_implicit_set_option", None, None, 1e-8)
    add("saa_operator_implicit_set_dt", None, 0.0)
    add("saa_operator_implicit_step", None, -1, None)
    return out


CASES = _cases()


def run():
    """The record of every case, and what must outlive the calls."""
    from synchronization_avoiding_algorithms_amd import _lib

    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    arrays = {
        "xyz": np.random.default_rng(0).random(3 * 14),
        "tets": np.array([0, 1, 2, 3, 1, 2, 3, 4], dtype=np.int32),
        "tets_high": np.array([0, 1, 2, 3, 1, 2, 3, 5], dtype=np.int32),
        "tets_negative": np.array([0, 1, 2, 3, -1, 2, 3, 4], dtype=np.int32),
        "cells10": np.array([*range(10), *range(4, 14)], dtype=np.int32),
        "cells10_high": np.array([*range(10), *range(5, 15)], dtype=np.int32),
        "cells10_negative": np.array([*range(10), *range(-1, 9)], dtype=np.int32),
        "dd": np.array([0, 1, 2], dtype=np.int32),
        "dd_high": np.array([0, 1, 15], dtype=np.int32),
        "dd_high_p2": np.array([0, 1, 42], dtype=np.int32),
        "dd_negative": np.array([0, -1, 2], dtype=np.int32),
    }
    handle, hollow, scratch = C.c_void_p(), C.c_void_p(), (C.c_double * 8)()
    number, index, count = C.c_double(), C.c_int32(), C.c_int64()
    env = {k: v.ctypes.data_as(dp if v.dtype == np.float64 else ip) for k, v in arrays.items()}
    env.update(out=C.byref(handle), hollow=C.addressof(hollow), p=C.addressof(scratch), d=C.pointer(number), i=C.pointer(index),
               n=C.pointer(count))
    records = []
    for name, args in CASES:
        handle.value = 0xdead                                        # a create sets *out = NULL before its first check
        records.append(refusals.call(lib, name, args, env))
        assert handle.value == (None if "@out" in args else 0xdead), (name, args)
    return records, (arrays, scratch)


def test_refusals_without_a_device_are_those_of_the_fixture():
    got, _ = run()
    refusals.compare(got, refusals.expected(CASES))
    from synchronization_avoiding_algorithms_amd import _lib

    family = {n for n in _lib.SIGNATURES if n.startswith("saa_operator_") and not n.endswith("_destroy")}
    assert {r["call"] for r in got} == family                       # every entry point of the family but the three destroys
    assert {r["rc"] for r in got} == {_lib.SAA_E_ARG, _lib.SAA_E_CAPACITY}


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_operator_refusals.py --write")
    refusals.write(run()[0], first=True)
