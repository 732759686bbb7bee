"""The refusals of the operator family of the C API that need a live handle, pinned against
``golden/operator_refusals.json``: return code and message, byte for byte (tests/operator_refusals.py has the record,
tests/test_operator_refusals.py the refusals that need no device).  One order-1 operator on ``structured_beam(1)`` and one
order-2 operator on its elevation; an explicit stepper with a shared set of one node and an interface buffer on the first,
an implicit stepper on the second.  :func:`script` is one sequence of calls: a refused one becomes a record, an accepted one
(a change of state that the next refusals need) must return ``SAA_OK``.  Only ``SAA_E_ARG`` and ``SAA_E_STATE`` are made: a
refused call launches nothing.  After the last refusal both steppers take a step and the operator applies, and the results
are finite: no refusal left a handle behind that does not work.

``python tests/test_gpu_operator_refusals.py --write`` regenerates this part of the fixture (on the GPU)."""
import ctypes as C
import sys

import numpy as np
import pytest

import operator_refusals as refusals

DT, ALPHA = 1e-4, 0.5          # one step is taken: stability is not at stake; 2/ALPHA = 4 is set_dt's bound


def script(R, A):
    """``R(call, *args)``: refused, recorded.  ``A(call, *args)``: accepted."""
    # -- the operator of either order
    R("saa_operator_load", "@op1", 0.0, 0.0, 1.0, None)
    R("saa_operator_load", "@op1", 0.0, "nan", 1.0, "@buf")
    R("saa_operator_load", "@op2", "inf", 0.0, 1.0, "@buf")
    R("saa_operator_diagonal", "@op1", None, None)
    for m in (0, 17):
        R("saa_operator_apply", "@op1", m, None, 0, None, None, 0)
    R("saa_operator_apply", "@op1", 1, None, "@ndof1", "@buf", "@buf", "@ndof1")
    R("saa_operator_apply", "@op1", 1, "@buf", "@ndof1", None, None, "@ndof1")
    R("saa_operator_apply", "@op1", 1, "@buf", "@ndof1-1", "@buf", None, "@ndof1")
    R("saa_operator_apply", "@op2", 16, "@buf", "@ndof2", None, "@buf", "@ndof2-1")
    R("saa_operator_element_bound", "@op2", "@buf", "@d", "@i", "@i")
    R("saa_operator_lumped_mass", "@op2", None)
    # op, material, x, f, energy_elem, n_inverted
    R("saa_operator_internal_force", "@op1", 0, None, "@buf", None, "@n")
    R("saa_operator_internal_force", "@op1", 1, "@buf", None, None, "@n")
    R("saa_operator_internal_force", "@op2", 0, "@buf", "@buf", "@buf", "@n")
    # op, material, u, v, kv, n_inverted
    R("saa_operator_tangent_apply", "@op1", 0, None, None, "@buf", "@n")
    R("saa_operator_tangent_apply", "@op1", 1, None, "@buf", None, "@n")
    for material in (1, 2):
        R("saa_operator_tangent_apply", "@op2", material, None, "@buf", "@buf", "@n")
    # op, material, u, m, v, ldv, kv, ldkv, n_inverted
    R("saa_operator_tangent_apply_block", "@op1", 0, None, 2, None, "@ndof1", "@buf", "@ndof1", "@n")
    R("saa_operator_tangent_apply_block", "@op1", 2, None, 2, "@buf", 0, None, 0, "@n")
    R("saa_operator_tangent_apply_block", "@op1", 2, None, 2, "@buf", 0, "@buf", 0, "@n")
    R("saa_operator_tangent_apply_block", "@op1", 0, None, 2, "@buf", "@ndof1-1", "@buf", "@ndof1", "@n")
    R("saa_operator_tangent_apply_block", "@op2", 1, "@buf", 16, "@buf", "@ndof2", "@buf", "@ndof2-1", "@n")
    # op, material, u, omega_e, omega_max, argmax, counts
    R("saa_operator_tangent_bound", "@op1", 0, None, None, None, "@i", "@n")
    R("saa_operator_tangent_bound", "@op1", 1, None, None, "@d", None, "@n")
    R("saa_operator_tangent_bound", "@op2", 2, None, None, "@d", "@i", "@n")
    # op, material, u, v, shift, out, dot, n_inverted
    R("saa_operator_shifted_apply", "@op1", 0, None, None, None, "@buf", None, "@n")
    R("saa_operator_shifted_apply", "@op1", 1, None, "@buf", None, None, None, "@n")
    R("saa_operator_shifted_apply", "@op2", 1, None, "@buf", None, "@buf", None, "@n")

    # -- stress recovery, order 1.  stress: op, m, x, ldx, sigma, ld_sigma, von_mises, energy, ld_elem, three totals
    R("saa_operator_stress", "@op2", 0, None, 0, None, 0, None, None, 0, None, None, None)
    R("saa_operator_stress", "@op1", 17, None, 0, None, 0, None, None, 0, None, None, None)
    R("saa_operator_stress", "@op1", 1, None, 0, None, 0, None, None, 0, None, None, None)
    R("saa_operator_stress", "@op1", 1, "@buf", "@ndof1-1", "@buf", 0, "@buf", None, 0, None, None, None)
    R("saa_operator_stress", "@op1", 1, "@buf", "@ndof1", "@buf", "@6elems-1", "@buf", None, 0, None, None, None)
    R("saa_operator_stress", "@op1", 1, "@buf", "@ndof1", "@buf", "@6elems", "@buf", None, "@elems-1", None, None, None)
    R("saa_operator_stress", "@op1", 1, "@buf", "@ndof1", None, 0, None, "@buf", "@elems-1", None, None, None)
    # nodal_average: op, m, k, elem, ld_elem, node, ld_node
    R("saa_operator_nodal_average", "@op2", 0, 0, None, 0, None, 0)
    R("saa_operator_nodal_average", "@op1", 0, 0, None, 0, None, 0)
    for k in (0, 9):
        R("saa_operator_nodal_average", "@op1", 1, k, None, 0, None, 0)
    R("saa_operator_nodal_average", "@op1", 1, 6, None, 0, "@buf", 0)
    R("saa_operator_nodal_average", "@op1", 1, 6, "@buf", 0, None, 0)
    R("saa_operator_nodal_average", "@op1", 1, 6, "@buf", "@6elems-1", "@buf", 0)
    R("saa_operator_nodal_average", "@op1", 1, 6, "@buf", "@6elems", "@buf", "@6nodes1-1")
    # stress_error: op, m, sigma_elem, ld_sigma, sigma_node, ld_node, sigma_other, ld_other, eta2, ld_eta, three totals
    R("saa_operator_stress_error", "@op2", 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", 0, "@buf", 0, "@buf", 0, None, 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", "@6elems-1", "@buf", 0, None, 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", "@6elems", "@buf", "@6nodes1-1", None, 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", "@6elems", None, 0, "@buf", "@6elems-1", "@buf", 0, None, None, None)
    R("saa_operator_stress_error", "@op1", 1, "@buf", "@6elems", None, 0, "@buf", "@6elems", "@buf", "@elems-1", None, None, None)
    # -- stress recovery, order 2.  stress_p2: op, m, x, ldx, sigma, ld_sigma, von_mises, ld_vm, energy, ld_elem, three totals
    R("saa_operator_stress_p2", "@op1", 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_p2", "@op1", 1, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_p2", "@op2", 1, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_p2", "@op2", 1, "@buf", "@ndof2-1", "@buf", 0, "@buf", 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_p2", "@op2", 1, "@buf", "@ndof2", "@buf", "@24elems-1", "@buf", 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_p2", "@op2", 1, "@buf", "@ndof2", "@buf", "@24elems", "@buf", "@4elems-1", "@buf", 0, None, None, None)
    R("saa_operator_stress_p2", "@op2", 1, "@buf", "@ndof2", "@buf", "@24elems", "@buf", "@4elems", "@buf", "@elems-1", None, None, None)
    # nodal_stress_p2: op, m, sigma, ld_sigma, sigma_node, ld_node
    R("saa_operator_nodal_stress_p2", "@op1", 17, None, 0, None, 0)
    R("saa_operator_nodal_stress_p2", "@op1", 16, None, 0, None, 0)
    R("saa_operator_nodal_stress_p2", "@op2", 1, None, 0, "@buf", 0)
    R("saa_operator_nodal_stress_p2", "@op2", 1, "@buf", "@24elems-1", None, 0)
    R("saa_operator_nodal_stress_p2", "@op2", 1, "@buf", "@24elems", "@buf", "@6nodes2-1")
    # stress_error_p2: the arguments of stress_error
    R("saa_operator_stress_error_p2", "@op1", 0, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op1", 1, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, None, 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", 0, None, 0, None, 0, None, 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", 0, "@buf", 0, "@buf", 0, None, 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", "@24elems-1", "@buf", 0, None, 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", "@24elems", "@buf", "@6nodes2-1", None, 0, "@buf", 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", "@24elems", None, 0, "@buf", "@24elems-1", "@buf", 0, None, None, None)
    R("saa_operator_stress_error_p2", "@op2", 1, "@buf", "@24elems", None, 0, "@buf", "@24elems", "@buf", "@elems-1", None, None, None)
    # stress_finite: op, material, measure, m, x, ldx, then (pointer, ld) of stress, von Mises, det F and energy, three totals, n_inverted
    none = (None, None, None, None)
    R("saa_operator_stress_finite", "@op1", 1, 0, 0, None, 0, None, 0, None, 0, None, 0, None, 0, *none)
    R("saa_operator_stress_finite", "@op1", 1, 0, 0, "@buf", 0, None, 0, None, 0, None, 0, None, 0, *none)
    R("saa_operator_stress_finite", "@op1", 1, 0, 1, "@buf", "@ndof1-1", "@buf", 0, "@buf", 0, "@buf", 0, "@buf", 0, *none)
    R("saa_operator_stress_finite", "@op1", 1, 0, 1, "@buf", "@ndof1", "@buf", "@6elems-1", "@buf", 0, "@buf", 0, "@buf", 0, *none)
    R("saa_operator_stress_finite", "@op2", 2, 1, 1, "@buf", "@ndof2", "@buf", "@24elems-1", "@buf", 0, "@buf", 0, "@buf", 0, *none)
    R("saa_operator_stress_finite", "@op2", 2, 1, 1, "@buf", "@ndof2", "@buf", "@24elems", "@buf", "@4elems-1", "@buf", 0, "@buf", 0, *none)
    R("saa_operator_stress_finite", "@op2", 2, 1, 1, "@buf", "@ndof2", "@buf", "@24elems", "@buf", "@4elems", "@buf", "@4elems-1", "@buf", 0, *none)
    R("saa_operator_stress_finite", "@op2", 2, 1, 1, "@buf", "@ndof2", "@buf", "@24elems", "@buf", "@4elems", "@buf", "@4elems", "@buf", "@elems-1", *none)

    # -- the two stepper creates on a live operator: op, mass, f_ext, dt, alpha, ramp, (material,) out
    R("saa_operator_stepper_create", "@op1", None, "@buf", DT, ALPHA, 1, "@out")
    R("saa_operator_stepper_create", "@op1", "@buf", None, DT, ALPHA, 1, "@out")
    R("saa_operator_stepper_create", "@op1", "@buf", "@buf", DT, ALPHA, 1, "@out")            # (a mass of zeros: the implementation's text)
    R("saa_operator_implicit_create", "@op2", None, "@buf", DT, ALPHA, 1, 0, "@out")
    R("saa_operator_implicit_create", "@op2", "@buf", None, DT, ALPHA, 1, 0, "@out")
    R("saa_operator_implicit_create", "@op2", "@buf", "@buf", DT, ALPHA, 1, 1, "@out")

    # -- the explicit stepper at rest, with its shared set (node 5, slot 0 of 1) and its interface buffer
    R("saa_operator_stepper_set_state", "@st", None, None, "nan")
    R("saa_operator_stepper_set_state", "@st", None, None, "-inf")
    for bad in ((0, 1, 0), (4, 0, 0), (4, 1, -1)):
        R("saa_operator_stepper_set_recorder", "@st", "@buf", *bad)
    R("saa_operator_stepper_set_option", "@st", None, 1.0)
    R("saa_operator_stepper_set_option", "@st", "stored", 1.0)
    R("saa_operator_stepper_set_option", "@st", "stored_geometry", 2.0)
    R("saa_operator_stepper_set_option", "@st", "passes", 4.0)
    R("saa_operator_stepper_step", "@st", -1)
    R("saa_operator_stepper_set_shared", "@st", -1, "@node", "@slot", 1)
    R("saa_operator_stepper_set_shared", "@st", 2, "@node", "@slot", 1)
    R("saa_operator_stepper_set_shared", "@st", 1, None, "@slot", 1)
    R("saa_operator_stepper_set_shared", "@st", 1, "@node", None, 1)
    R("saa_operator_stepper_set_shared", "@st", 1, "@node_high", "@slot", 1)                  # (the implementation's texts)
    R("saa_operator_stepper_set_shared", "@st", 1, "@node", "@slot_high", 1)
    R("saa_operator_stepper_set_shared", "@st", 2, "@node_twice", "@slots", 2)
    R("saa_operator_stepper_step_finish", "@st", "@buf", -1)
    R("saa_operator_stepper_step_finish", "@st", None, 0)
    R("saa_operator_stepper_step_predicted", "@st", -1, "@buf", 0, None, 0)
    R("saa_operator_stepper_step_predicted", "@st", 1, "@buf", -1, None, 0)
    R("saa_operator_stepper_step_predicted", "@st", 1, "@buf", 0, "@buf", -1)
    R("saa_operator_stepper_step_predicted", "@st", 1, None, 0, None, 0)
    R("saa_operator_stepper_halo_gather", "@st", None)
    R("saa_operator_stepper_halo_scatter", "@st", None)
    R("saa_operator_stepper_set_dt", "@st", "nan")
    R("saa_operator_stepper_set_dt", "@st", 0.0)
    R("saa_operator_stepper_set_dt", "@st", 4.0)
    R("saa_operator_stepper_set_dt", "@st", DT / 2)                                            # a shared set is in place
    A("saa_operator_stepper_set_interface_buffer", "@st", None)
    R("saa_operator_stepper_step_begin", "@st")
    A("saa_operator_stepper_set_interface_buffer", "@st", "@iface")

    # -- between step_begin and step_finish: everything that changes the stepper is refused
    A("saa_operator_stepper_step_begin", "@st")
    R("saa_operator_stepper_set_state", "@st", None, None, 0.0)
    R("saa_operator_stepper_set_recorder", "@st", None, 0, 1, 0)
    R("saa_operator_stepper_set_option", "@st", "passes", 3.0)
    R("saa_operator_stepper_step", "@st", 1)
    R("saa_operator_stepper_set_shared", "@st", 0, None, None, 0)
    R("saa_operator_stepper_set_interface_buffer", "@st", "@iface")
    R("saa_operator_stepper_step_begin", "@st")
    R("saa_operator_stepper_step_predicted", "@st", 1, "@buf", 0, None, 0)
    R("saa_operator_stepper_halo_scatter", "@st", "@buf")
    R("saa_operator_stepper_set_energy", "@st", None, 0, 1, 0, None)
    R("saa_operator_stepper_set_material", "@st", 1)
    R("saa_operator_stepper_set_dt", "@st", DT / 2)
    A("saa_operator_stepper_step_finish", "@st", None, 0)

    # -- the states that the energy balance, the passes option and the material exclude
    A("saa_operator_stepper_set_energy", "@st", "@energy", 4, 1, 0, None)
    R("saa_operator_stepper_set_option", "@st", "passes", 2.0)
    R("saa_operator_stepper_set_material", "@st", 2)
    A("saa_operator_stepper_set_shared", "@st", 0, None, None, 0)                            # (switches the energy balance off)
    A("saa_operator_stepper_set_energy", "@st", "@energy", 4, 1, 0, None)
    R("saa_operator_stepper_set_dt", "@st", DT / 2)                                            # the energy balance is recorded
    A("saa_operator_stepper_set_energy", "@st", None, 0, 1, 0, None)
    A("saa_operator_stepper_set_option", "@st", "passes", 2.0)
    R("saa_operator_stepper_set_dt", "@st", DT / 2)                                            # passes is 2
    R("saa_operator_stepper_set_energy", "@st", "@energy", 4, 1, 0, None)
    A("saa_operator_stepper_set_option", "@st", "passes", 3.0)
    A("saa_operator_stepper_set_material", "@st", 1)
    R("saa_operator_stepper_set_energy", "@st", "@energy", 4, 1, 0, None)
    A("saa_operator_stepper_set_material", "@st", 0)

    # -- the implicit stepper
    R("saa_operator_implicit_set_state", "@imp", None, None, "nan")
    for bad in ((0, 1, 0), (4, 0, 0), (4, 1, -1)):
        R("saa_operator_implicit_set_recorder", "@imp", "@buf", *bad)
    R("saa_operator_implicit_set_option", "@imp", None, 1.0)
    R("saa_operator_implicit_set_option", "@imp", "tolerance", 1e-8)
    R("saa_operator_implicit_set_option", "@imp", "tol", 1.0)
    R("saa_operator_implicit_set_option", "@imp", "max_newton", 0.5)
    R("saa_operator_implicit_set_option", "@imp", "max_cg", "nan")
    R("saa_operator_implicit_set_dt", "@imp", 0.0)
    R("saa_operator_implicit_set_dt", "@imp", "inf")
    R("saa_operator_implicit_step", "@imp", -1, "@info")
    R("saa_operator_implicit_step", "@imp", 1, None)


def run():
    """The records of :func:`script`; then one accepted step of each stepper and one apply."""
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper, OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    lib = _lib.load()
    mesh = structured_beam(1)
    quad = to_quadratic(mesh)
    lmd, mu = fs.lame(1e6, 0.3)
    ip = C.POINTER(C.c_int32)
    with ModalOperator(mesh.points, mesh.tets, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0) as op1, \
            ModalOperator(quad.points, quad.tets10, fs.node_to_dof(plane_nodes(quad.points)), lmd, mu, 1.0, 0) as op2:
        dev = op1.torch_device
        n_elems = op1.n_elems
        assert op2.n_elems == n_elems and (op1.order, op2.order) == (1, 2)
        sizes = {"ndof1": op1.n_dof, "ndof2": op2.n_dof, "elems": n_elems, "4elems": 4 * n_elems, "6elems": 6 * n_elems,
                 "24elems": 24 * n_elems, "6nodes1": 6 * op1.n_nodes, "6nodes2": 6 * op2.n_nodes}
        zeros = torch.zeros(16 * 24 * n_elems, dtype=torch.float64, device=dev)   # no refused call reads or writes it
        iface = torch.zeros(3, dtype=torch.float64, device=dev)
        energy = torch.zeros((4, 5), dtype=torch.float64, device=dev)
        lists = {"node": [5], "slot": [0], "node_high": [op1.n_nodes], "slot_high": [1], "node_twice": [5, 5], "slots": [0, 1]}
        lists = {k: np.array(v, dtype=np.int32) for k, v in lists.items()}
        handle, number, index, count, info = C.c_void_p(), C.c_double(), C.c_int32(), C.c_int64(), _lib.ImplicitInfo()
        with OperatorStepper(op1, op1.lumped_mass(), op1.load((0.0, -0.5, -0.5)), DT, ALPHA) as st, \
                ImplicitStepper(op2, op2.lumped_mass(), op2.load((0.0, -0.5, -0.5)), 100 * DT, ALPHA) as imp:
            st.set_shared(lists["node"], lists["slot"], 1)
            st.set_interface_buffer(iface)
            env = {**sizes, **{k + "-1": v - 1 for k, v in sizes.items()}, **{k: v.ctypes.data_as(ip) for k, v in lists.items()},
                   "op1": op1._h, "op2": op2._h, "st": st._h, "imp": imp._h, "buf": C.c_void_p(zeros.data_ptr()),
                   "iface": C.c_void_p(iface.data_ptr()), "energy": C.c_void_p(energy.data_ptr()), "out": C.byref(handle),
                   "d": C.pointer(number), "i": C.pointer(index), "n": C.pointer(count), "info": C.byref(info)}
            records = []

            def refused(name, *args):
                handle.value = 0xdead                                # a create sets *out = NULL before its first check
                records.append(refusals.call(lib, name, args, env))
                assert handle.value == (None if "@out" in args else 0xdead), (name, args)

            def accepted(name, *args):
                rc = getattr(lib, name)(*[refusals.resolve(a, env) for a in args])
                assert rc == _lib.SAA_OK, (name, args, rc, lib.saa_last_error())

            script(refused, accepted)
            # every handle still works
            st.step(1)
            done = imp.step(1)
            kx, _ = op1.apply(st.state()[0])
            torch.cuda.synchronize(dev)
            assert done["converged"] and done["steps_done"] == 1 and imp.steps_done == 1
            assert st.steps_done == 1                                # (the split step went past the Python counter)
            d0, _, tn = st.state()
            assert bool(torch.isfinite(d0).all()) and float(d0.abs().max()) > 0.0 and bool(torch.isfinite(kx).all())
            assert abs(tn - 2 * DT) < 1e-18 and abs(imp.state()[3] - 100 * DT) < 1e-18
            assert float(zeros.abs().max()) == 0.0
    return records


@pytest.mark.gpu
def test_refusals_on_live_handles_are_those_of_the_fixture():
    from synchronization_avoiding_algorithms_amd import _lib

    got = run()
    refusals.compare(got, refusals.expected([(r["call"], r["args"]) for r in got]))
    assert {r["rc"] for r in got} == {_lib.SAA_E_ARG, _lib.SAA_E_STATE}
    in_flight = [r for r in got if r["message"].endswith("a synchronised step is in flight")]
    assert len(in_flight) == 11 and all(r["rc"] == _lib.SAA_E_STATE for r in in_flight)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_gpu_operator_refusals.py --write")
    refusals.write(run(), first=False)
