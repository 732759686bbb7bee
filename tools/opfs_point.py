#!/usr/bin/env python3
"""What a finite-strain material costs on the operator stepper on one MI355X: us/step of the whole-mesh step
(``saa_operator_stepper_step``) with the material ``linear``, ``svk`` and ``neo_hookean`` on structured_beam(n) (n = 19:
1 028 850 tets), as it is at order 1 and elevated to order 2.  The linear step is the parent's - the same kernels, which the
unchanged resource rows of saa_opstep.hip below show -, at order 2 with the stored geometry (the pass the finite-strain
kernel is shaped after, reading the same table) and also with the recomputing default.  The variants are timed alternately,
twice each, with HIP events around regions of at least ``--seconds`` after a warm-up of every case; the smaller of the two
rounds is compared and both are printed, so the spread can be read next to the difference.  The bytes a step has to move,
by count, stand next to the times.  Writes one text file (default profiles/opfs_step_stats.txt).

    python tools/opfs_point.py [--n 19] [--seconds 1.0] [--out FILE]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from p2_step_point import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opfs_step_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    bw = C.c_double()
    _lib.check(_lib.load().saa_device_copy_bandwidth(0, 1 << 30, 10, C.byref(bw)))
    bw = bw.value
    E, nu, rho, fz, alpha = 1e6, 0.3, 1.0, 0.5, 0.5
    lmd, mu = fs.lame(E, nu)
    say(f"Finite-strain materials on the operator stepper, one {torch.cuda.get_device_name(0)}: us/step of the whole-mesh step by "
        f"material (linear = the parent's kernels).")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, the variants "
        f"alternating, two rounds; the ratios compare the smaller of each.  State: from rest under the ramped load (0, -fz, -fz), "
        f"fz = {fz}: the arithmetic of a step does not depend on the state.")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a step has to move, by count (each array once; ne elements, nn nodes, npe nodes per element):")
    say("  node/update pass, both orders:      4 npe ne (pairs) + 8 nn (offsets) + 24 npe ne (contributions) + 144 nn")
    say("  order 2 element pass, stored table: 40 ne (cells) + 324 ne (geometry, bits) + 24 nn (d0) + 240 ne (contributions)")
    say("     - the linear stored-geometry pass and both finite-strain passes alike")
    say("  order 2 element pass, recomputing:  40 ne (cells) + 48 nn (coordinates, mask) + 24 nn (d0) + 240 ne (contributions)")
    say("  order 1 element pass, all three:    16 ne (cells) + 48 nn (coordinates, mask) + 24 nn (d0) + 96 ne (contributions)")
    best, nbytes = {}, {}

    def compare(order, st, variants):
        for name, setup in variants:                                  # warm-up of every case
            setup()
            st.step(10)
        torch.cuda.synchronize()
        for rnd in (1, 2):
            for name, setup in variants:
                setup()
                st.set_state(None, None, 0.0)
                us, steps = timed(st.step, args.seconds)
                key = (order, name)
                best[key] = min(best.get(key, us), us)
                b = nbytes[key]
                say(f"{f'order {order}, {name} (round {rnd})':52s} {us:9.1f} {steps:7d} {b / 1e9:9.3f} {b / (1e-6 * us) / 1e12:6.3f} "
                    f"{b / (1e-6 * us) / bw:10.2f}")

    linear = structured_beam(args.n)
    for order in (2, 1):
        mesh = to_quadratic(linear) if order == 2 else linear
        cells = mesh.tets10 if order == 2 else mesh.tets
        ne, nn, npe = len(cells), len(mesh.points), 10 if order == 2 else 4
        b_nd = 4 * npe * ne + 8 * nn + 24 * npe * ne + 144 * nn
        b_st = 40 * ne + 324 * ne + 24 * nn + 240 * ne
        b_re = 40 * ne + 48 * nn + 24 * nn + 240 * ne
        b_p1 = 16 * ne + 48 * nn + 24 * nn + 96 * ne
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {ne} tets, {nn} nodes")
        say(f"{'case':52s} {'us/step':>9s} {'steps':>7s} {'GB moved':>9s} {'TB/s':>6s} {'of copy bw':>10s}")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, rho, 0) as op:
            mass, load = op.lumped_mass(), op.load((0.0, -fz, -fz))
            ts = stable_time_step_operator(op, mass, 0.9)
            with OperatorStepper(op, mass, load, ts["dt"], alpha) as st:
                def linear_case(stored):
                    st.set_material("linear")
                    st.set_option("stored_geometry", stored)

                if order == 2:
                    variants = [("linear, stored geometry", lambda: linear_case(1)), ("linear, recomputing", lambda: linear_case(0)),
                                ("svk", lambda: st.set_material("svk")), ("neo_hookean", lambda: st.set_material("neo_hookean"))]
                    for name, _ in variants:
                        nbytes[(order, name)] = (b_re if name == "linear, recomputing" else b_st) + b_nd
                else:
                    variants = [("linear", lambda: st.set_material("linear")), ("svk", lambda: st.set_material("svk")),
                                ("neo_hookean", lambda: st.set_material("neo_hookean"))]
                    for name, _ in variants:
                        nbytes[(order, name)] = b_p1 + b_nd
                compare(order, st, variants)
                d0 = st.state()[0]
                say(f"  dt = 0.9 * 2/omega_max = {ts['dt']:.6e} of the linear operator; state after the last run: max|d| = "
                    f"{float(d0.abs().max()):.6e} (finite: {bool(torch.isfinite(d0).all())}), inverted {st.inverted()}")
            torch.cuda.synchronize()
    say()
    say(f"{'case':40s} {'us/step':>9s} {'/ linear':>9s} {'/ linear, stored':>17s}")
    for (order, name), us in best.items():
        base = best[(order, "linear, recomputing" if order == 2 else "linear")]
        stored = f"{us / best[(2, 'linear, stored geometry')]:17.3f}" if order == 2 else ""
        say(f"{f'order {order}, {name}':40s} {us:9.1f} {us / base:9.3f} {stored}")
    say("(/ linear: against the parent's default step of that order - at order 2 the recomputing pass.)")
    for file in ("saa_opfs.hip", "saa_opstep.hip"):
        say()
        say(f"Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file={file}):")
        if os.path.exists("/opt/rocm/bin/hipcc"):
            res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), f"--file={file}"],
                                 capture_output=True, text=True)
            for ln in res.stdout.splitlines():
                say("  " + ln)
        else:
            say("  hipcc not installed here: not measured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
