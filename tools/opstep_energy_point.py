#!/usr/bin/env python3
"""What the energy balance costs on the operator stepper on one MI355X: us/step with ``record_energy`` on against off, on
structured_beam(n) (n = 19: 1 028 850 tets) elevated to order 2 and as it is at order 1, for the whole mesh
(``saa_operator_stepper_step``) and for rank 0 of two slabs timed alone (``step_begin`` + ``step_finish`` and
``step_predicted`` from a table of zeros; a world of one: nothing is reduced).  Off launches the ENERGY = false instantiations
of the node and finish passes, which carry none of the balance - the resource rows of saa_opstep.hip below show both - so the
ratio on / off is the cost of the feature.  The two are timed alternately, twice each, with HIP events around regions of at least ``--seconds`` after a warm-up of every case;
the smaller of the two rounds is compared and both are printed, so the spread can be read next to the difference.
Writes one text file (default profiles/p2_energy_step_stats.txt).

    python tools/opstep_energy_point.py [--n 19] [--seconds 1.0] [--out FILE]
"""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2_energy_step_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorRank, OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, slab_partition, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    E, nu, rho, fz, alpha = 1e6, 0.3, 1.0, 0.5, 0.5
    lmd, mu = fs.lame(E, nu)
    say(f"Energy balance on the operator stepper, one {torch.cuda.get_device_name(0)}: us/step with record_energy on against off "
        f"(off = the ENERGY = false instantiations).")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, off and on alternating, "
        f"two rounds; the ratio compares the smaller of each.")
    best = {}

    def compare(key, st, fn):
        for rnd in (1, 2):
            for on in (0, 1):
                st.set_state(None, None, 0.0)
                st.record_energy(64 if on else 0, every=1000)       # (a row every 1000 steps: W and D are summed every step)
                us, steps = timed(fn, args.seconds)
                k = (key, on)
                best[k] = min(best.get(k, us), us)
                say(f"{key + (', energy on' if on else ', energy off') + f' (round {rnd})':64s} {us:9.1f} {steps:7d}")
        st.record_energy(0)

    linear = structured_beam(args.n)
    for order in (2, 1):
        mesh = to_quadratic(linear) if order == 2 else linear
        cells = mesh.tets10 if order == 2 else mesh.tets
        dnodes = plane_nodes(mesh.points)
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {len(cells)} tets, {len(mesh.points)} nodes")
        say(f"{'case':64s} {'us/step':>9s} {'steps':>7s}")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(dnodes), lmd, mu, rho, 0) as op:
            mass, load = op.lumped_mass(), op.load((0.0, -fz, -fz))
            ts = stable_time_step_operator(op, mass, 0.9)
            with OperatorStepper(op, mass, load, ts["dt"], alpha) as st:
                if order == 2:
                    st.set_option("stored_geometry", 1)
                compare(f"order {order}, whole mesh, step", st, st.step)
                d0 = st.state()[0]
                say(f"  dt = 0.9 * 2/omega_max = {ts['dt']:.6e}; state after the last run: max|d| = {float(d0.abs().max()):.6e} "
                    f"(finite: {bool(torch.isfinite(d0).all())})")
            torch.cuda.synchronize()
        layouts, gs = fs.build_layouts(cells, slab_partition(mesh, 2), 2, len(mesh.points), dnodes)
        lay = layouts[0]
        with OperatorRank(mesh.points, lay, gs, mass, load, lmd, mu, rho, ts["dt"], alpha, stored_geometry=1 if order == 2 else None,
                          layouts=layouts) as rank:
            st = rank.stepper
            say(f"  rank 0 of two slabs: {len(lay.elements)} tets, {len(lay.nodes)} nodes, {len(lay.shared_local)} shared nodes")
            table = torch.zeros((50, rank.input_size), dtype=torch.float64, device=rank.tensor_device)

            def synced(n):
                for _ in range(n):
                    st.step_begin()
                    st.step_finish()

            compare(f"order {order}, rank 0 of 2, step_begin + step_finish", st, synced)
            compare(f"order {order}, rank 0 of 2, step_predicted", st, lambda n: st.step_predicted(n, table))
    say()
    say(f"{'case':56s} {'off':>9s} {'on':>9s} {'on - off':>9s} {'on / off':>9s}")
    for key in dict.fromkeys(k for k, _ in best):
        off, on = best[(key, 0)], best[(key, 1)]
        say(f"{key:56s} {off:9.1f} {on:9.1f} {on - off:+9.1f} {on / off:9.3f}")
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_opstep.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opstep.hip"],
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
