#!/usr/bin/env python3
"""Timings of the partitioned step on the order-2 operator stepper on one MI355X: structured_beam(n) elevated (n = 19:
1 028 850 tets) cut in two slabs, rank 0 timed alone (world of one: nothing is reduced, the interface buffer stays what
the rank wrote).  us/step of ``saa_operator_stepper_step`` (the local step), of ``step_begin`` + ``step_finish`` and of
``step_predicted`` from a table of zeros, each timed twice, alternating.  The expectation to be checked: begin + finish
costs one plain step plus one small launch over the shared dofs; a predicted step costs a plain step.  HIP events around
regions of at least ``--seconds`` each after a warm-up of every case.  Writes one text file (default
profiles/p2_part_step_stats.txt).

    python tools/opstep_part_point.py [--n 19] [--seconds 1.0] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2_part_step_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorRank
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, slab_partition, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    mesh = to_quadratic(structured_beam(args.n))
    E, nu, rho, fz, alpha = 1e6, 0.3, 1.0, 0.5, 0.5
    lmd, mu = fs.lame(E, nu)
    dnodes = plane_nodes(mesh.points)
    with ModalOperator(mesh.points, mesh.tets10, fs.node_to_dof(dnodes), lmd, mu, rho, 0) as op:
        mass, load = op.lumped_mass(), op.load((0.0, -fz, -fz))
        ts = stable_time_step_operator(op, mass, 0.9)
        torch.cuda.synchronize()
    layouts, gs = fs.build_layouts(mesh.tets10, slab_partition(mesh, 2), 2, len(mesh.points), dnodes)
    lay = layouts[0]
    say(f"Partitioned step on the order-2 operator stepper, one {torch.cuda.get_device_name(0)}: structured_beam({args.n}) elevated = "
        f"{len(mesh.tets10)} tets, {len(mesh.points)} nodes, cut in two slabs; rank 0 timed alone: {len(lay.elements)} tets, "
        f"{len(lay.nodes)} nodes, {len(lay.shared_local)} shared nodes of {len(gs)} in all.")
    say(f"HRZ mass of the whole mesh; dt = 0.9 * 2/omega_max = {ts['dt']:.6e}.")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first.")
    say()
    say(f"{'case':44s} {'us/step':>9s} {'steps':>7s}")
    best = {}
    with OperatorRank(mesh.points, lay, gs, mass, load, lmd, mu, rho, ts["dt"], alpha) as rank:
        st = rank.stepper
        table = torch.zeros((50, rank.input_size), dtype=torch.float64, device=rank.tensor_device)

        def synced(n):
            for _ in range(n):
                st.step_begin()
                st.step_finish()

        for stored in (0, 1):
            st.set_option("stored_geometry", stored)
            for rnd in (1, 2):
                for name, fn in (("step (local)", st.step), ("step_begin + step_finish", synced),
                                 ("step_predicted", lambda n: st.step_predicted(n, table))):
                    st.set_state(None, None, 0.0)
                    us, steps = timed(fn, args.seconds)
                    key = f"{name}, stored_geometry={stored}"
                    best[key] = min(best.get(key, us), us)
                    say(f"{key + f' (round {rnd})':44s} {us:9.1f} {steps:7d}")
        d0 = st.state()[0]
        say()
        say(f"state after the last run: max|d| = {float(d0.abs().max()):.6e} (finite: {bool(torch.isfinite(d0).all())})")
    for stored in (0, 1):
        a, b, c = (best[f"{k}, stored_geometry={stored}"] for k in ("step (local)", "step_begin + step_finish", "step_predicted"))
        say(f"stored_geometry={stored}: begin + finish - step = {b - a:+.1f} us/step ({b / a:.3f} x); step_predicted - step = "
            f"{c - a:+.1f} us/step ({c / a:.3f} x).")
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
