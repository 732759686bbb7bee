#!/usr/bin/env python3
"""What following the time step costs on one MI355X: us per call of the bound pass ``saa_operator_tangent_bound`` per material,
of one ``saa_operator_stepper_set_dt``, of one plain step, of one ``saa_operator_tangent_apply`` and of one Lanczos check
(``OperatorStepper.stable_time_step``) on structured_beam(n) (n = 19: 1 028 850 tets), as it is at order 1 and elevated to
order 2, and from them the share of a run spent following with a check every 10 steps.  The device cases are timed alternately,
twice each, with HIP events around regions of at least ``--seconds`` after a warm-up of every case; both rounds are printed and
the smaller is used.  A bound call and a Lanczos check synchronise, so their figures hold the host's part too; the Lanczos check
is a host loop and is timed by the wall clock, twice.  Writes one text file (default profiles/dt_follow_kernel_stats.txt).

    python tools/dt_follow_point.py [--n 19] [--seconds 1.0] [--out FILE]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from p2_step_point import timed  # noqa: E402

EVERY = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dt_follow_kernel_stats.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.load()
    lmd, mu = fs.lame(1e6, 0.3)
    say(f"Following the time step on the operator handle, one {torch.cuda.get_device_name(0)}: us per call.")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, the cases alternating, "
        f"two rounds; the smaller of each is used below.  State u: a smooth field at max|H| about 1e-2, released at rest; material of "
        f"the stepper: svk.  A bound call synchronises the stream (it returns the maximum), so its figure includes that wait.")
    best = {}
    base = structured_beam(args.n)
    for order in (2, 1):
        mesh = to_quadratic(base) if order == 2 else base
        cells = mesh.tets10 if order == 2 else mesh.tets
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {len(cells)} tets, {len(mesh.points)} nodes")
        say(f"{'case':44s} {'us/call':>10s} {'calls':>7s}")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0) as op:
            x = np.asarray(mesh.points, dtype=np.float64)
            u = np.zeros_like(x)
            u[:, 1] = 2e-4 * x[:, 0] ** 2
            u[:, 2] = 1e-2 * np.sin(0.5 * x[:, 0])
            u = torch.as_tensor(u.reshape(-1), device=op.torch_device) * op.free
            g = torch.Generator(device="cpu").manual_seed(0)
            v = (torch.rand(op.n_dof, generator=g, dtype=torch.float64) - 0.5).to(op.torch_device)
            y = torch.empty_like(v)
            pu, pv, py = (C.c_void_p(t.data_ptr()) for t in (u, v, y))
            mass = op.lumped_mass()
            bound0 = op.tangent_bound(None, "linear")
            dt = 0.9 * 2.0 / bound0["omega_max"]                       # certified for the linear operator: no Lanczos needed here
            with OperatorStepper(op, mass, torch.zeros_like(u), dt, 0.5, ramp=True, material="svk") as st:
                st.set_state(u, u, 0.0)
                w, arg = C.c_double(), C.c_int32()

                def bound(mat):
                    def run(n):
                        for _ in range(n):
                            _lib.check(lib.saa_operator_tangent_bound(op._h, mat, pu, None, C.byref(w), C.byref(arg), None))
                    return run

                def set_dt(n):                                         # (the same dt launches nothing: alternate two values)
                    for k in range(n):
                        _lib.check(lib.saa_operator_stepper_set_dt(st._h, dt * (0.99 if k % 2 == 0 else 1.0)))

                def step(n):
                    _lib.check(lib.saa_operator_stepper_step(st._h, n))

                def tangent(n):
                    for _ in range(n):
                        _lib.check(lib.saa_operator_tangent_apply(op._h, 1, pu, pv, py, None))

                cases = [("bound, linear", bound(0)), ("bound, svk", bound(1)), ("bound, neo_hookean", bound(2)), ("set_dt (svk)", set_dt),
                         ("plain step (svk)", step), ("tangent apply (svk)", tangent)]
                for _, fn in cases:
                    fn(10)
                torch.cuda.synchronize()
                for rnd in (1, 2):
                    for name, fn in cases:
                        us, calls = timed(fn, args.seconds)
                        best[(order, name)] = min(best.get((order, name), us), us)
                        say(f"{f'order {order}, {name} (round {rnd})':44s} {us:10.1f} {calls:7d}")
                st.set_dt(dt)
                st.set_state(u, u, 0.0)
                for rnd in (1, 2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    chk = st.stable_time_step()
                    torch.cuda.synchronize()
                    us = 1e6 * (time.perf_counter() - t0)
                    best[(order, "lanczos check")] = min(best.get((order, "lanczos check"), us), us)
                    say(f"{f'order {order}, Lanczos check (round {rnd}, wall)':44s} {us:10.1f} {1:7d}")
                b = op.tangent_bound(u, "svk")
                say(f"  bound(0) {bound0['omega_max']:.6e}, bound(u) svk {b['omega_max']:.6e} at element {b['element']}, counts "
                    f"{(b['n_nonpositive'], b['n_inverted'], b['n_nonfinite'])}; Lanczos omega_max(u) {chk['omega_max']:.6e}: bound / Lanczos "
                    f"{b['omega_max'] / chk['omega_max']:.3f}")
    say()
    say(f"{'order':6s} {'bound svk / tangent apply':>26s} {'bound svk / step':>17s} {'Lanczos check / bound svk':>26s} "
        f"{f'share of a run following, S = {EVERY}':>34s}")
    for order in (2, 1):
        bd, sd, stp = best[(order, "bound, svk")], best[(order, "set_dt (svk)")], best[(order, "plain step (svk)")]
        share = (bd + sd) / (EVERY * stp + bd + sd)
        say(f"{order:<6d} {bd / best[(order, 'tangent apply (svk)')]:26.2f} {bd / stp:17.2f} {best[(order, 'lanczos check')] / bd:26.1f} "
            f"{100 * share:33.1f}%")
    say("(the share counts one bound pass and one set_dt per check; a check that leaves dt alone costs the bound pass only)")
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_opdt.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_opdt.hip"],
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
