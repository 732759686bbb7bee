#!/usr/bin/env python3
"""Timings of the explicit step on the order-2 operator handle on one MI355X: structured_beam(n) elevated (n = 19:
1 028 850 tets, about 1.45 M nodes), HRZ mass, dt = 0.9 * 2/omega_max from Lanczos.  us/step and element-updates/s of
the element pass with stored geometry, the element pass that recomputes its Jacobians, the node/update pass, and the whole
step with either element pass (the stepper's "passes" and "stored_geometry" options), next to the yardstick - what the
library could do for the same step before the stepper existed: ``saa_operator_apply`` with m = 1 followed by the update as
torch elementwise operations - and ``saa_device_copy_bandwidth``.  HIP events around regions of at least ``--seconds`` each
after a warm-up of every case; the two whole-step variants and the yardstick are timed twice, alternating.  Writes one
text file (default profiles/p2_step_kernel_stats.txt).

    python tools/p2_step_point.py [--n 19] [--seconds 1.0] [--out FILE]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, seconds, chunk=50):
    """(us per step, steps) of ``fn(chunk)`` = ``chunk`` steps, from HIP events around a region of at least ``seconds``."""
    import torch

    fn(chunk)
    torch.cuda.synchronize()
    reps = 2
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(chunk)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * seconds:
            return 1e3 * ms / (reps * chunk), reps * chunk
        reps = max(2 * reps, int(reps * 1.2e3 * seconds / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2_step_kernel_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import OperatorStepper, reference_rule_dt
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.load()
    bw = C.c_double()
    _lib.check(lib.saa_device_copy_bandwidth(0, 1 << 30, 10, C.byref(bw)))
    bw = bw.value
    mesh = to_quadratic(structured_beam(args.n))
    ne, nn = len(mesh.tets10), len(mesh.points)
    E, nu, rho, fz, alpha = 1e6, 0.3, 1.0, 0.5, 0.5
    lmd, mu = fs.lame(E, nu)
    op = ModalOperator(mesh.points, mesh.tets10, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, rho, 0)
    mass, load = op.lumped_mass(), op.load((0.0, -fz, -fz))
    t = time.perf_counter()
    ts = stable_time_step_operator(op, mass, 0.9)
    torch.cuda.synchronize()
    t_dt = time.perf_counter() - t
    rule = reference_rule_dt(mesh.points, mesh.tets10, E, nu, rho, 0.9)
    say(f"Explicit step on the order-2 operator handle, one {torch.cuda.get_device_name(0)}: structured_beam({args.n}) elevated = "
        f"{ne} tets, {nn} nodes, {3 * nn} dofs.")
    say(f"HRZ mass; omega_max = {ts['omega_max']:.6f} (Lanczos, {t_dt:.1f} s), dt_crit = {ts['dt_crit']:.6e}, dt = 0.9 dt_crit = "
        f"{ts['dt']:.6e}; the reference's edge-length rule gives {rule:.6e} = {rule / ts['dt_crit']:.2f} x dt_crit.")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a pass has to move (each array once; ne elements, nn nodes):")
    say("  element pass, recomputing: 40 ne (cells) + 48 nn (coordinates, mask) + 24 nn (d0) + 240 ne (contributions)")
    say("  element pass, stored:      40 ne (cells) + 324 ne (geometry, bits) + 24 nn (d0) + 240 ne (contributions)")
    say("  node/update pass:          40 ne (pairs) + 8 nn (offsets) + 240 ne (contributions) + 144 nn (mask, mass, f, d0, dn in, dn out)")
    b_re = 40 * ne + 48 * nn + 24 * nn + 240 * ne
    b_st = 40 * ne + 324 * ne + 24 * nn + 240 * ne
    b_nd = 40 * ne + 8 * nn + 240 * ne + 144 * nn
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first.")
    say()
    say(f"{'case':44s} {'us/step':>9s} {'steps':>7s} {'Melem-upd/s':>12s} {'GB moved':>9s} {'TB/s':>6s} {'of copy bw':>10s}")

    def row(name, us, steps, nbytes=None):
        tail = f" {nbytes / 1e9:9.3f} {nbytes / (1e-6 * us) / 1e12:6.3f} {nbytes / (1e-6 * us) / bw:10.2f}" if nbytes else ""
        say(f"{name:44s} {us:9.1f} {steps:7d} {ne / us:12.1f}{tail}")

    st = OperatorStepper(op, mass, load, ts["dt"], alpha, ramp=True)

    def stepper_case(stored, passes):
        st.set_option("stored_geometry", stored)
        st.set_option("passes", passes)
        st.set_state(None, None, 0.0)
        return timed(st.step, args.seconds)

    row("element pass, stored geometry", *stepper_case(1, 1), b_st)
    row("element pass, recomputing", *stepper_case(0, 1), b_re)
    row("node/update pass", *stepper_case(0, 2), b_nd)

    # the yardstick: the block apply with one column, then the update as torch elementwise operations
    free = op.free
    dt = ts["dt"]
    den = mass + alpha * mass * dt / 2.0
    state = {"d0": torch.zeros_like(mass), "dn": torch.zeros_like(mass), "tn": 0.0}
    kx = torch.empty_like(mass)

    def composed(n):
        for _ in range(n):
            d0, dn = state["d0"], state["dn"]
            op.apply_raw(1, d0, op.n_dof, kx, None)
            d1 = (dt * dt * (load * min(state["tn"], 1.0) - kx) + 2.0 * mass * d0 - mass * dn + dt / 2.0 * mass * alpha * dn) / den
            d1 *= free
            state["dn"], state["d0"] = d0, d1
            state["tn"] += dt

    whole = {}
    for rnd in (1, 2):
        for name, fn in (("whole step, stored geometry", lambda: stepper_case(1, 3)),
                         ("whole step, recomputing", lambda: stepper_case(0, 3)),
                         ("saa_operator_apply m=1 + torch update", lambda: timed(composed, args.seconds))):
            us, steps = fn()
            whole.setdefault(name, []).append(us)
            row(f"{name} (round {rnd})", us, steps, {"whole step, stored geometry": b_st + b_nd,
                                                      "whole step, recomputing": b_re + b_nd}.get(name))
    d0, _, tn = st.state()
    say()
    say(f"state after the last stepper run: tn = {tn:.6f}, max|d| = {float(d0.abs().max()):.6e} (finite: {bool(torch.isfinite(d0).all())})")
    s_us, r_us, y_us = (min(whole[k]) for k in ("whole step, stored geometry", "whole step, recomputing",
                                                  "saa_operator_apply m=1 + torch update"))
    best, other, b_us, o_us = ("stored geometry", "recomputing", s_us, r_us) if s_us < r_us else ("recomputing", "stored geometry", r_us, s_us)
    say(f"Faster element pass in the whole step: {best} ({b_us:.1f} us/step against {o_us:.1f} for {other}: {o_us / b_us:.3f} x).")
    say(f"Fused step ({best}) against the composition: {y_us:.1f} / {b_us:.1f} = {y_us / b_us:.2f} x.")
    st.close()
    op.close()
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
