#!/usr/bin/env python3
"""Timings of the quadratic-tetrahedron (order 2) operator on one MI355X: K apply, M apply and load on structured_beam(n)
elevated (n = 19: 1 028 850 tets, about 1.45 M nodes) for m = 1, 8, 16 columns, HIP events around regions of at least
``--seconds`` each after a warm-up of every shape; the bytes each pass has to move and their share of
``saa_device_copy_bandwidth``; the register counts of the kernels; the wall time of ``drivers steady_state --order 2`` and
``drivers modal --order 2`` (child processes, each under its own time limit) with their iteration counts.  Writes one text
file (default profiles/p2_kernel_stats.txt).

    python tools/p2_point.py [--n 19] [--steady-n 19] [--modal-n 19] [--seconds 0.5] [--out FILE] [--no-drivers]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, seconds):
    """ms per call of ``fn`` from HIP events around a region of at least ``seconds`` (sized from a first short region)."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 5
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * seconds:
            return ms / reps, reps
        reps = max(2 * reps, int(reps * 1.2e3 * seconds / max(ms, 1e-3)))


def driver(args, limit):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    t = time.perf_counter()
    try:
        out = subprocess.run([sys.executable, "-m", "synchronization_avoiding_algorithms_amd.drivers", *args], cwd=ROOT,
                             capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        return None, time.perf_counter() - t, f"not finished within {limit} s"
    return out, time.perf_counter() - t, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--steady-n", type=int, default=19)
    ap.add_argument("--modal-n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--driver-limit", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2_kernel_stats.txt"))
    ap.add_argument("--scratch", default=os.path.join(ROOT, "p2_point_out"), help="where the drivers write their results")
    ap.add_argument("--no-drivers", action="store_true")
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.load()
    bw = C.c_double()
    _lib.check(lib.saa_device_copy_bandwidth(0, 1 << 30, 10, C.byref(bw)))
    bw = bw.value
    t = time.perf_counter()
    mesh = to_quadratic(structured_beam(args.n))
    t_elev = time.perf_counter() - t
    ne, nn = len(mesh.tets10), len(mesh.points)
    lmd, mu = fs.lame(1e6, 0.3)
    say(f"Order-2 operator on one {torch.cuda.get_device_name(0)}: structured_beam({args.n}) elevated = {ne} tets, {nn} nodes, "
        f"{3 * nn} dofs (to_quadratic on the host: {t_elev:.1f} s).")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a pass has to move (each array once; m columns):")
    say("  element pass K or M: 40 ne (cells) + 48 nn (coordinates, mask) + m (24 nn (x) + 240 ne (contributions))")
    say("  node pass:           40 ne (pairs) + 32 nn (offsets, mask) + m (240 ne (contributions) + 24 nn (y))")
    say("  load:                element pass with m = 1 without x and mask, then the node pass")
    say("Times: HIP events around a region of >= %.2f s per figure, every shape warmed up first." % args.seconds)
    say()
    t = time.perf_counter()
    op = ModalOperator(mesh.points, mesh.tets10, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0)
    torch.cuda.synchronize()
    say(f"operator create (CSR on the host + copies): {time.perf_counter() - t:.2f} s")
    say(f"{'case':24s} {'ms':>9s} {'reps':>6s} {'GB moved':>9s} {'TB/s':>7s} {'of copy bw':>10s}")
    for m in (1, 8, 16):
        X = torch.rand((m, op.n_dof), dtype=torch.float64, device="cuda")
        KX, MX = torch.empty_like(X), torch.empty_like(X)
        elem = 40 * ne + 48 * nn + m * (24 * nn + 240 * ne)
        node = 40 * ne + 32 * nn + m * (240 * ne + 24 * nn)
        for name, fn, nbytes in ((f"K apply m={m}", lambda: op.apply_raw(m, X, op.n_dof, KX, None), elem + node),
                                 (f"M apply m={m}", lambda: op.apply_raw(m, X, op.n_dof, None, MX), elem + node),
                                 (f"K+M apply m={m}", lambda: op.apply_raw(m, X, op.n_dof, KX, MX), 2 * (elem + node))):
            ms, reps = timed(fn, args.seconds)
            rate = nbytes / (1e-3 * ms)
            say(f"{name:24s} {ms:9.3f} {reps:6d} {nbytes / 1e9:9.3f} {rate / 1e12:7.3f} {rate / bw:10.2f}")
    nbytes = (40 * ne + 24 * nn + 240 * ne) + (40 * ne + 32 * nn + 240 * ne + 24 * nn)
    ms, reps = timed(lambda: op.load((0.0, -0.5, -0.5)), args.seconds)
    say(f"{'load':24s} {ms:9.3f} {reps:6d} {nbytes / 1e9:9.3f} {nbytes / (1e-3 * ms) / 1e12:7.3f} {nbytes / (1e-3 * ms) / bw:10.2f}")
    ms, reps = timed(lambda: op.diagonal(), args.seconds)
    say(f"{'diagonal (K and M)':24s} {ms:9.3f} {reps:6d}")
    op.close()
    say()
    say("For context, the linear apply on structured_beam(19) (1 028 850 tets, 190 400 nodes), profiles/modal_kernel_stats.txt:")
    say("  K only 0.151 / 1.159 / 2.377 ms for m = 1 / 8 / 16.")
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_p2.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_p2.hip"],
                             capture_output=True, text=True)
        for ln in res.stdout.splitlines():
            say("  " + ln)
    else:
        say("  hipcc not installed here: not measured")
    if not args.no_drivers:
        say()
        say("Drivers (child processes, wall time of the whole command: import, mesh, elevation, operator, solve, output):")
        out, wall, why = driver(["steady_state", "--order", "2", "--synthetic", str(args.steady_n), "--out", args.scratch],
                                args.driver_limit)
        if why or out.returncode != 0:
            say(f"  steady_state --order 2 --synthetic {args.steady_n}: {why or f'failed with return code {out.returncode}: ' + out.stderr[-400:]}")
        else:
            m = re.search(r"steady solve \(order 2\): .*", out.stdout)
            say(f"  steady_state --order 2 --synthetic {args.steady_n}: {wall:.1f} s; {m.group(0) if m else out.stdout[-300:]}")
        if why is not None or out.returncode != 0:
            # after a time limit, a fault or any other failure of a GPU child nothing more is started on the device
            say(f"  modal --order 2 --synthetic {args.modal_n} --k 6: not started, because the steady_state child did not end cleanly")
        else:
            out, wall, why = driver(["modal", "--order", "2", "--synthetic", str(args.modal_n), "--k", "6"], args.driver_limit)
            if why or out.returncode != 0:
                say(f"  modal --order 2 --synthetic {args.modal_n} --k 6: {why or 'failed: ' + out.stderr[-400:]}")
            else:
                r = json.loads(out.stdout.strip().splitlines()[-1])
                say(f"  modal --order 2 --synthetic {args.modal_n} --k 6: {wall:.1f} s; {r['n_elems']} tets, {r['n_nodes']} nodes, "
                    f"outer {r['outer_iterations']}, inner {r['inner_iterations']}, converged {r['modes_converged']}, "
                    f"lowest_modes {r['seconds']['lowest_modes']:.1f} s")
                say(f"    frequencies_hz {r['frequencies_hz']}")
                say(f"    residuals {r['residuals']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
