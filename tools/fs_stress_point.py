#!/usr/bin/env python3
"""Timings of the finite-strain stress recovery on one MI355X: structured_beam(n) (n = 19: 1 028 850 tets), as it is for
order 1 and elevated for order 2, the element pass of csrc/saa_stress_fs.hip (saa_operator_stress_finite) for each material
and measure at m = 1, 8 and 16 columns with every output, and in the same run the linear stress entry of that order
(saa_operator_stress, saa_operator_stress_p2) and ``saa_device_copy_bandwidth``.  There is no bar to meet; the expectation to
check is that the pass is bound by the same bytes as the linear one.  Next to each time: the bytes the pass has to move,
counted from the shapes with each array read or written once, the rate they give and its share of the copy rate.  HIP events
around regions of at least ``--seconds`` each after a warm-up of every case; every case is timed twice, the rounds
alternating over the cases.  Writes one text file (default profiles/fs_stress_kernel_stats.txt).

    python tools/fs_stress_point.py [--n 19] [--seconds 0.3] [--orders 1,2] [--out FILE]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, seconds):
    """(us per call, calls) of ``fn()`` from HIP events around a region of at least ``seconds``."""
    import torch

    fn()
    fn()
    torch.cuda.synchronize()
    reps = 4
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * seconds:
            return 1e3 * ms / reps, reps
        reps = max(2 * reps, int(reps * 1.2e3 * seconds / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--orders", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fs_stress_kernel_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery, StressRecovery

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.load()
    bw = C.c_double()
    _lib.check(lib.saa_device_copy_bandwidth(0, 1 << 30, 10, C.byref(bw)))
    bw = bw.value
    lmd, mu = fs.lame(1e6, 0.3)
    say(f"Finite-strain stress recovery, one {torch.cuda.get_device_name(0)} (tools/fs_stress_point.py): structured_beam({args.n}), "
        "the element pass of saa_operator_stress_finite with every output against the linear entry of the same order.")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a pass has to move (each array once; ne elements, nn nodes, m columns), every output written:")
    say("  order 1, finite: 16 ne (cells) + 24 nn (coordinates) + m (24 nn (x) + 48 ne (stress) + 8 ne (von Mises) + 8 ne (det F) + 8 ne (W_e))")
    say("  order 1, linear: the same without det F")
    say("  order 2, finite: 40 ne (cells) + 320 ne (geometry table) + m (24 nn (x) + 192 ne (stress) + 32 ne (von Mises) + 32 ne (det F) + 8 ne (W_e))")
    say("                   (the table is read again for every column, 320 ne m from the caches; it is counted once)")
    say("  order 2, linear: 40 ne (cells) + 24 nn (coordinates) + m (24 nn (x) + 192 ne (sigma) + 32 ne (von Mises) + 8 ne (W_e))")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, two rounds.")
    say("The time of a call includes the final reduction kernel (one workgroup per column); no inversion count is asked for.")

    for order in (int(o) for o in args.orders.split(",")):
        mesh = structured_beam(args.n)
        if order == 2:
            mesh = to_quadratic(mesh)
            rec = QuadraticStressRecovery(mesh.points, mesh.tets10, lmd, mu)
        else:
            rec = StressRecovery(mesh.points, mesh.tets, lmd, mu)
        ne, nn, nq = rec.n_elems, rec.n_nodes, 4 if order == 2 else 1
        dev = rec.torch_device
        say()
        say(f"order {order}: {ne} tets, {nn} nodes, {3 * nn} dofs")
        say(f"{'case':40s} {'us/call':>10s} {'calls':>6s} {'GB moved':>9s} {'TB/s':>6s} {'of copy bw':>10s} {'of linear':>9s}")
        g = torch.Generator(device=dev).manual_seed(3)
        for m in (1, 8, 16):
            X = (torch.rand((m, 3 * nn), dtype=torch.float64, device=dev, generator=g) - 0.5) * 1e-3
            S = torch.empty((m, 6 * nq * ne), dtype=torch.float64, device=dev)
            V, D = (torch.empty((m, nq * ne), dtype=torch.float64, device=dev) for _ in range(2))
            W = torch.empty((m, ne), dtype=torch.float64, device=dev)
            T, M = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
            A = torch.empty(m, dtype=torch.int32, device=dev)
            per_col = 24 * nn + (6 * nq + 2 * nq + 1) * 8 * ne
            if order == 2:
                fixed_fs, fixed_lin = 360 * ne, 40 * ne + 24 * nn
                linear = lambda: rec.stress_raw(m, X, 3 * nn, S, 24 * ne, V, 4 * ne, W, ne, T, M, A)  # noqa: E731
            else:
                fixed_fs = fixed_lin = 16 * ne + 24 * nn
                linear = lambda: rec.stress_raw(m, X, 3 * nn, S, 6 * ne, V, W, ne, T, M, A)  # noqa: E731
            cases = [(f"linear, m={m}", fixed_lin + m * (per_col - 8 * nq * ne), linear)]
            for material, mat in (("svk", 1), ("neo_hookean", 2)):
                for measure, meas in (("pk2", 0), ("cauchy", 1)):
                    cases.append((f"{material} {measure}, m={m}", fixed_fs + m * per_col,
                                  lambda mat=mat, meas=meas: rec.stress_finite_raw(mat, meas, m, X, 3 * nn, S, 6 * nq * ne, V, nq * ne,
                                                                                   D, nq * ne, W, ne, T, M, A)))
            base = {}
            for rnd in (1, 2):
                for name, nbytes, fn in cases:
                    us, calls = timed(fn, args.seconds)
                    if name.startswith("linear"):
                        base[rnd] = us
                    rate = nbytes / (1e-6 * us)
                    say(f"{name + f' (round {rnd})':40s} {us:10.1f} {calls:6d} {nbytes / 1e9:9.3f} {rate / 1e12:6.3f} {rate / bw:10.2f} "
                        f"{us / base[rnd]:9.2f}")
            torch.cuda.synchronize()
            say(f"  m={m}: energy_total[0] = {float(T[0]):.6e}, outputs finite: {bool(torch.isfinite(S).all() and torch.isfinite(T).all())}")
            del X, S, V, D, W
        rec.close()
        del rec
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_stress_fs.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_stress_fs.hip"],
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
