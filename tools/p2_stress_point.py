#!/usr/bin/env python3
"""Timings of the stress recovery and error estimate of quadratic tetrahedra on one MI355X: structured_beam(n) elevated
(n = 19: 1 028 850 tets, about 1.45 M nodes), the three passes of csrc/saa_stress_p2.hip at m = 1, 8 and 16 columns with
every output: the element pass (saa_operator_stress_p2), the nodal pass (saa_operator_nodal_stress_p2) and the error pass
in both forms (saa_operator_stress_error_p2).  Next to each time: the bytes the pass has to move, counted from the shapes
with each array read or written once, the rate they give, and its share of ``saa_device_copy_bandwidth`` measured in the
same run - to be read against the shares of the linear passes on the same beam (profiles/stress_kernel_stats.txt,
profiles/estimate_kernel_stats.txt: 0.46 element, 0.07 nodal, 0.53 error).  HIP events around regions of at least
``--seconds`` each after a warm-up of every case; every case is timed twice, the rounds alternating over the cases.
Writes one text file (default profiles/p2_stress_kernel_stats.txt).

    python tools/p2_stress_point.py [--n 19] [--seconds 0.5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINEAR_SHARE = {"element": 0.46, "nodal": 0.07, "error": 0.53}


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
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2_stress_kernel_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import _lib
    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.mesh import structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.stress import QuadraticStressRecovery

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
    lmd, mu = fs.lame(1e6, 0.3)
    rec = QuadraticStressRecovery(mesh.points, mesh.tets10, lmd, mu)
    dev = rec.torch_device
    say(f"Stress recovery and error estimate of quadratic tetrahedra, one {torch.cuda.get_device_name(0)} "
        f"(tools/p2_stress_point.py): structured_beam({args.n}) elevated = {ne} tets, {nn} nodes, {3 * nn} dofs.")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a pass has to move (each array once; ne elements, nn nodes, m columns), every output written:")
    say("  element pass:        40 ne (cells) + 24 nn (coordinates) + m (24 nn (x) + 192 ne (sigma) + 32 ne (von Mises) + 8 ne (W_e))")
    say("  nodal pass:          8 nn (offsets) + 40 ne (pairs) + 8 ne (|V_e|) + 8 nn (weight sums) + m (192 ne (sigma) + 48 nn (sigma*))")
    say("  error, nodal form:   40 ne (cells) + 24 nn (coordinates) + m (192 ne (sigma) + 48 nn (sigma*) + 8 ne (eta2))")
    say("  error, element form: 40 ne (cells) + 24 nn (coordinates) + m (2 * 192 ne (two fields) + 8 ne (eta2))")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, two rounds.")
    say("The time of a call includes the final reduction kernel (one workgroup per column).")
    say()
    say(f"{'case':34s} {'us/call':>10s} {'calls':>6s} {'GB moved':>9s} {'TB/s':>6s} {'of copy bw':>10s} {'linear pass':>11s}")

    g = torch.Generator(device=dev).manual_seed(3)
    results = {}
    for m in (1, 8, 16):
        X = (torch.rand((m, 3 * nn), dtype=torch.float64, device=dev, generator=g) - 0.5) * 1e-3
        S = torch.empty((m, ne, 4, 6), dtype=torch.float64, device=dev)
        S2 = torch.empty_like(S)
        V = torch.empty((m, ne, 4), dtype=torch.float64, device=dev)
        W, H = (torch.empty((m, ne), dtype=torch.float64, device=dev) for _ in range(2))
        N = torch.empty((m, nn, 6), dtype=torch.float64, device=dev)
        T, M = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
        A = torch.empty(m, dtype=torch.int32, device=dev)
        rec.stress_raw(m, X.flip(0).contiguous(), 3 * nn, S2, 24 * ne)
        cases = (
            ("element", f"element pass, m={m}", 40 * ne + 24 * nn + m * (24 * nn + 232 * ne),
             lambda: rec.stress_raw(m, X, 3 * nn, S, 24 * ne, V, 4 * ne, W, ne, T, M, A)),
            ("nodal", f"nodal pass, m={m}", 48 * ne + 16 * nn + m * (192 * ne + 48 * nn),
             lambda: rec.nodal_raw(m, S, 24 * ne, N, 6 * nn)),
            ("error", f"error pass, nodal form, m={m}", 40 * ne + 24 * nn + m * (200 * ne + 48 * nn),
             lambda: rec.error_raw(m, S, 24 * ne, N, 6 * nn, None, 0, H, ne, T, M, A)),
            ("error", f"error pass, element form, m={m}", 40 * ne + 24 * nn + m * 392 * ne,
             lambda: rec.error_raw(m, S, 24 * ne, None, 0, S2, 24 * ne, H, ne, T, M, A)),
        )
        for rnd in (1, 2):
            for kind, name, nbytes, fn in cases:
                us, calls = timed(fn, args.seconds)
                results.setdefault(name, []).append(us)
                rate = nbytes / (1e-6 * us)
                say(f"{name + f' (round {rnd})':34s} {us:10.1f} {calls:6d} {nbytes / 1e9:9.3f} {rate / 1e12:6.3f} {rate / bw:10.2f} "
                    f"{LINEAR_SHARE[kind]:11.2f}")
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(T).all() and torch.isfinite(H).all() and torch.isfinite(N).all())
        say(f"  m={m}: eta2_total[0] = {float(T[0]):.6e}, outputs finite: {finite}")
        del X, S, S2, V, W, H, N
    rec.close()
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_stress_p2.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_stress_p2.hip"],
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
