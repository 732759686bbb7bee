#!/usr/bin/env python3
"""What the finite-strain tangent apply costs on one MI355X: us per call of ``saa_operator_tangent_apply`` (element pass and node
sum, one column) with ``svk`` and ``neo_hookean`` on structured_beam(n) (n = 19: 1 028 850 tets), as it is at order 1 and
elevated to order 2 - next to it, in the same run, the force pass of the same material (``saa_operator_internal_force``) and
the linear apply at ``m = 1`` (``saa_operator_apply``).  The cases are timed alternately, twice each, with HIP events around
regions of at least ``--seconds`` after a warm-up of every case; both rounds are printed and the smaller is compared.  The
bytes a call has to move, by count, stand next to the times: the tangent pass moves the force pass's bytes plus one more
gathered column, and is expected to cost about that ratio.  Writes one text file (default profiles/tangent_kernel_stats.txt).

    python tools/tangent_point.py [--n 19] [--seconds 1.0] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_kernel_stats.txt"))
    args = ap.parse_args()

    import numpy as np
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
    lmd, mu = fs.lame(1e6, 0.3)
    say(f"Finite-strain tangent apply on the operator handle, one {torch.cuda.get_device_name(0)}: us per call (element pass + node "
        f"sum, one column).")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure, every case warmed up first, the cases alternating, "
        f"two rounds; the ratios compare the smaller of each.  State u: a smooth field at max|H| about 1e-2; direction v: noise.")
    say(f"saa_device_copy_bandwidth (1 GiB, read + write): {bw / 1e12:.3f} TB/s.")
    say("Bytes a call has to move, by count (each array once; ne elements, nn nodes, npe nodes per element):")
    say("  node sum, every case:                  4 npe ne (pairs) + 8 nn (offsets) + 24 npe ne (contributions) + 48 nn (mask, y)")
    say("  order 2 force pass (stored table):     40 ne (cells) + 324 ne (geometry, bits) + 24 nn (u) + 240 ne (contributions)")
    say("  order 2 tangent pass:                  the force pass + 24 nn (v); neo_hookean reads u four times per element, from L1/L2")
    say("  order 2 linear apply (recomputing):    40 ne (cells) + 48 nn (coordinates, mask) + 24 nn (x) + 240 ne (contributions)")
    say("  order 1 force pass and linear apply:   16 ne (cells) + 48 nn (coordinates, mask) + 24 nn (u) + 96 ne (contributions)")
    say("  order 1 tangent pass:                  the force pass + 24 nn (v)")
    say("  (a stored per-point tangent table at order 2 would be >= 60 doubles = 480 B per element and apply, against the 240 B of")
    say("   the thirty gathered - and cached - displacements it replaces: H(u) is recomputed)")
    best = {}
    base = structured_beam(args.n)
    for order in (2, 1):
        mesh = to_quadratic(base) if order == 2 else base
        cells = mesh.tets10 if order == 2 else mesh.tets
        ne, nn, npe = len(cells), len(mesh.points), 10 if order == 2 else 4
        b_node = 28 * npe * ne + 56 * nn
        b_force = (40 * ne + 324 * ne + 24 * nn + 240 * ne) if order == 2 else (16 * ne + 72 * nn + 96 * ne)
        b_linear = (40 * ne + 72 * nn + 240 * ne) if order == 2 else b_force
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {ne} tets, {nn} nodes")
        say(f"{'case':44s} {'us/call':>9s} {'calls':>7s} {'GB moved':>9s} {'TB/s':>6s} {'of copy bw':>10s}")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0) as op:
            x = np.asarray(mesh.points, dtype=np.float64)
            u = np.zeros_like(x)
            u[:, 1] = 2e-4 * x[:, 0] ** 2
            u[:, 2] = 1e-2 * np.sin(0.5 * x[:, 0])
            u = torch.as_tensor(u.reshape(-1), device=op.torch_device)
            g = torch.Generator(device="cpu").manual_seed(0)
            v = (torch.rand(op.n_dof, generator=g, dtype=torch.float64) - 0.5).to(op.torch_device)
            y = torch.empty_like(v)
            pu, pv, py = (C.c_void_p(t.data_ptr()) for t in (u, v, y))

            def tangent(mat):
                def run(n):
                    for _ in range(n):
                        _lib.check(lib.saa_operator_tangent_apply(op._h, mat, pu, pv, py, None))
                return run

            def force(mat):
                def run(n):
                    for _ in range(n):
                        _lib.check(lib.saa_operator_internal_force(op._h, mat, pu, py, None, None))
                return run

            def linear(n):
                for _ in range(n):
                    _lib.check(lib.saa_operator_apply(op._h, 1, pv, op.n_dof, py, None, op.n_dof))

            cases = [("linear apply, m = 1", linear, b_linear + b_node)]
            for name, mat in (("svk", 1), ("neo_hookean", 2)):
                cases += [(f"{name} force", force(mat), b_force + b_node), (f"{name} tangent", tangent(mat), b_force + 24 * nn + b_node)]
            for _, fn, _ in cases:
                fn(10)
            torch.cuda.synchronize()
            for rnd in (1, 2):
                for name, fn, b in cases:
                    us, calls = timed(fn, args.seconds)
                    best[(order, name)] = (min(best.get((order, name), (us, b))[0], us), b)
                    say(f"{f'order {order}, {name} (round {rnd})':44s} {us:9.1f} {calls:7d} {b / 1e9:9.3f} {b / (1e-6 * us) / 1e12:6.3f} "
                        f"{b / (1e-6 * us) / bw:10.2f}")
            n_inv = C.c_int64(0)
            _lib.check(lib.saa_operator_tangent_apply(op._h, 2, pu, pv, py, C.byref(n_inv)))
            say(f"  max|K_T v| = {float(y.abs().max()):.6e} (finite: {bool(torch.isfinite(y).all())}), inverted {n_inv.value}")
    say()
    say(f"{'case':36s} {'us/call':>9s} {'/ force':>9s} {'bytes / force':>14s} {'/ linear apply':>15s}")
    for (order, name), (us, b) in best.items():
        if not name.endswith("tangent"):
            continue
        f_us, f_b = best[(order, name.replace("tangent", "force"))]
        say(f"{f'order {order}, {name}':36s} {us:9.1f} {us / f_us:9.3f} {b / f_b:14.3f} {us / best[(order, 'linear apply, m = 1')][0]:15.3f}")
    say()
    say("Registers (hipcc -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.py --file=saa_optan.hip):")
    if os.path.exists("/opt/rocm/bin/hipcc"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--file=saa_optan.hip"],
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
