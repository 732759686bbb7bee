#!/usr/bin/env python3
"""What the block tangent apply costs on one MI355X: us per call of ``saa_operator_tangent_apply_block`` with ``m`` = 1, 8, 16
columns, ``svk`` and ``neo_hookean``, on structured_beam(n) (n = 19: 1 028 850 tets) as it is at order 1 and elevated to order
2 - next to it, in the same run, (a) ``m`` calls of the one-column ``saa_operator_tangent_apply`` and (b) the linear
``saa_operator_apply`` with the same ``m`` (its K output only).  The cases are timed alternately, ``--rounds`` times each, with
HIP events around regions of at least ``--seconds`` that end in a synchronise, after a warm-up of every case; every round is
printed, so that the spread is known, and the smaller is compared.  Writes one text file (default
profiles/tangent_block_stats.txt).

    python tools/tangent_block_point.py [--n 19] [--seconds 1.0] [--rounds 2] [--orders 2,1] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from p2_step_point import timed  # noqa: E402

COLUMNS = (1, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--orders", default="2,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_block_stats.txt"))
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
    lmd, mu = fs.lame(1e6, 0.3)
    say(f"Block tangent apply on the operator handle, one {torch.cuda.get_device_name(0)}: us per call of m columns (element pass + "
        f"node sum).")
    say(f"Times: HIP events around a region of >= {args.seconds:.2f} s per figure that ends in a synchronise, every case warmed up "
        f"first, the cases alternating, {args.rounds} round(s); the ratios compare the smallest of each.  State u: a smooth field at "
        f"max|H| about 1e-2; columns v: noise.")
    say("block: one saa_operator_tangent_apply_block call; singles: m saa_operator_tangent_apply calls; linear: one "
        "saa_operator_apply call (K only).")
    best, spread = {}, {}
    base = structured_beam(args.n)
    for order in (int(o) for o in args.orders.split(",")):
        mesh = to_quadratic(base) if order == 2 else base
        cells = mesh.tets10 if order == 2 else mesh.tets
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {len(cells)} tets, {len(mesh.points)} nodes")
        say(f"{'case':52s} {'us/call':>10s} {'us/column':>10s} {'calls':>7s}")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0) as op:
            x = np.asarray(mesh.points, dtype=np.float64)
            u = np.zeros_like(x)
            u[:, 1] = 2e-4 * x[:, 0] ** 2
            u[:, 2] = 1e-2 * np.sin(0.5 * x[:, 0])
            u = torch.as_tensor(u.reshape(-1), device=op.torch_device)
            g = torch.Generator(device="cpu").manual_seed(0)
            V = (torch.rand((16, op.n_dof), generator=g, dtype=torch.float64) - 0.5).to(op.torch_device)
            Y = torch.empty_like(V)
            pu, pv, py = (C.c_void_p(t.data_ptr()) for t in (u, V, Y))
            cols = [(C.c_void_p(V[j].data_ptr()), C.c_void_p(Y[j].data_ptr())) for j in range(16)]

            def block(mat, m):
                def run(n):
                    for _ in range(n):
                        _lib.check(lib.saa_operator_tangent_apply_block(op._h, mat, pu, m, pv, op.n_dof, py, op.n_dof, None))
                return run

            def singles(mat, m):
                def run(n):
                    for _ in range(n):
                        for a, b in cols[:m]:
                            _lib.check(lib.saa_operator_tangent_apply(op._h, mat, pu, a, b, None))
                return run

            def linear(m):
                def run(n):
                    for _ in range(n):
                        _lib.check(lib.saa_operator_apply(op._h, m, pv, op.n_dof, py, None, op.n_dof))
                return run

            cases = []
            for m in COLUMNS:
                cases.append((f"linear apply, m = {m}", linear(m), m))
                for name, mat in (("svk", 1), ("neo_hookean", 2)):
                    cases += [(f"{name} block, m = {m}", block(mat, m), m), (f"{name} singles, m = {m}", singles(mat, m), m)]
            for _, fn, _ in cases:
                fn(2)
            torch.cuda.synchronize()
            for rnd in range(1, args.rounds + 1):
                for name, fn, m in cases:
                    us, calls = timed(fn, args.seconds, chunk=4)
                    key = (order, name)
                    best[key] = min(best.get(key, us), us)
                    spread[key] = max(spread.get(key, us), us)
                    say(f"{f'order {order}, {name} (round {rnd})':52s} {us:10.1f} {us / m:10.1f} {calls:7d}")
            # the two routes agree (different kernels: to round-off)
            for name, mat in (("svk", 1), ("neo_hookean", 2)):
                n_inv = C.c_int64(0)
                _lib.check(lib.saa_operator_tangent_apply_block(op._h, mat, pu, 16, pv, op.n_dof, py, op.n_dof, C.byref(n_inv)))
                one = torch.empty(op.n_dof, dtype=torch.float64, device=op.torch_device)
                _lib.check(lib.saa_operator_tangent_apply(op._h, mat, pu, cols[15][0], C.c_void_p(one.data_ptr()), None))
                torch.cuda.synchronize()
                say(f"  {name}: max|K_T v| = {float(Y.abs().max()):.6e} (finite: {bool(torch.isfinite(Y).all())}), inverted {n_inv.value}, "
                    f"column 15 against the one-column entry {float((Y[15] - one).abs().max() / one.abs().max()):.2e}")
    say()
    say(f"{'case':40s} {'block us':>10s} {'singles us':>11s} {'block/singles':>14s} {'block/linear':>13s} {'spread of the rounds':>21s}")
    for (order, name), us in best.items():
        if " block" not in name:
            continue
        m = int(name.rsplit("=", 1)[1])
        s_us = best[(order, name.replace("block", "singles"))]
        l_us = best[(order, f"linear apply, m = {m}")]
        sp = max(spread[k] / best[k] - 1.0 for k in ((order, name), (order, name.replace("block", "singles"))))
        say(f"{f'order {order}, {name}':40s} {us:10.1f} {s_us:11.1f} {us / s_us:14.3f} {us / l_us:13.3f} {100 * sp:20.1f}%")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
