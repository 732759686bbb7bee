#!/usr/bin/env python3
"""What the implicit stepper costs on one MI355X: structured_beam(n) (n = 19: 1 028 850 tets) as it is at order 1 and elevated
to order 2, St. Venant-Kirchhoff, lumped mass of the handle (HRZ at order 2), constant load ``(0, -fz, -fz)`` from rest, ``alpha =
0.5``.  Two measurements per order, no bar on either:

1. Time per PCG iteration.  The device loop: wall time of ``ImplicitStepper.step`` over the PCG iterations it reports, so the
   Newton overhead (force pass, residual pass, the host's look at the status block) is inside the figure.  Next to it the same
   iteration composed from what the library offered before: ``op.tangent_apply`` plus the torch vector operations of
   ``steady._tangent_pcg``, the shift added in torch, the host looking every 25 iterations - that loop alone, nothing of Newton.
2. Wall time of an implicit run at ``dt = F * 2/omega_max`` for ``F`` = 10 and 50 against the explicit stepper (``0.9 * 2/omega_max``)
   over the same physical time, ``--span`` explicit limits (default 200).

Wall times are ``time.perf_counter`` around a region that ends in a device synchronisation, after a warm-up.  Writes one text
file (default profiles/implicit_kernel_stats.txt).

    python tools/implicit_point.py [--n 19] [--span 200] [--fz 50] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=19)
    ap.add_argument("--span", type=float, default=200.0, help="physical time of the runs in units of 2/omega_max")
    ap.add_argument("--fz", type=float, default=50.0)
    ap.add_argument("--orders", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "implicit_kernel_stats.txt"))
    args = ap.parse_args()

    import torch

    from synchronization_avoiding_algorithms_amd import fem_setup as fs
    from synchronization_avoiding_algorithms_amd.dynamics import ImplicitStepper, OperatorStepper
    from synchronization_avoiding_algorithms_amd.mesh import plane_nodes, structured_beam, to_quadratic
    from synchronization_avoiding_algorithms_amd.modal import ModalOperator, stable_time_step_operator

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    lmd, mu = fs.lame(1e6, 0.3)
    alpha, material = 0.5, "svk"
    say(f"Implicit Newmark stepper on the operator handle, one {torch.cuda.get_device_name(0)}: {material}, constant load (0, -{args.fz:g}, "
        f"-{args.fz:g}) from rest, alpha = {alpha}, tol = 1e-10, check_every = 25.  Wall times (perf_counter, region ends in a device "
        "synchronisation, after a warm-up run of the same case).")
    base = structured_beam(args.n)
    for order in (int(o) for o in args.orders.split(",")):
        mesh = to_quadratic(base) if order == 2 else base
        cells = mesh.tets10 if order == 2 else mesh.tets
        say()
        say(f"order {order}: structured_beam({args.n}){' elevated' if order == 2 else ''} = {len(cells)} tets, {len(mesh.points)} nodes")
        with ModalOperator(mesh.points, cells, fs.node_to_dof(plane_nodes(mesh.points)), lmd, mu, 1.0, 0) as op:
            mass = op.lumped_mass()
            load = op.load((0.0, -args.fz, -args.fz))
            ts = stable_time_step_operator(op, mass, 0.9)
            dt_crit = ts["dt_crit"]
            say(f"  2/omega_max = {dt_crit:.6e} (Lanczos), explicit dt = {ts['dt']:.6e}, span = {args.span:g} x 2/omega_max = "
                f"{args.span * dt_crit:.6e}")

            def explicit():
                with OperatorStepper(op, mass, load, ts["dt"], alpha, ramp=False, material=material) as st:
                    n = int(round(args.span * dt_crit / ts["dt"]))
                    st.step(n)
                    d = st.state()[0]
                return n, float(d.abs().max())

            def implicit(factor):
                def run():
                    with ImplicitStepper(op, mass, load, factor * dt_crit, alpha, ramp=False, material=material) as st:
                        info = st.step(max(1, int(round(args.span / factor))))
                        d = st.state()[0]
                    return info, float(d.abs().max())
                return run

            explicit()
            t_ex, (n_ex, d_ex) = wall(explicit)
            say(f"  explicit stepper: {n_ex} steps in {1e3 * t_ex:.1f} ms ({1e6 * t_ex / n_ex:.1f} us/step), max|d| = {d_ex:.6e}")
            for factor in (10.0, 50.0):
                implicit(factor)()
                t_im, (info, d_im) = wall(implicit(factor))
                say(f"  implicit, dt-factor {factor:g}: {info['steps_done']} steps in {1e3 * t_im:.1f} ms, converged {info['converged']}, "
                    f"{info['newton_iterations']} Newton and {info['cg_iterations']} PCG iterations "
                    f"({1e6 * t_im / max(info['cg_iterations'], 1):.1f} us per PCG iteration, all of the step inside), max|d| = {d_im:.6e}; "
                    f"implicit / explicit wall time = {t_im / t_ex:.2f}")

            # the same PCG iteration composed from what the library offered before: tangent_apply + torch, the shift in torch
            with ImplicitStepper(op, mass, load, 10.0 * dt_crit, alpha, ramp=False, material=material) as st:
                st.step(2)
                u = st.state()[0]
            dt = 10.0 * dt_crit
            shift = (4.0 / (dt * dt) + 2.0 * alpha / dt) * mass * op.free
            diag_k, _ = op.diagonal(k=True, m=False)
            den = diag_k + shift
            minv = torch.where(den > 0, op.free / torch.where(den > 0, den, 1.0), op.free)
            g = torch.Generator(device="cpu").manual_seed(0)
            r0 = ((torch.rand(op.n_dof, generator=g, dtype=torch.float64) - 0.5).to(op.torch_device)) * op.free

            def composed(n_iter, check_every=25):
                x, r = torch.zeros_like(r0), r0.clone()
                z = minv * r
                p, rz = z.clone(), torch.dot(r, z)
                alive = torch.ones((), dtype=torch.float64, device=r0.device)
                for it in range(1, n_iter + 1):
                    ap_ = op.tangent_apply(u, p, material) + shift * p
                    pap = torch.dot(p, ap_)
                    alive = alive * (pap > 0)
                    a = alive * rz / torch.where(pap > 0, pap, 1.0)
                    x = x + a * p
                    r = r - a * ap_
                    z = minv * r
                    rz_new = torch.dot(r, z)
                    p = z + torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, 1.0), 0.0) * p
                    rz = rz_new
                    if it % check_every == 0:
                        float(alive), float(torch.linalg.vector_norm(r))
                return x

            def device_apply(n_iter):
                out = None
                for _ in range(n_iter):
                    out, _ = op.shifted_apply(u, r0, shift, material, dot=True)
                return out

            composed(50)
            t_co, _ = wall(lambda: composed(200))
            device_apply(50)
            t_ap, _ = wall(lambda: device_apply(200))
            say(f"  composed iteration (tangent_apply + torch vector operations, host look every 25): {1e6 * t_co / 200:.1f} us per "
                f"iteration over 200; saa_operator_shifted_apply with the dot alone (element pass, shifted node pass, the final sum): "
                f"{1e6 * t_ap / 200:.1f} us per call")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
