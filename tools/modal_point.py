"""Kernel timings of the modal kernels (run it under rocprofv3 --kernel-trace --stats): element bound on the 8.2M-tet beam, block apply m = 1/8/16 on 1M tets."""
import sys
import time

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import numpy as np
import torch

from synchronization_avoiding_algorithms_amd import fem_setup as fs
from synchronization_avoiding_algorithms_amd.mesh import clamp_nodes, structured_beam
from synchronization_avoiding_algorithms_amd.modal import ModalOperator

lmd, mu = fs.lame(1e6, 0.3)
dev = torch.device("cuda", 0)
for n in (38, 19):
    m = structured_beam(n)
    op = ModalOperator(m.points, m.tets, fs.node_to_dof(clamp_nodes(m)), lmd, mu, 1.0, 0)
    print(f"structured_beam({n}): {len(m.tets)} tets, {len(m.points)} nodes", flush=True)
    for _ in range(5):
        t = time.perf_counter()
        b = op.element_bound()
        print(f"  element_bound host wall {1e3 * (time.perf_counter() - t):.3f} ms omega_max {b['omega_max']:.6e}", flush=True)
    if n == 19:
        for mc in (1, 8, 16):
            X = torch.rand((mc, op.n_dof), dtype=torch.float64, device=dev)
            KX, MX = torch.empty_like(X), torch.empty_like(X)
            for _ in range(2):
                op.apply_raw(mc, X, op.n_dof, KX, None)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                op.apply_raw(mc, X, op.n_dof, KX, None)
            e1.record()
            torch.cuda.synchronize()
            kms = e0.elapsed_time(e1) / 10
            e0.record()
            for _ in range(10):
                op.apply_raw(mc, X, op.n_dof, KX, MX)
            e1.record()
            torch.cuda.synchronize()
            print(f"  apply m={mc}: K only {kms:.3f} ms, K+M {e0.elapsed_time(e1) / 10:.3f} ms", flush=True)
    op.close()
    del m
