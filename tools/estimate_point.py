"""Kernel timings of the stress error estimate (HIP-event wall times; run it under rocprofv3 --kernel-trace --stats for the
per-kernel durations).  structured_beam(19) (1 028 850 tets): saa_operator_stress_error with every output, against nodal
values (the Zienkiewicz-Zhu form: 24 gathered values per element and column) and against a second element field, at
m = 1 and 16, and the whole estimate (element stress -> nodal average -> error) at m = 16.  Bytes moved are computed
from the shapes (each value read or written once: the compulsory traffic) and compared with saa_device_copy_bandwidth
(read + write bytes per second) measured in the same run."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from synchronization_avoiding_algorithms_amd import _lib
from synchronization_avoiding_algorithms_amd import fem_setup as fs
from synchronization_avoiding_algorithms_amd.mesh import structured_beam
from synchronization_avoiding_algorithms_amd.stress import StressRecovery

REPS = 10
lmd, mu = fs.lame(1e6, 0.3)
dev = torch.device("cuda", 0)
lib = _lib.load()
bw = C.c_double()
_lib.check(lib.saa_device_copy_bandwidth(0, 1 << 30, 20, C.byref(bw)))
print(f"saa_device_copy_bandwidth: {bw.value / 1e12:.3f} TB/s (read + write)", flush=True)


def timed(fn):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e-3


def report(case, sec, nbytes):
    rate = nbytes / sec
    print(f"  {case:34s} {sec * 1e6:9.1f} us  {nbytes / 1e9:7.3f} GB  {rate / 1e12:6.3f} TB/s  {rate / bw.value:5.2f} of copy",
          flush=True)


m = structured_beam(19)
nn, ne = len(m.points), len(m.tets)
rec = StressRecovery(m.points, m.tets, lmd, mu, device=0)
print(f"structured_beam(19): {ne} tets, {nn} nodes", flush=True)
for mc in (1, 16):
    S = torch.rand((mc, ne, 6), dtype=torch.float64, device=dev) - 0.5
    O = torch.rand((mc, ne, 6), dtype=torch.float64, device=dev) - 0.5
    N = torch.rand((mc, nn, 6), dtype=torch.float64, device=dev) - 0.5
    Et = torch.empty((mc, ne), dtype=torch.float64, device=dev)
    T, M = torch.empty(mc, dtype=torch.float64, device=dev), torch.empty(mc, dtype=torch.float64, device=dev)
    A = torch.empty(mc, dtype=torch.int32, device=dev)
    sec = timed(lambda: rec.error_raw(mc, S, 6 * ne, N, 6 * nn, None, 0, Et, ne, T, M, A))
    report(f"error vs nodal values, m={mc}", sec, 24 * ne + (48 * ne + 48 * nn + 8 * ne) * mc)  # tets + |V_e|; per column
    sec = timed(lambda: rec.error_raw(mc, S, 6 * ne, None, 0, O, 6 * ne, Et, ne, T, M, A))
    report(f"error vs element field, m={mc}", sec, 8 * ne + (96 * ne + 8 * ne) * mc)
    if mc == 16:
        sec = timed(lambda: rec.error_raw(mc, S, 6 * ne, N, 6 * nn, None, 0, None, 0, T, M, A))
        report(f"error vs nodal values, totals only, m={mc}", sec, 24 * ne + (48 * ne + 48 * nn) * mc)
        X = torch.rand((mc, 3 * nn), dtype=torch.float64, device=dev) - 0.5
        sec = timed(lambda: rec.estimate(X))
        print(f"  estimate(X) = element -> nodal -> error, m={mc}: {sec * 1e6:9.1f} us", flush=True)
        del X
    del S, O, N, Et
rec.close()
