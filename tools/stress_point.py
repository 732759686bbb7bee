"""Kernel timings of the stress recovery (run it once plain for the HIP-event wall times, once under rocprofv3
--kernel-trace --stats for the per-kernel durations).  structured_beam(19) (1 028 850 tets) and structured_beam(38)
(8.2M tets): the element pass with every output at m = 1 and 16, the totals alone at m = 16, the nodal average of k = 6
components at m = 1 and 16.  Bytes moved are computed from the shapes (each value read or written once: the compulsory
traffic) and compared with saa_device_copy_bandwidth (read + write bytes per second) measured in the same run."""
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


for n in (19, 38):
    m = structured_beam(n)
    nn, ne = len(m.points), len(m.tets)
    rec = StressRecovery(m.points, m.tets, lmd, mu, device=0)
    print(f"structured_beam({n}): {ne} tets, {nn} nodes", flush=True)
    geo = 16 * ne + 24 * nn  # tets + coordinates
    for mc in (1, 16):
        X = torch.rand((mc, 3 * nn), dtype=torch.float64, device=dev) - 0.5
        S = torch.empty((mc, ne, 6), dtype=torch.float64, device=dev)
        V, W = torch.empty((mc, ne), dtype=torch.float64, device=dev), torch.empty((mc, ne), dtype=torch.float64, device=dev)
        T, M = torch.empty(mc, dtype=torch.float64, device=dev), torch.empty(mc, dtype=torch.float64, device=dev)
        A = torch.empty(mc, dtype=torch.int32, device=dev)
        sec = timed(lambda: rec.stress_raw(mc, X, 3 * nn, S, 6 * ne, V, W, ne, T, M, A))
        report(f"element, all outputs, m={mc}", sec, geo + 24 * nn * mc + 64 * ne * mc)
        if mc == 16:
            sec = timed(lambda: rec.stress_raw(mc, X, 3 * nn, None, 0, None, None, 0, T, M, A))
            report(f"element, totals only, m={mc}", sec, geo + 24 * nn * mc)
        Nod = torch.empty((mc, nn, 6), dtype=torch.float64, device=dev)
        sec = timed(lambda: rec.nodal_raw(mc, 6, S, 6 * ne, Nod, 6 * nn))
        report(f"nodal average, k=6, m={mc}", sec, 24 * ne + 16 * nn + 48 * ne * mc + 48 * nn * mc)
        del X, S, V, W, Nod
    rec.close()
    del m
