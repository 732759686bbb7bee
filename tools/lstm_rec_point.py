#!/usr/bin/env python3
"""Time ``saa_lstm_recurrence_forward`` at the production shape of the training pass (B = 10, T = 20, widths 50 and 100), for
one build of the library or for two next to each other:

    python tools/lstm_rec_point.py [--other OLDER/libsaa_hip.so] [--repeats 5] [--seconds 1.0]

Every figure is device events around a run of back-to-back launches long enough to last ``--seconds`` (calibrated once per
library and width), after a warm-up; with ``--other`` the two libraries alternate, repeat by repeat, in one process on one
GPU.  Prints per library and width the microseconds per launch of every repeat, their median and their min-max spread, and
the largest difference between the outputs of the two builds."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch  # before the library: one HIP runtime per process, torch's

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synchronization_avoiding_algorithms_amd import _lib  # noqa: E402

B, T = 10, 20


def bind(path):
    lib = C.CDLL(path)
    res, args = _lib.SIGNATURES["saa_lstm_recurrence_forward"]
    lib.saa_lstm_recurrence_forward.restype, lib.saa_lstm_recurrence_forward.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="a second libsaa_hip.so (an older build) to alternate with")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    libs = {"this": bind(_lib.LIB_PATH)}
    if a.other:
        libs["other"] = bind(os.path.abspath(a.other))
    stream = torch.cuda.current_stream().cuda_stream
    for width in (50, 100):
        g = torch.Generator().manual_seed(width)
        pre = (torch.randn(B, T, 4 * width, generator=g) * 0.5).cuda()
        W = (torch.randn(4 * width, width, generator=g) * 0.2).cuda()
        c0 = (torch.randn(B, width, generator=g) * 0.3).cuda()
        outs = {k: [torch.empty(B, T, n, device="cuda") for n in (width, width, 4 * width, width)] for k in libs}

        def launch(k, n):
            fn, o = libs[k].saa_lstm_recurrence_forward, [t.data_ptr() for t in outs[k]]
            for _ in range(n):
                code = fn(0, B, T, width, 0, pre.data_ptr(), None, c0.data_ptr(), W.data_ptr(), *o, stream)
                if code != 0:
                    raise RuntimeError(f"saa_lstm_recurrence_forward returned {code}")

        def timed(k, n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            launch(k, n)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e-3

        count = {}
        for k in libs:
            timed(k, 2000)                                          # warm-up
            count[k] = max(2000, int(2000 * a.seconds * 1.1 / timed(k, 2000)))
        us = {k: [] for k in libs}
        for _ in range(a.repeats):
            for k in libs:
                us[k].append(timed(k, count[k]) / count[k] * 1e6)
        for k, v in us.items():
            print(f"width {width:3d} {k:5s}: {count[k]} launches per region, us per launch "
                  f"{' '.join(f'{x:.3f}' for x in v)} | median {statistics.median(v):.3f} min {min(v):.3f} max {max(v):.3f}")
        if a.other:
            diff = max(float((x - y).abs().max()) for x, y in zip(outs["this"], outs["other"]))
            print(f"width {width:3d}: largest difference between the two builds' outputs {diff:.2e}; "
                  f"median(this) / median(other) = {statistics.median(us['this']) / statistics.median(us['other']):.4f}")


if __name__ == "__main__":
    main()
