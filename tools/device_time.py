"""The timed window of the preprocessing benchmarks (bench_preprocess, bench_resize, bench_labelprep, bench_filters): `warmup` calls, a
synchronisation, then `rounds` windows of `iters` back-to-back calls between two HIP events."""
import numpy as np


def device_ms(fn, iters, rounds, warmup=0):
    """(milliseconds per call of every round, their median, what the last call returned)."""
    import torch
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms, float(np.median(ms)), out
