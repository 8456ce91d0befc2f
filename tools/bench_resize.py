"""Device time of the Lanczos-4 volume resize -- resize_volume alone, every pass of it alone, and prepare_imaging(check=False,
target_size=...) -- on a synthetic uint16 stack of 512x512x140 (the reference's RAW_IMG_SIZE) resized to 512x512x128 (its
TARG_RAW_IMG_SIZE: the Z pass only) and to 256x256x128 (all three axes).  The input is resident on the device before the timed window; the
window is `--iters` back-to-back calls between two HIP events after `--warmup` calls; the median of `--rounds` windows is reported.  Prints
every case, then one JSON line.  Needs a GPU; reads nothing outside the repository.

A pass reads its source once and writes its target once (the 36 T bytes of its table aside): 4 (L + T) outer inner bytes.  The rate printed
is that of these bytes over the device time, beside its share of the 6.3 TB/s a float4 copy reaches on an MI355X.  The same volume is
resized in every iteration, so whatever part of it the 256 MiB Infinity Cache holds is read from there.

    python tools/bench_resize.py [--iters 50] [--warmup 3] [--rounds 5] [--cases 512x512x140:512x512x128,512x512x140:256x256x128]"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.device_time import device_ms  # noqa: E402

CASES = '512x512x140:512x512x128,512x512x140:256x256x128'
COPY_RATE = 6.3e12           # bytes / s: what a float4 copy measures on an MI355X (the HBM3E specification is 8.0e12)


def synth(shape, seed=0):
    """A vessel-like 16-bit stack: a dim noisy background whose level drifts with depth, sparse bright voxels."""
    rng = np.random.default_rng(seed)
    depth = (0.08 + 0.04 * np.cos(np.arange(shape[2]) / 9.0))[None, None, :]
    v = rng.gamma(2.0, 0.5, shape).astype(np.float32) * depth.astype(np.float32)
    v += (rng.random(shape, dtype=np.float32) < 0.01) * rng.random(shape, dtype=np.float32)
    return np.clip(v * 65535.0, 0, 65535.0).astype(np.uint16)


def passes(shape, target):
    """[(axis name, outer, L, inner, T)] of the passes resize_volume runs, in its order."""
    s, out = list(shape), []
    for axis in (1, 0, 2):
        if s[axis] != target[axis]:
            out.append(('YXZ'[(1, 0, 2).index(axis)], math.prod(s[:axis]), s[axis], math.prod(s[axis + 1:]), target[axis]))
            s[axis] = target[axis]
    return out


def timed(fn, warmup, iters, rounds):
    ms, med, _ = device_ms(fn, iters, rounds, warmup)
    return [round(m, 4) for m in ms], med


def rate(nbytes, ms):
    return dict(bytes=nbytes, gbytes_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), share_of_copy_rate=round(nbytes / (ms * 1e-3) / COPY_RATE, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cases', default=CASES)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_resize: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd.preprocess import as_raw_volume, prepare_imaging, resample_axis, resize_volume, zscore_slices
    res = {'bench': 'resize', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rounds': a.rounds, 'cases': []}
    for spec in a.cases.split(','):
        shape, target = (tuple(int(d) for d in s.split('x')) for s in spec.split(':'))
        raw = as_raw_volume(synth(shape), 'cuda:0')
        x = zscore_slices(raw)                                      # a resident fp32 volume: what resize_volume alone is timed on
        case = dict(shape=list(shape), target=list(target), passes=[])
        total = 0
        for name, outer, L, inner, T in passes(shape, target):
            src = torch.randn(outer, L, inner, device='cuda:0')
            rounds, med = timed(lambda: resample_axis(src, T), a.warmup, a.iters, a.rounds)
            nbytes = 4 * (L + T) * outer * inner
            total += nbytes
            case['passes'].append(dict(axis=name, outer=outer, L=L, inner=inner, T=T, device_ms_rounds=rounds, device_ms=round(med, 4), **rate(nbytes, med)))
            print('%s -> %s pass %s (outer %d, L %d, inner %d, T %d): %.4f ms, %.0f GB/s (%.0f %% of a copy)'
                  % (shape, target, name, outer, L, inner, T, med, nbytes / med / 1e6, 100 * nbytes / (med * 1e-3) / COPY_RATE), flush=True)
            del src
        rounds, med = timed(lambda: resize_volume(x, target), a.warmup, a.iters, a.rounds)
        case['resize_volume'] = dict(device_ms_rounds=rounds, device_ms=round(med, 4), **rate(total, med))
        print('%s -> %s resize_volume: %s ms (median %.4f), %.0f GB/s of pass bytes' % (shape, target, ' '.join('%.4f' % r for r in rounds), med, total / med / 1e6), flush=True)
        for tgt, key in ((None, 'prepare_imaging'), (target, 'prepare_imaging_target')):
            rounds, med = timed(lambda: prepare_imaging(raw, check=False, target_size=tgt), a.warmup, a.iters, a.rounds)
            case[key] = dict(device_ms_rounds=rounds, device_ms=round(med, 4))
            print('%s prepare_imaging(check=False, target_size=%s): median %.4f ms' % (shape, tgt, med), flush=True)
        res['cases'].append(case)
        del raw, x
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
