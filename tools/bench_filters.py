"""Device time of the imaging filters -- median_filter (3,3,3) and (3,3,1), threshold_outliers, and prepare_imaging(preprocess=('median',
'rsom'), check=False) -- on synthetic uint8, uint16 and float32 volumes of 256x256x128 and 512x512x140 (the reference's RAW_IMG_SIZE),
beside two baselines taken on the same machine in the same run:

  the streaming floor: the input bytes plus 4 output bytes per voxel at the rate a device-to-device copy of an fp32 volume of the same
    shape reaches here (its bytes read plus its bytes written over its time) -- what a pass that reads the volume once and writes fp32
    once cannot beat; printed for the two single-pass filters (threshold_outliers and the composed recipe make several passes);
  the host: scipy.ndimage.median_filter / the numpy recipe of threshold_outliers / both followed by the reference's RSOM steps, on the
    float32 copy of the volume, as the reference's user runs them.  scipy.ndimage and numpy's element-wise passes run on one thread,
    whatever the number of cores, which is printed.

The raw volume is resident on the device before the timed window; the window is `--iters` back-to-back calls between two HIP events
after `--warmup` calls.  The same volume is filtered in every iteration, so whatever part of it the 256 MiB Infinity Cache holds is read
from there -- for the copy that measures the floor just as for the filters.  Prints every case, then one JSON line.  Needs a GPU; reads
nothing outside the repository.

    python tools/bench_filters.py [--iters 50] [--warmup 3] [--rounds 5] [--shapes 256x256x128,512x512x140] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_preprocess import host_recipe, synth  # noqa: E402
from tools.device_time import device_ms  # noqa: E402

SIZES = [(256, 256, 128), (512, 512, 140)]
DTYPES = ['uint8', 'uint16', 'float32']


def volume(shape, dtype):
    if dtype == 'float32':
        return synth(shape, 'uint16').astype(np.float32) / np.float32(257.0)
    return synth(shape, dtype)


def host_threshold_outliers(x, threshold=6):
    """The numpy recipe of threshold_outliers (mean, std, |z|, the extreme values within the threshold, clip)."""
    mean, std = np.mean(x), np.std(x)
    z = np.abs((x - mean) / std)
    keep = z <= threshold
    return np.clip(x, a_min=np.min(x[keep]), a_max=np.max(x[keep]))


def host_times(x32):
    """Seconds of each host baseline on the float32 volume, and the results the device is compared with."""
    import scipy.ndimage
    t, ref = {}, {}
    for name, size in (('median333', (3, 3, 3)), ('median331', (3, 3, 1))):
        t0 = time.perf_counter()
        ref[name] = scipy.ndimage.median_filter(x32, size=size)
        t[name] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref['outliers'] = host_threshold_outliers(x32)
    t['outliers'] = time.perf_counter() - t0
    t['median_rsom'] = t['median333'] + host_recipe(ref['median333'])[0]['total']
    return t, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default=','.join('x'.join(str(d) for d in s) for s in SIZES))
    ap.add_argument('--no-host', action='store_true', help='skip the host baselines (scipy takes tens of seconds on the large volume)')
    a = ap.parse_args()
    shapes = [tuple(int(d) for d in s.split('x')) for s in a.shapes.split(',')]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_filters: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd.preprocess import as_raw_volume, median_filter, prepare_imaging, threshold_outliers
    cores = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    res = {'bench': 'filters', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rounds': a.rounds, 'host_threads_used': 1,
           'host_cores': cores, 'cases': []}
    print('host baselines: scipy.ndimage / numpy on 1 thread (%d cores available)' % cores, flush=True)
    for shape in shapes:
        n = int(np.prod(shape))
        src = torch.empty(n, device='cuda:0').normal_()
        dst = torch.empty_like(src)
        _, copy_ms, _ = device_ms(lambda: dst.copy_(src), a.iters, a.rounds, a.warmup)
        copy_rate = 8.0 * n / (copy_ms * 1e-3)
        del src, dst
        print('%s: fp32 copy %.4f ms, %.0f GB/s (read + written)' % (shape, copy_ms, copy_rate / 1e9), flush=True)
        host, ref = ({}, {}) if a.no_host else host_times(volume(shape, 'float32'))
        for dtype in DTYPES:
            raw = volume(shape, dtype)
            esz = raw.dtype.itemsize
            floor_ms = (esz + 4.0) * n / copy_rate * 1e3
            vol = as_raw_volume(raw, 'cuda:0')
            runs = (('median333', lambda: median_filter(vol, (3, 3, 3)), True),
                    ('median331', lambda: median_filter(vol, (3, 3, 1)), True),
                    ('outliers', lambda: threshold_outliers(vol), False),
                    ('median_rsom', lambda: prepare_imaging(vol, preprocess=('median', 'rsom'), check=False), False))
            for name, fn, single_pass in runs:
                _, ms, out = device_ms(fn, a.iters, a.rounds, a.warmup)
                case = dict(shape=list(shape), dtype=dtype, op=name, voxels=n, device_ms=round(ms, 4), copy_gbytes_per_s=round(copy_rate / 1e9, 1))
                line = '%s %-7s %-11s device %.4f ms' % (shape, dtype, name, ms)
                if single_pass:
                    case.update(floor_ms=round(floor_ms, 4), over_floor=round(ms / floor_ms, 2))
                    line += ', floor %.4f ms (x%.2f)' % (floor_ms, ms / floor_ms)
                if name in host:
                    case.update(host_s=round(host[name], 3), host_over_device=round(host[name] / (ms * 1e-3), 1))
                    line += ', host %.3f s (x%.0f)' % (host[name], host[name] / (ms * 1e-3))
                    if dtype == 'float32' and name in ref:          # the host ran on this very volume: the device must agree exactly
                        case['equals_host'] = bool(np.array_equal(out.cpu().numpy(), ref[name]))
                        line += ', equals the host result: %s' % case['equals_host']
                print(line, flush=True)
                res['cases'].append(case)
                del out
            del vol
    print(json.dumps(res))


if __name__ == '__main__':
    main()
