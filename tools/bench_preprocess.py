"""Device time of prepare_imaging(check=False) -- slice moments, z-score, radix select of four order statistics, percentile clip and
rescale -- on synthetic uint8 and uint16 volumes of 256x256x128 and 512x512x140 (the reference's RAW_IMG_SIZE), beside the host time of
the same recipe in numpy / scipy on this machine.  The raw volume is resident on the device before the timed window (the upload is a copy
of 1 or 2 bytes per voxel and is timed separately); the window is `--iters` back-to-back calls between two HIP events after `--warmup`
calls.  Prints every round, then one JSON line.  Needs a GPU; reads nothing outside the repository.

The same volume is preprocessed in every iteration, so whatever part of it the 256 MiB Infinity Cache holds is read from there: the rate
printed is that of the passes' bytes over the device time, and its share of the 8.0 TB/s HBM3E peak (6.3 TB/s is what a copy reaches).

    python tools/bench_preprocess.py [--iters 200] [--warmup 5] [--rounds 5] [--shapes 256x256x128,512x512x140]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.device_time import device_ms  # noqa: E402

SIZES = [(256, 256, 128), (512, 512, 140)]
DTYPES = ['uint8', 'uint16']
HBM_PEAK = 8.0e12            # bytes / s, the MI355X's HBM3E specification; a float4 copy measures 6.3e12


def synth(shape, dtype, seed=0):
    """A vessel-like stack: a dim noisy background whose level drifts with depth, sparse bright voxels."""
    rng = np.random.default_rng(seed)
    top = 255.0 if dtype == 'uint8' else 65535.0
    depth = (0.08 + 0.04 * np.cos(np.arange(shape[2]) / 9.0))[None, None, :]
    v = rng.gamma(2.0, 0.5, shape).astype(np.float32) * depth.astype(np.float32)
    v += (rng.random(shape, dtype=np.float32) < 0.01) * rng.random(shape, dtype=np.float32)
    return np.clip(v * top, 0, top).astype(dtype)


def host_recipe(raw, lower=0.05, upper=99.95):
    """The reference's steps on the host, as its user runs them: float32 stack, slice loop, two scoreatpercentile calls, clip, min-max,
    (x - 0.5) / 0.5.  Returns (seconds of each stage, result)."""
    import scipy.stats
    t0 = time.perf_counter()
    img = raw.astype(np.float32)
    for z in range(img.shape[2]):
        sl = img[..., z]
        sd = np.std(sl)
        img[..., z] = (sl - np.mean(sl)) / sd if sd > 0. else sl - np.mean(sl)
    t1 = time.perf_counter()
    lp = scipy.stats.scoreatpercentile(img, lower)
    up = scipy.stats.scoreatpercentile(img, upper)
    t2 = time.perf_counter()
    img[img < lp] = lp
    img[img > up] = up
    mn, mx = img.min(), img.max()
    img = ((img - mn) / (mx - mn) - 0.5) / 0.5
    t3 = time.perf_counter()
    return dict(slices=t1 - t0, percentiles=t2 - t1, clip_rescale=t3 - t2, total=t3 - t0), img


def pass_bytes(n, esz):
    """Bytes the device passes move: moments read the raw volume, the z-score reads it again and writes fp32, four digit passes read fp32,
    the rescale reads and writes fp32 (in place)."""
    return n * (2 * esz + 4 + 4 * 4 + 4 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', default=','.join('x'.join(str(d) for d in s) for s in SIZES))
    a = ap.parse_args()
    shapes = [tuple(int(d) for d in s.split('x')) for s in a.shapes.split(',')]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_preprocess: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd.preprocess import as_raw_volume, prepare_imaging
    res = {'bench': 'preprocess', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rounds': a.rounds, 'cases': []}
    for shape in shapes:
        for dtype in DTYPES:
            raw = synth(shape, dtype)
            n, esz = raw.size, raw.dtype.itemsize
            host, ref = host_recipe(raw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vol = as_raw_volume(raw, 'cuda:0')
            torch.cuda.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            out = None
            for _ in range(a.warmup):
                out = prepare_imaging(vol, check=False)
            torch.cuda.synchronize()
            err = float(np.abs(out.cpu().numpy()[..., 0].astype(np.float64) - ref).max())      # the host recipe is fp32: agreement, not parity
            rounds, med, out = device_ms(lambda: prepare_imaging(vol, check=False), a.iters, a.rounds)
            t0 = time.perf_counter()
            for _ in range(a.iters):
                prepare_imaging(vol, check=True)
            checked_ms = (time.perf_counter() - t0) * 1e3 / a.iters
            case = dict(shape=list(shape), dtype=dtype, voxels=n, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4),
                        checked_wall_ms=round(checked_ms, 4), upload_ms=round(upload_ms, 3), pass_bytes=pass_bytes(n, esz),
                        gbytes_per_s=round(pass_bytes(n, esz) / (med * 1e-3) / 1e9, 1),
                        share_of_hbm_peak=round(pass_bytes(n, esz) / (med * 1e-3) / HBM_PEAK, 3), host_s={k: round(v, 4) for k, v in host.items()},
                        host_over_device=round(host['total'] / (med * 1e-3), 1), max_abs_diff_vs_host_fp32=err)
            print('%s %s: device %s ms (median %.3f), checked %.3f ms wall, host %.3f s, %.0f GB/s of pass bytes (%.0f %% of the HBM peak), |diff| %.2e'
                  % (shape, dtype, ' '.join('%.3f' % r for r in rounds), med, checked_ms, host['total'], case['gbytes_per_s'], 100 * case['share_of_hbm_peak'], err), flush=True)
            res['cases'].append(case)
            del vol, out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
