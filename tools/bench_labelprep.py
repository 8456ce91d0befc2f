"""Device time of prepare_segmentation(check=False) -- conversion to fp32, min / max, the exact value mode of the normalised stack, the
binarising pass -- at 256x256x128 and 512x512x140 (the reference's RAW_IMG_SIZE) on three inputs: (a) a binary uint8 label stack, (b) the
same stack resized by a non-integer factor (three Lanczos-4 passes and the clamp in front), (c) an all-distinct fp32 volume, the worst
case of the mode's hash table: every value is a global insert of its own.  Beside each: the host time of the same recipe in numpy / scipy
on this machine, and the streaming floor -- the bytes the passes move over 6.3 TB/s, what a copy reaches.  The raw volume is resident on
the device before the timed window; the window is `--iters` back-to-back calls between two HIP events after `--warmup` calls.  Prints
every case, then one JSON line.  Needs a GPU; reads nothing outside the repository.

    python tools/bench_labelprep.py [--iters 20] [--warmup 3] [--rounds 3] [--shapes 256x256x128,512x512x140] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.device_time import device_ms  # noqa: E402

SIZES = [(256, 256, 128), (512, 512, 140)]
COPY_RATE = 6.3e12           # bytes / s: what a float4 copy measures on the MI355X (the HBM3E specification is 8.0e12)
RESIZE = 1.3                 # case (b): every axis grows by this factor (rounded)


def synth_labels(shape, seed=0):
    """A vessel-like binary stack: a few percent of the voxels are foreground (255), in runs along z."""
    rng = np.random.default_rng(seed)
    seeds = rng.random(shape, dtype=np.float32) < 0.01
    fg = seeds.copy()
    for s in range(1, 4):
        fg[..., s:] |= seeds[..., :-s]
    return np.where(fg, 255, 0).astype(np.uint8)


def synth_distinct(shape, seed=0):
    """n different fp32 values in a random order: the n bit patterns that follow 1.0 (they reach about 21 at 512x512x140)."""
    n = int(np.prod(shape))
    bits = np.random.default_rng(seed).permutation(n).astype(np.uint32) + np.uint32(0x3F800000)
    return bits.view(np.float32).reshape(shape)


def host_recipe(stack):
    """The reference's steps on the host: min-max, scipy's mode, the inversion, (x - 0.5) / 0.5, binarise.  (seconds, result)"""
    import scipy.stats
    t0 = time.perf_counter()
    s = stack.astype(np.float32)
    s = (s - s.min()) / (s.max() - s.min())
    if scipy.stats.mode(s, axis=None).mode == 1:
        s -= 1.
        s = abs(s)
    s = (s - 0.5) / 0.5
    s[s < 0.] = -1.0
    s[s >= 0.] = 1.0
    return time.perf_counter() - t0, s


def slots(n):
    s = 2
    while s < 2 * n:
        s <<= 1
    return s


def pass_bytes(n_in, esz, n, resized_passes):
    """Bytes the device passes move: the conversion reads the raw stack and writes fp32; each resize pass reads its input and writes its
    output (given as a list of (voxels in, voxels out)) and the clamp reads and writes fp32; min / max reads fp32 twice; the mode fills
    its table (8 bytes a slot), reads fp32 once and scans the table; the binarising pass reads and writes fp32."""
    b = n_in * (esz + 4)
    for vin, vout in resized_passes:
        b += 4 * (vin + vout)
    if resized_passes:
        b += 8 * n
    return b + 8 * n + (8 * slots(n) + 4 * n + 8 * slots(n)) + 8 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', default=','.join('x'.join(str(d) for d in s) for s in SIZES))
    ap.add_argument('--no-host', action='store_true', help='skip the numpy / scipy recipe (minutes on the all-distinct volume)')
    a = ap.parse_args()
    shapes = [tuple(int(d) for d in s.split('x')) for s in a.shapes.split(',')]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_labelprep: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd.preprocess import as_raw_volume, prepare_segmentation, resize_volume
    res = {'bench': 'labelprep', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rounds': a.rounds, 'cases': []}
    for shape in shapes:
        labels = synth_labels(shape)
        target = tuple(int(round(d * RESIZE)) for d in shape)
        for name, raw, tgt in (('binary-uint8', labels, None), ('binary-uint8-resized', labels, target), ('distinct-fp32', synth_distinct(shape), None)):
            n_in, esz = raw.size, raw.dtype.itemsize
            out_shape = shape if tgt is None else tgt
            n = int(np.prod(out_shape))
            passes = []
            if tgt is not None:                                             # Y, then X, then Z
                s1, s2 = (shape[0], tgt[1], shape[2]), (tgt[0], tgt[1], shape[2])
                passes = [(n_in, int(np.prod(s1))), (int(np.prod(s1)), int(np.prod(s2))), (int(np.prod(s2)), n)]
            vol = as_raw_volume(raw, 'cuda:0')
            out = None
            for _ in range(a.warmup):
                out = prepare_segmentation(vol, check=False, target_size=tgt)
            torch.cuda.synchronize()
            _, info = prepare_segmentation(vol, target_size=tgt, return_info=True)
            host_s, same = None, None
            if not a.no_host:
                stack = raw if tgt is None else np.clip(resize_volume(vol, tgt).cpu().numpy(), 0, 255)      # the host is timed on the device's resize
                host_s, ref = host_recipe(stack)
                same = bool(np.array_equal(out.cpu().numpy()[..., 0], ref))
            rounds, med, out = device_ms(lambda: prepare_segmentation(vol, check=False, target_size=tgt), a.iters, a.rounds)
            nbytes = pass_bytes(n_in, esz, n, passes)
            floor_ms = nbytes / COPY_RATE * 1e3
            case = dict(case=name, shape=list(shape), out_shape=list(out_shape), voxels=n, device_ms_rounds=[round(r, 4) for r in rounds],
                        device_ms=round(med, 4), pass_bytes=nbytes, table_bytes=8 * slots(n), floor_ms=round(floor_ms, 4),
                        device_over_floor=round(med / floor_ms, 2), host_s=None if host_s is None else round(host_s, 3),
                        host_over_device=None if host_s is None else round(host_s / (med * 1e-3), 1), equals_host=same, info=info)
            if name == 'distinct-fp32':
                case['inserts_per_s_whole_call'] = round(n / (med * 1e-3), 0)
            print('%s %s: device %s ms (median %.3f), floor %.3f ms (x%.2f), host %s s, equal to the host recipe: %s, %s'
                  % (shape, name, ' '.join('%.3f' % r for r in rounds), med, floor_ms, med / floor_ms,
                     'n/a' if host_s is None else '%.2f' % host_s, same, info), flush=True)
            res['cases'].append(case)
            del vol, out
            torch.cuda.empty_cache()
    # the mode alone on the all-distinct volumes: its achieved inserts per second
    from van_gan_amd.preprocess import value_mode
    for shape in shapes:
        x = torch.from_numpy(synth_distinct(shape)).to('cuda:0')
        ms = device_ms(lambda: value_mode(x), a.iters, 1, a.warmup)[1]
        print('%s value_mode, all distinct: %.3f ms, %.3g inserts / s' % (shape, ms, x.numel() / (ms * 1e-3)), flush=True)
        res['cases'].append(dict(case='value_mode-distinct-fp32', shape=list(shape), device_ms=round(ms, 4), inserts_per_s=round(x.numel() / (ms * 1e-3), 0)))
        del x
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
