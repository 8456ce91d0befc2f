"""Device time of vessel_mask and of its three stages -- binarise_prediction, label_components, and the removal of small components on
given labels -- on a synthetic prediction of 512x512x140 voxels (the reference's RAW_IMG_SIZE): synth.py's label recipe (tubular blobs,
5 % foreground) in blocks of 128x128x140, the tubes bright on a dark background with Gaussian noise, so that the threshold leaves a
vascular network and some thousands of specks.  Beside it, the path it replaces, on this machine: device -> host copy of the mask,
scipy.ndimage.label, the np.bincount filter, host -> device copy of the result.  The prediction is resident on the device before the
timed window; the window is `--iters` back-to-back calls between two HIP events after `--warmup` calls.  Prints every case, then one
JSON line.  There is no pass / fail ratio: both numbers are reported.  Needs a GPU; reads nothing outside the repository.

    python tools/bench_components.py [--iters 10] [--warmup 2] [--rounds 3] [--shape 512x512x140] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.device_time import device_ms  # noqa: E402

BLOCK = (128, 128)


def synth_prediction(shape, seed=0):
    """fp32 [X,Y,Z] in [0, 255]: 255 * minmax of (0.15 + 0.7 * tubes + noise), the tubes from synth_volumes' real_S."""
    import torch
    from van_gan_amd.synth import synth_volumes
    X, Y, Z = shape
    bx, by = -(-X // BLOCK[0]), -(-Y // BLOCK[1])
    _, S = synth_volumes(bx * by, BLOCK[0], BLOCK[1], Z, seed=1234 + seed)                  # [B, 128, 128, Z, 1] in {-1, +1}
    S = S[..., 0].reshape(bx, by, BLOCK[0], BLOCK[1], Z).permute(0, 2, 1, 3, 4).reshape(bx * BLOCK[0], by * BLOCK[1], Z)[:X, :Y]
    g = torch.Generator().manual_seed(seed)
    v = 0.15 + 0.35 * (S + 1.0) + 0.1 * torch.randn(S.shape, generator=g)
    v = (v - v.min()) / (v.max() - v.min())
    return (255.0 * v).to(torch.float32).contiguous()


def host_path(mask_dev, min_size, connectivity):
    """(seconds of each step, result on the device): copy out, scipy.ndimage.label, bincount filter, copy back."""
    import scipy.ndimage as ndi
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask_dev.cpu().numpy()
    t1 = time.perf_counter()
    lab, K = ndi.label(m, structure=ndi.generate_binary_structure(3, connectivity))
    t2 = time.perf_counter()
    keep = np.bincount(lab.ravel(), minlength=K + 1) >= min_size
    keep[0] = False
    out = keep[lab].astype(np.uint8)
    t3 = time.perf_counter()
    back = torch.from_numpy(out).to(mask_dev.device)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    return dict(copy_out_s=t1 - t0, label_s=t2 - t1, filter_s=t3 - t2, copy_back_s=t4 - t3, total_s=t4 - t0, components=int(K)), back


# bytes per voxel each launch moves through HBM at the least (reads + writes), the random reads of a union-find not counted
LAUNCH_BYTES = {
    'threshold': 4 + 1, 'local': 1 + 12, 'border': 1, 'flatten': 4 + 4 + 4, 'number': 4, 'relabel': 4 + 4, 'filter': 4 + 1,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', default='512x512x140')
    ap.add_argument('--threshold', type=float, default=127.5)
    ap.add_argument('--min-size', type=int, default=64)
    ap.add_argument('--connectivity', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip the scipy path (seconds)')
    a = ap.parse_args()
    shape = tuple(int(d) for d in a.shape.split('x'))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_components: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd import postprocess as P
    pred = synth_prediction(shape).to('cuda:0')
    n = pred.numel()
    mask = P.binarise_prediction(pred, a.threshold)
    labels, K, sizes = P.label_components(mask, a.connectivity, return_sizes=True)
    result = torch.tensor([K, 0, int(mask.sum()), 0], dtype=torch.int32, device=pred.device)
    full_sizes = torch.zeros(P.sizes_capacity(n), dtype=torch.int32, device=pred.device)
    full_sizes[:K + 1] = sizes
    out, info = P.vessel_mask(pred, a.threshold, a.min_size, a.connectivity, return_info=True)
    res = {'bench': 'components', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'voxels': n, 'iters': a.iters, 'rounds': a.rounds,
           'threshold': a.threshold, 'min_size': a.min_size, 'connectivity': a.connectivity, 'info': info, 'launch_bytes_per_voxel': LAUNCH_BYTES, 'cases': []}
    print('%s: %d voxels, %s' % (shape, n, info), flush=True)
    stages = [
        ('binarise_prediction', lambda: P.binarise_prediction(pred, a.threshold)),
        ('binarise_prediction(otsu)', lambda: P.binarise_prediction(pred, 'otsu')),
        ('label_components', lambda: P.label_components(mask, a.connectivity)),
        ('filter (vg_cc_filter on given labels)', lambda: P._filter(labels, full_sizes, result, a.min_size)),
        ('remove_small_objects', lambda: P.remove_small_objects(mask, a.min_size, a.connectivity)),
        ('vessel_mask', lambda: P.vessel_mask(pred, a.threshold, a.min_size, a.connectivity)),
    ]
    for c in (1, 2):
        if c != a.connectivity:
            stages.append(('label_components(connectivity=%d)' % c, lambda c=c: P.label_components(mask, c)))
    for name, fn in stages:
        rounds, med, _ = device_ms(fn, a.iters, a.rounds, a.warmup)
        print('%-42s device %s ms (median %.3f)' % (name, ' '.join('%.3f' % r for r in rounds), med), flush=True)
        res['cases'].append(dict(case=name, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4)))
        torch.cuda.empty_cache()
    if not a.no_host:
        host, back = host_path(mask, a.min_size, a.connectivity)
        host['equals_device'] = bool(torch.equal(back, out))
        print('host path: %s' % {k: (round(v, 4) if isinstance(v, float) else v) for k, v in host.items()}, flush=True)
        res['host'] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in host.items()}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
