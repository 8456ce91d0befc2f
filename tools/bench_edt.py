"""Device time of distance_transform_edt, fill_holes and vessel_radius on the vessel mask of a synthetic prediction of 512x512x140 voxels
(bench_components' prediction run through vessel_mask), beside the path they replace on this machine: device -> host copy of the mask,
scipy.ndimage.distance_transform_edt / binary_fill_holes, host -> device copy of the result.  Then the worst case of the transform,
timed once: one background voxel in a block of 256^3, where no scan ends early.  The mask is resident on the device before the timed
window; a window is `--iters` back-to-back calls between two HIP events after `--warmup` calls, and the figure is the median of
`--rounds` windows.  Prints every case, then one JSON line.  There is no pass / fail ratio: both numbers are reported.  Needs a GPU;
reads nothing outside the repository.

    python tools/bench_edt.py [--iters 10] [--warmup 2] [--rounds 3] [--shape 512x512x140] [--worst 256] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_components import synth_prediction  # noqa: E402
from tools.device_time import device_ms  # noqa: E402

# bytes per voxel each launch must move through HBM at the least (reads + writes); the neighbours an axis pass looks at are counted as
# cache hits, the label reads of the face kernel as nothing
LAUNCH_BYTES = {
    'edt pass Z (int32)': 1 + 4, 'edt pass Y (int32)': 4 + 4, 'edt pass X (int32 -> fp32)': 4 + 4,
    'edt pass Z (fp64)': 1 + 8, 'edt pass Y (fp64)': 8 + 8, 'edt pass X (fp64 -> fp32)': 8 + 4,
    'invert': 1 + 1, 'label (vg_cc_label, six launches)': 1 + 12 + 1 + 12 + 4 + 8, 'mark': 0, 'apply': 1 + 4 + 1,
}


def host_path(mask_dev, fn):
    """(seconds of each step, result on the device): copy out, fn on the host, copy back."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask_dev.cpu().numpy()
    t1 = time.perf_counter()
    out = fn(m)
    t2 = time.perf_counter()
    back = torch.from_numpy(np.ascontiguousarray(out)).to(mask_dev.device)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dict(copy_out_s=round(t1 - t0, 4), scipy_s=round(t2 - t1, 4), copy_back_s=round(t3 - t2, 4), total_s=round(t3 - t0, 4)), back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', default='512x512x140')
    ap.add_argument('--worst', type=int, default=256, help='edge of the worst-case block (0: skip it)')
    ap.add_argument('--no-host', action='store_true', help='skip the scipy paths (seconds)')
    a = ap.parse_args()
    shape = tuple(int(d) for d in a.shape.split('x'))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_edt: no GPU (a CPU run cannot give a device time)')
    import scipy.ndimage as ndi
    from van_gan_amd import postprocess as P
    pred = synth_prediction(shape).to('cuda:0')
    mask, info = P.vessel_mask(pred, return_info=True)
    del pred
    n = mask.numel()
    sampling = (2.0, 0.5, 1.25)
    radius = P.distance_transform_edt(mask)
    res = {'bench': 'edt', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'voxels': n, 'iters': a.iters, 'rounds': a.rounds,
           'mask': info, 'largest_radius': float(radius.max()), 'mean_radius_of_foreground': float(radius[mask != 0].mean()),
           'launch_bytes_per_voxel': LAUNCH_BYTES, 'cases': []}
    print('%s: %d voxels, %s, largest radius %.3f' % (shape, n, info, res['largest_radius']), flush=True)
    stages = [
        ('distance_transform_edt', lambda: P.distance_transform_edt(mask)),
        ('distance_transform_edt(squared)', lambda: P.distance_transform_edt(mask, squared=True)),
        ('distance_transform_edt(sampling)', lambda: P.distance_transform_edt(mask, sampling)),
        ('fill_holes', lambda: P.fill_holes(mask)),
        ('label_components(inverted mask, 1)', lambda: P.label_components(mask == 0, 1)),
        ('vessel_radius', lambda: P.vessel_radius(mask)),
        ('vessel_radius(fill=False)', lambda: P.vessel_radius(mask, fill=False)),
    ]
    for name, fn in stages:
        rounds, med, _ = device_ms(fn, a.iters, a.rounds, a.warmup)
        print('%-42s device %s ms (median %.3f)' % (name, ' '.join('%.3f' % r for r in rounds), med), flush=True)
        res['cases'].append(dict(case=name, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4)))
        torch.cuda.empty_cache()
    if not a.no_host:
        host = {}
        host['distance_transform_edt'], back = host_path(mask, lambda m: ndi.distance_transform_edt(m).astype(np.float32))
        host['distance_transform_edt']['equals_device'] = bool(torch.equal(back, radius))
        host['fill_holes'], back = host_path(mask, lambda m: ndi.binary_fill_holes(m).astype(np.uint8))
        host['fill_holes']['equals_device'] = bool(torch.equal(back, P.fill_holes(mask)))
        host['fill_holes']['filled_voxels'] = int(back.sum()) - int(mask.sum())
        for k, v in host.items():
            print('host %s: %s' % (k, v), flush=True)
        res['host'] = host
    if a.worst:
        e = a.worst
        block = torch.ones(e, e, e, dtype=torch.uint8, device='cuda:0')
        block[0, 0, 0] = 0
        P.distance_transform_edt(block[:8].contiguous())               # the kernels are loaded; this size has not run
        rounds, med, out = device_ms(lambda: P.distance_transform_edt(block, squared=True), 1, 1, 0)
        ok = int(out[-1, -1, -1]) == 3 * (e - 1) ** 2 and int(out[0, 0, 1]) == 1
        print('worst case %d^3, one background voxel: device %.3f ms (one call), far corner right: %s' % (e, med, ok), flush=True)
        res['worst_case'] = dict(edge=e, device_ms_once=round(med, 4), far_corner_right=ok)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
