"""Device time of skeletonize, skeleton_nodes and vessel_centreline on the vessel mask of a synthetic prediction of 512x512x140 voxels
(bench_components' prediction run through vessel_mask), beside the host restatement of the same thinning on the same mask
(tests/skeleton_restate.py: numpy, vectorised per sub-step -- NOT scikit-image, which is not on these machines; it is what the device
is tested against, and the only other implementation of this schedule).  The mask is resident on the device before the timed window; a
window is `--iters` back-to-back calls between two HIP events after `--warmup` calls, and the figure is the median of `--rounds`
windows.  skeletonize and vessel_centreline thin until nothing changes, so their windows hold one read-back per four passes; the
enqueue-only form (max_passes = the passes needed) is timed beside them.  Prints every case, then one JSON line.  There is no pass /
fail ratio: the numbers are reported.  Needs a GPU; reads nothing outside the repository.

    python tools/bench_skeleton.py [--iters 10] [--warmup 2] [--rounds 3] [--shape 512x512x140] [--no-host]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_skeleton.py --kernels-only --calls 5
        (per-launch times of sk_pack / sk_mark / sk_thin / sk_unpack / sk_degree: a run of its own, then tools/kstat.py DIR 5 sk_)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tools.bench_components import synth_prediction  # noqa: E402
from tools.device_time import device_ms  # noqa: E402

# what a launch must move at the least, in bytes per voxel: pack reads the bytes and writes the bits, unpack the reverse; a pass is 6 mark
# launches (read two bit words, write one) and 48 thin launches that together read the image and the marks once more and write what changed
FLOOR_BYTES = {'pack': 1 + 1 / 8, 'unpack': 1 / 8 + 1, 'pass (54 launches), at most': 6 * 3 / 8 + 6 * 2 / 8, 'degree': 1 + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', default='512x512x140')
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement (tens of seconds)')
    ap.add_argument('--kernels-only', action='store_true', help='--calls calls of skeletonize and skeleton_nodes and nothing else: the run to trace')
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    shape = tuple(int(d) for d in a.shape.split('x'))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_skeleton: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd import postprocess as P
    pred = synth_prediction(shape).to('cuda:0')
    mask, info = P.vessel_mask(pred, return_info=True)
    del pred
    n = mask.numel()
    skel, sk_info = P.skeletonize(mask, return_info=True)
    passes = sk_info['passes']
    if a.kernels_only:
        for _ in range(a.calls):
            P.skeleton_nodes(P.skeletonize(mask, passes))
        torch.cuda.synchronize()
        print(json.dumps({'bench': 'skeleton', 'kernels_only': True, 'calls': a.calls, 'passes': passes, 'launches_per_call': 2 + 54 * passes + 1}))
        return
    nodes = P.skeleton_nodes(skel)
    on = nodes[skel != 0]
    res = {'bench': 'skeleton', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'voxels': n, 'iters': a.iters, 'rounds': a.rounds,
           'mask': info, 'passes': passes, 'deleted': sk_info['deleted'], 'skeleton_voxels': int(skel.sum()),
           'end_points': int((on == 1).sum()), 'segment_voxels': int((on == 2).sum()), 'junction_voxels': int((on >= 3).sum()),
           'isolated_voxels': int((on == 0).sum()), 'bit_volume_bytes': shape[0] * shape[1] * ((shape[2] + 63) // 64) * 8,
           'launches_per_pass': 54, 'floor_bytes_per_voxel': FLOOR_BYTES, 'cases': []}
    print('%s: %d voxels, %s; %d passes %s -> %d skeleton voxels, %d end points, %d junction voxels'
          % (shape, n, info, passes, sk_info['deleted'], res['skeleton_voxels'], res['end_points'], res['junction_voxels']), flush=True)
    stages = [
        ('skeletonize', lambda: P.skeletonize(mask)),
        ('skeletonize(max_passes=%d) enqueue-only' % passes, lambda: P.skeletonize(mask, passes)),
        ('skeletonize(max_passes=1): pack, one pass, unpack', lambda: P.skeletonize(mask, 1)),
        ('skeleton_nodes', lambda: P.skeleton_nodes(skel)),
        ('vessel_centreline', lambda: P.vessel_centreline(mask)),
        ('vessel_radius (what vessel_centreline adds the thinning to)', lambda: P.vessel_radius(mask)),
    ]
    for name, fn in stages:
        rounds, med, _ = device_ms(fn, a.iters, a.rounds, a.warmup)
        print('%-62s device %s ms (median %.3f)' % (name, ' '.join('%.3f' % r for r in rounds), med), flush=True)
        res['cases'].append(dict(case=name, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4)))
        torch.cuda.empty_cache()
    if not a.no_host:
        import skeleton_restate as R
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = mask.cpu().numpy()
        t1 = time.perf_counter()
        want, deleted = R.skeletonize(m)
        t2 = time.perf_counter()
        res['host_numpy_restatement'] = dict(copy_out_s=round(t1 - t0, 4), thinning_s=round(t2 - t1, 3), passes=len(deleted),
                                             equals_device=bool(np.array_equal(want, skel.cpu().numpy())) and deleted == sk_info['deleted'])
        print('host numpy restatement (not scikit-image): %s' % res['host_numpy_restatement'], flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
