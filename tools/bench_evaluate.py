"""Device time of evaluate_segmentation and of the entries of csrc/vg_evaluate.hip one by one, on the vessel mask of a synthetic prediction
of 512x512x140 voxels (bench_components' prediction) as the ground truth and that mask rolled by one voxel along Y with its first three
z-planes cleared as the prediction.  Beside them, in the same process, the yardsticks that exist without this file: vg_fill_holes_apply
(a streaming pass; its achieved bytes per second), vg_neighbour_count26 (the 26-neighbour pass) and vg_order_stats on an fp32 array of
as many values (the radix select).  Then the same scores on the host: numpy counts, scipy.ndimage binary_erosion,
distance_transform_edt and label, the cell count of tests/evaluate_restate.py and the thinning of tests/skeleton_restate.py, compared
with the device's.  Everything is resident on the device before the timed window; a window is `--iters` back-to-back calls between two
HIP events after `--warmup` calls, and the figure is the median of `--rounds` windows.  evaluate_segmentation reads its result block
back once per call (and, thinning until nothing changes, a few words per four passes), so its windows hold those read-backs.  Prints
every case, then one JSON line.  There is no pass / fail ratio: the numbers are reported.  Needs a GPU; reads nothing outside the
repository.

    python tools/bench_evaluate.py [--iters 10] [--warmup 2] [--rounds 3] [--shape 512x512x140] [--no-host] [--no-host-skeleton]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_evaluate.py --kernels-only --calls 5
        (per-launch times of the ev_ kernels: a run of its own, then tools/kstat.py DIR 5 ev_)"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tools.bench_components import synth_prediction  # noqa: E402
from tools.device_time import device_ms  # noqa: E402

# what a launch must move at the least, in bytes per voxel
FLOOR_BYTES = {'vg_mask_counts': 2, 'vg_mask_surface': 1 + 2, 'vg_euler_characteristic': 1, 'vg_masked_stats reduce': 4 + 1, 'vg_fill_holes_apply': 1 + 4 + 1,
               'vg_neighbour_count26': 1 + 1, 'vg_order_stats pass': 4}


def host_scores(P, T, skeleton: bool):
    """(seconds per part, dict of scores) on the host, by scipy where scipy has the function"""
    import scipy.ndimage as ndi
    import evaluate_restate as R
    import skeleton_restate as S
    sec, out = {}, {}
    t = time.perf_counter()
    out.update(R.overlap(P, T))
    sec['overlap'] = time.perf_counter() - t
    t = time.perf_counter()
    sp, st = R.surface(P) != 0, R.surface(T) != 0
    d_pt, d_tp = ndi.distance_transform_edt(~st)[sp], ndi.distance_transform_edt(~sp)[st]
    out.update(surface_pred=int(sp.sum()), surface_truth=int(st.sum()), hausdorff=float(max(d_pt.max(), d_tp.max())),
               hausdorff_percentile=float(max(np.sort(d)[R.rank(0.95, len(d))] for d in (d_pt, d_tp))),
               assd=(math.fsum(d_pt.tolist()) + math.fsum(d_tp.tolist())) / (len(d_pt) + len(d_tp)))
    sec['surface'] = time.perf_counter() - t
    t = time.perf_counter()
    out.update(betti_pred=R.betti(P), betti_truth=R.betti(T), euler_pred=R.euler(P), euler_truth=R.euler(T))
    sec['topology'] = time.perf_counter() - t
    if skeleton:
        t = time.perf_counter()
        c = R.cldice(P, T)
        out.update(tprec=c['tprec'], tsens=c['tsens'], cldice=c['cldice'])
        sec['cldice'] = time.perf_counter() - t
    return {k: round(v, 3) for k, v in sec.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', default='512x512x140')
    ap.add_argument('--no-host', action='store_true', help='skip the host scores')
    ap.add_argument('--no-host-skeleton', action='store_true', help='skip the thinning of the two masks on the host (the slowest part)')
    ap.add_argument('--kernels-only', action='store_true', help='--calls calls of evaluate_segmentation and nothing else: the run to trace')
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    shape = tuple(int(d) for d in a.shape.split('x'))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_evaluate: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd import postprocess as P
    from van_gan_amd._lib import lib
    from van_gan_amd.ops import _p, stream
    dev = 'cuda:0'
    truth = P.vessel_mask(synth_prediction(shape).to(dev))
    pred = torch.roll(truth, 1, 1)
    pred[:, :, :3] = 0
    n = truth.numel()
    X, Y, Z = shape
    if a.kernels_only:
        for _ in range(a.calls):
            P.evaluate_segmentation(pred, truth, max_passes=8)
        torch.cuda.synchronize()
        print(json.dumps({'bench': 'evaluate', 'kernels_only': True, 'calls': a.calls}))
        return
    scores = P.evaluate_segmentation(pred, truth)
    res = {'bench': 'evaluate', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'voxels': n, 'iters': a.iters, 'rounds': a.rounds,
           'scores': {k: v for k, v in scores.as_dict().items()}, 'floor_bytes_per_voxel': FLOOR_BYTES, 'cases': []}
    print('%s: %d voxels; %s' % (shape, n, res['scores']), flush=True)

    block = torch.zeros(64, dtype=torch.uint8, device=dev)
    surf, nsurf, out8 = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(3))
    P._check(lib.vg_mask_surface(_p(pred), X, Y, Z, _p(surf), _p(nsurf), _p(block), stream()), 'vg_mask_surface')
    sq = P._edt(nsurf, shape, None, True)
    dist = P._edt(nsurf, shape, (0.5, 1.0, 2.5), False)
    labels, _, result = P._label((truth == 0).view(torch.uint8), shape, 1)
    flags = torch.empty(P.sizes_capacity(n), dtype=torch.uint8, device=dev)
    P._check(lib.vg_fill_holes_mark(_p(labels), X, Y, Z, _p(flags), stream()), 'vg_fill_holes_mark')
    sbytes = int(lib.vg_masked_stats_scratch_bytes(n, 4))
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    obytes = int(lib.vg_order_stats_scratch_bytes(n, 4))
    oscratch = torch.empty(obytes, dtype=torch.uint8, device=dev)
    ostats = torch.empty(4, device=dev)
    q1, q4 = (ctypes.c_double * 1)(0.95), (ctypes.c_double * 4)(0.5, 0.95, 1.0, 0.25)
    r1, r4 = (ctypes.c_int64 * 1)(int(0.95 * n)), (ctypes.c_int64 * 4)(n // 2, int(0.95 * n), n - 1, n // 4)
    ones = torch.ones(shape, dtype=torch.uint8, device=dev)

    def stats(keys, sel, kind, q, R):
        P._check(lib.vg_masked_stats(_p(keys), _p(sel), n, kind, q, R, _p(block), _p(scratch), sbytes, stream()), 'vg_masked_stats')

    stages = [
        ('evaluate_segmentation, everything on (thinning until nothing changes)', lambda: P.evaluate_segmentation(pred, truth)),
        ('evaluate_segmentation, everything on, max_passes=8 (one read-back)', lambda: P.evaluate_segmentation(pred, truth, max_passes=8)),
        ('evaluate_segmentation with a sampling', lambda: P.evaluate_segmentation(pred, truth, (0.5, 1.0, 2.5), max_passes=8)),
        ('evaluate_segmentation, overlap only', lambda: P.evaluate_segmentation(pred, truth, topology=False, surface=False, cldice=False)),
        ('evaluate_segmentation, overlap and topology', lambda: P.evaluate_segmentation(pred, truth, surface=False, cldice=False)),
        ('evaluate_segmentation, overlap and surface', lambda: P.evaluate_segmentation(pred, truth, topology=False, cldice=False)),
        ('evaluate_segmentation, overlap and cldice, max_passes=8', lambda: P.evaluate_segmentation(pred, truth, topology=False, surface=False, max_passes=8)),
        ('entry: vg_mask_counts (memset, 1 launch)', lambda: P._check(lib.vg_mask_counts(_p(pred), _p(truth), n, _p(block), stream()), 'vg_mask_counts')),
        ('entry: vg_mask_surface, both outputs (memset, 1 launch)',
         lambda: P._check(lib.vg_mask_surface(_p(pred), X, Y, Z, _p(surf), _p(nsurf), _p(block), stream()), 'vg_mask_surface')),
        ('entry: vg_euler_characteristic (memset, 1 launch)', lambda: P._check(lib.vg_euler_characteristic(_p(pred), X, Y, Z, _p(block), stream()), 'vg_euler_characteristic')),
        ('entry: vg_flags_count (memset, 1 launch)', lambda: P._check(lib.vg_flags_count(_p(flags), _p(result), n, _p(block), stream()), 'vg_flags_count')),
        ('entry: vg_masked_stats, squared int32 over the surface, R = 1 (10 launches)', lambda: stats(sq, surf, P.EVAL_SQ_I32, q1, 1)),
        ('entry: vg_masked_stats, fp32 over the surface, R = 1', lambda: stats(dist, surf, P.EVAL_DIST_F32, q1, 1)),
        ('entry: vg_masked_stats, fp32 over every voxel, R = 1', lambda: stats(dist, ones, P.EVAL_DIST_F32, q1, 1)),
        ('entry: vg_masked_stats, fp32 over every voxel, R = 4', lambda: stats(dist, ones, P.EVAL_DIST_F32, q4, 4)),
        ('yardstick: vg_order_stats on the same fp32 array, R = 1 (9 launches)',
         lambda: P._check(lib.vg_order_stats(_p(dist), n, r1, 1, _p(ostats), _p(oscratch), obytes, stream()), 'vg_order_stats')),
        ('yardstick: vg_order_stats on the same fp32 array, R = 4',
         lambda: P._check(lib.vg_order_stats(_p(dist), n, r4, 4, _p(ostats), _p(oscratch), obytes, stream()), 'vg_order_stats')),
        ('yardstick: vg_fill_holes_apply (a streaming pass, 6 bytes per voxel)',
         lambda: P._check(lib.vg_fill_holes_apply(_p(truth), _p(labels), _p(flags), n, _p(out8), stream()), 'vg_fill_holes_apply')),
        ('yardstick: vg_neighbour_count26 (skeleton_nodes)', lambda: P._check(lib.vg_neighbour_count26(_p(pred), X, Y, Z, _p(out8), stream()), 'vg_neighbour_count26')),
    ]
    for name, fn in stages:
        rounds, med, _ = device_ms(fn, a.iters, a.rounds, a.warmup)
        print('%-82s device %s ms (median %.3f)' % (name, ' '.join('%.3f' % r for r in rounds), med), flush=True)
        res['cases'].append(dict(case=name, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4)))
        torch.cuda.empty_cache()
    ms = {c['case'].split(' (')[0].split(',')[0]: c['device_ms'] for c in res['cases']}
    res['gbytes_per_s'] = {k: round(FLOOR_BYTES[k] * n / (ms[case] * 1e-3) / 1e9, 1) for k, case in (
        ('vg_mask_counts', 'entry: vg_mask_counts'), ('vg_mask_surface', 'entry: vg_mask_surface'), ('vg_euler_characteristic', 'entry: vg_euler_characteristic'),
        ('vg_fill_holes_apply', 'yardstick: vg_fill_holes_apply'), ('vg_neighbour_count26', 'yardstick: vg_neighbour_count26'))}
    print('achieved GB/s against the bytes a launch must move: %s' % res['gbytes_per_s'], flush=True)
    if not a.no_host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hp, ht = pred.cpu().numpy(), truth.cpu().numpy()
        copy_s = time.perf_counter() - t0
        sec, want = host_scores(hp, ht, not a.no_host_skeleton)
        got = scores.as_dict()
        close = ('assd',)
        same = all((abs(got[k] - v) <= 1e-12 * abs(v)) if k in close else got[k] == v for k, v in want.items())
        res['host'] = dict(copy_out_s=round(copy_s, 4), seconds=sec, total_s=round(sum(sec.values()), 3), equals_device=bool(same),
                           differing=[k for k, v in want.items() if (k not in close and got[k] != v)])
        print('host: %s' % res['host'], flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
