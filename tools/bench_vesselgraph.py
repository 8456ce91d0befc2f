"""Device time of skeleton_graph, one prune_spurs round and vessel_graph on the skeleton of the vessel mask of a synthetic prediction of
512x512x140 voxels (bench_skeleton's mask and skeleton), with the entries of skeleton_graph timed one by one (classify, the two
vg_cc_label calls, the tables, the prune pair), beside the host restatement of the same graph on the same skeleton
(tests/vesselgraph_restate.py: numpy and scipy.ndimage.label; what the device is tested against).  Everything is resident on the device
before the timed window; a window is `--iters` back-to-back calls between two HIP events after `--warmup` calls, and the figure is the
median of `--rounds` windows.  skeleton_graph reads two counts back per call to size its tables, so its windows hold that read-back.
Prints every case, then one JSON line.  There is no pass / fail ratio: the numbers are reported.  Needs a GPU; reads nothing outside
the repository.

    python tools/bench_vesselgraph.py [--iters 10] [--warmup 2] [--rounds 3] [--shape 512x512x140] [--min-spur 6] [--no-host]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_vesselgraph.py --kernels-only --calls 5
        (per-launch times of sg_classify / sg_accumulate / sg_finalise / sg_flag / sg_apply: a run of its own, then tools/kstat.py DIR 5 sg_)"""
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

# what a launch must move at the least, in bytes per voxel: classify reads the mask and writes three byte volumes; accumulate and apply
# read one byte where the mask is background, which is nearly everywhere, and apply writes one
FLOOR_BYTES = {'classify': 1 + 3, 'accumulate': 1, 'apply': 1 + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shape', default='512x512x140')
    ap.add_argument('--min-spur', type=float, default=6.0)
    ap.add_argument('--no-host', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--kernels-only', action='store_true', help='--calls calls of skeleton_graph and one prune round and nothing else: the run to trace')
    ap.add_argument('--calls', type=int, default=5)
    a = ap.parse_args()
    shape = tuple(int(d) for d in a.shape.split('x'))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_vesselgraph: no GPU (a CPU run cannot give a device time)')
    from van_gan_amd import postprocess as P
    from van_gan_amd._lib import lib
    from van_gan_amd.ops import _p, stream
    pred = synth_prediction(shape).to('cuda:0')
    mask = P.vessel_mask(pred)
    del pred
    skel, radius = P.vessel_centreline(mask)
    n = mask.numel()
    if a.kernels_only:
        for _ in range(a.calls):
            P.prune_spurs(skel, a.min_spur)
        torch.cuda.synchronize()
        print(json.dumps({'bench': 'vesselgraph', 'kernels_only': True, 'calls': a.calls}))
        return
    g = P.skeleton_graph(skel, radius)
    summary = P.network_summary(g)
    pruned, pinfo = P.prune_spurs(skel, a.min_spur, return_info=True)
    res = {'bench': 'vesselgraph', 'device': torch.cuda.get_device_name(0), 'shape': list(shape), 'voxels': n, 'iters': a.iters, 'rounds': a.rounds,
           'skeleton_voxels': int(skel.sum()), 'summary': summary, 'min_spur': a.min_spur, 'prune': pinfo, 'floor_bytes_per_voxel': FLOOR_BYTES, 'cases': []}
    print('%s: %d voxels, %d on the skeleton; %s; one round at min_length %g: %s' % (shape, n, res['skeleton_voxels'], summary, a.min_spur, pinfo), flush=True)
    X, Y, Z = shape
    deg, bm, nm = (torch.empty(shape, dtype=torch.uint8, device=skel.device) for _ in range(3))
    half, nodes, kind = g.seg_half_steps, g.seg_nodes, g.node_kind
    tables = {f: torch.empty_like(getattr(g, f)) for f in ('seg_half_steps', 'seg_voxels', 'seg_ends', 'seg_nodes', 'seg_length', 'seg_chord', 'seg_radius_mean',
                                                          'node_voxels', 'node_degree', 'node_kind', 'node_centroid')}
    rminmax = torch.empty(g.E + 1, 2, device=skel.device)
    bad = torch.empty(2, dtype=torch.int32, device=skel.device)
    nbytes = int(lib.vg_skelgraph_scratch_bytes(g.E, g.V))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=skel.device)
    flags = torch.empty(g.E + 1, dtype=torch.uint8, device=skel.device)
    out = torch.empty_like(skel)
    counts = torch.empty(2, dtype=torch.int32, device=skel.device)

    def classify():
        P._check(lib.vg_skelgraph_classify(_p(skel), X, Y, Z, _p(deg), _p(bm), _p(nm), stream()), 'vg_skelgraph_classify')

    def fill_tables(r):
        t = tables
        P._check(lib.vg_skelgraph_tables(_p(skel), _p(g.degree), _p(g.segment_labels), _p(g.node_labels), None if r is None else _p(r), X, Y, Z, g.E, g.V, None,
                                         _p(t['seg_half_steps']), _p(t['seg_voxels']), _p(t['seg_ends']), _p(t['seg_nodes']), _p(t['seg_length']), _p(t['seg_chord']),
                                         None if r is None else _p(t['seg_radius_mean']), None if r is None else _p(rminmax), _p(t['node_voxels']),
                                         _p(t['node_degree']), _p(t['node_kind']), _p(t['node_centroid']), _p(bad), _p(scratch), nbytes, stream()), 'vg_skelgraph_tables')

    def prune():
        P._check(lib.vg_skelgraph_prune(_p(skel), _p(g.degree), _p(g.segment_labels), _p(g.node_labels), X, Y, Z, g.E, g.V, _p(half), _p(nodes), _p(kind),
                                        a.min_spur, None, _p(flags), _p(out), _p(counts), stream()), 'vg_skelgraph_prune')
    classify()
    stages = [
        ('skeleton_graph', lambda: P.skeleton_graph(skel)),
        ('skeleton_graph with the radius', lambda: P.skeleton_graph(skel, radius)),
        ('prune_spurs, one round (a skeleton_graph and the prune pair)', lambda: P.prune_spurs(skel, a.min_spur)),
        ('vessel_graph', lambda: P.vessel_graph(mask)),
        ('vessel_centreline (what vessel_graph adds the graph to)', lambda: P.vessel_centreline(mask)),
        ('entry: vg_skelgraph_classify (1 launch)', classify),
        ('entry: vg_cc_label of the segment mask (6 launches)', lambda: P._label(bm, shape, 3)),
        ('entry: vg_cc_label of the node mask (6 launches)', lambda: P._label(nm, shape, 3)),
        ('entry: vg_skelgraph_tables (2 memsets, accumulate, finalise)', lambda: fill_tables(None)),
        ('entry: vg_skelgraph_tables with the radius', lambda: fill_tables(radius)),
        ('entry: vg_skelgraph_prune (memset, flag, apply)', prune),
        ('skeleton_nodes (sk_degree_kernel, the yardstick of a streaming pass)', lambda: P.skeleton_nodes(skel)),
    ]
    for name, fn in stages:
        rounds, med, _ = device_ms(fn, a.iters, a.rounds, a.warmup)
        print('%-70s device %s ms (median %.3f)' % (name, ' '.join('%.3f' % r for r in rounds), med), flush=True)
        res['cases'].append(dict(case=name, device_ms_rounds=[round(r, 4) for r in rounds], device_ms=round(med, 4)))
        torch.cuda.empty_cache()
    if not a.no_host:
        import vesselgraph_restate as G
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s, r = skel.cpu().numpy(), radius.cpu().numpy()
        t1 = time.perf_counter()
        want = G.graph(s, r)
        t2 = time.perf_counter()
        wp = G.prune_round(s, a.min_spur)
        t3 = time.perf_counter()
        same = all(np.array_equal(getattr(g, f).cpu().numpy(), want[f]) for f in ('segment_labels', 'node_labels', 'seg_voxels', 'seg_nodes', 'seg_ends', 'seg_half_steps',
                                                                                  'seg_length', 'seg_radius_mean', 'node_voxels', 'node_degree', 'node_kind'))
        res['host_numpy_restatement'] = dict(copy_out_s=round(t1 - t0, 4), graph_s=round(t2 - t1, 3), prune_round_s=round(t3 - t2, 3), equals_device=bool(same),
                                             prune_equals_device=bool(np.array_equal(wp[0], pruned.cpu().numpy())) and [wp[1]] == pinfo['spurs'])
        print('host numpy restatement: %s' % res['host_numpy_restatement'], flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
