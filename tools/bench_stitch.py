"""Sliding-window inference modes side by side, in one process: bench.py --infer's configuration (256x256x128 volume, 128^3 windows,
stride 50, symmetric pad 0.1, 10 % border crop, process_img, window_batch 2; bf16 and fp16) stitched with blend='count' (the default
per-window path), blend='gaussian' and blend='gaussian' + tta='xyz' (8 forwards per window).
    python tools/bench_stitch.py [--rounds 7] [--volumes 3] [--warmup 2] [--tta-volumes 2]
count and gaussian alternate round by round (a round = `volumes` volumes, host clock around them ending in a device synchronise); every
round's figure is printed so that the spread is on the line, and gaussian / count is formed from the medians.  The TTA figure is
information only: 8 times as many forwards cost 8 times as much.  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--volumes', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--tta-volumes', type=int, default=2)
    ap.add_argument('--size', type=int, default=128, help='window edge (the volume is 2 x 2 x 1 windows); 128 is the configuration of record')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stitch.py needs the GPU: there is nothing to time without one')
    from van_gan_amd import VanGan
    dev = 'cuda:0'
    k = (a.size,) * 3
    eng = VanGan(k, batch_size=2, device=dev, seed=0)
    vol = (torch.rand(2 * a.size, 2 * a.size, a.size, 1, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    base = dict(stride=(50, 50, 50), complete=True, padFactor=0.1, process_img=True, window_batch=2)
    modes = {'count': dict(), 'gaussian': dict(blend='gaussian'), 'gaussian_tta_xyz': dict(blend='gaussian', tta='xyz')}
    out = {'workload': 'stitch_subvolumes %dx%dx%d, windows of %d^3, stride 50, pad 0.1, process_img, window_batch 2' % (tuple(vol.shape[:3]) + (a.size,)),
           'rounds': a.rounds, 'volumes_per_round': a.volumes, 'warmup': a.warmup}

    def run(mode, precision, n):
        res = None
        t0 = time.perf_counter()
        for _ in range(n):
            res = eng.stitch_subvolumes('gen_IS', vol, k, precision=precision, **base, **modes[mode])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, res

    for precision in (None, 'fp16'):
        tag = precision or 'bf16'
        last = {}
        for m in ('count', 'gaussian'):
            _, last[m] = run(m, precision, max(a.warmup, 2))
        per = {'count': [], 'gaussian': []}
        for _ in range(a.rounds):
            for m in per:
                ms, last[m] = run(m, precision, a.volumes)
                per[m].append(ms)
        r = {}
        for m, v in per.items():
            s = sorted(v)
            r[m] = {'ms_per_volume_median': s[len(s) // 2], 'ms_per_volume_min': s[0], 'ms_per_volume_max': s[-1], 'rounds_ms': v}
        r['gaussian_over_count'] = r['gaussian']['ms_per_volume_median'] / r['count']['ms_per_volume_median']
        run('gaussian_tta_xyz', precision, 1)
        ms, last['gaussian_tta_xyz'] = run('gaussian_tta_xyz', precision, a.tta_volumes)
        r['gaussian_tta_xyz'] = {'ms_per_volume': ms, 'volumes': a.tta_volumes, 'over_count': ms / r['count']['ms_per_volume_median']}
        r['finite'] = all(bool(torch.isfinite(t).all()) for t in last.values())
        r['max_abs_gaussian_minus_count'] = float((last['gaussian'] - last['count']).abs().max())
        out[tag] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
