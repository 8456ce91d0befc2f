"""Spectral-normalisation mode beside the default: the flagship train step (128^3, batch 1, bf16, noise + dropout + clDice on) of
VanGan(spectral_norm=True) and of the default engine, timed alternately in one process like bench.py's headline loop (host clock
around `steps` unsynchronised steps ending in a device synchronise), and the projection alone (vg_spectral_norm over the four
wrapped kernels of both discriminators + their repack, device events) against its HBM floor: 16 B per wrapped weight and step.
    python tools/bench_specnorm.py [--size 128] [--steps 20] [--warmup 5] [--rounds 3] [--project-only]
`--project-only --steps N` is the run to put under `rocprofv3 --kernel-trace --stats` (sn_pass_kernel / sn_fold_kernel / sn_scale_kernel)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.29          # float4 copy on an MI355X (MI355X_MICROARCH.md)
WRAPPED_WEIGHTS = 64 * 64 + 4096 * 128 + 8192 * 256 + 16384 * 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--project-only', action='store_true')
    a = ap.parse_args()
    from van_gan_amd import VanGan, ops
    from van_gan_amd.synth import synth_volumes
    dev = 'cuda:0'
    dims = (a.size,) * 3
    out = {}
    sn = VanGan(dims, batch_size=1, device=dev, seed=0, spectral_norm=True)
    ops.set_device(0)
    for _ in range(a.warmup):
        sn.disc_S.project(2); sn.disc_I.project(2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        sn.disc_S._sn.run(2); sn.disc_I._sn.run(2)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.steps
    floor = 2 * 16 * WRAPPED_WEIGHTS / (HBM_ACHIEVABLE_TBS * 1e12) * 1e6
    out['projection_us_per_step'] = us
    out['projection_hbm_floor_us'] = floor
    out['projection_bytes_per_step'] = 2 * 16 * WRAPPED_WEIGHTS
    out['projection_note'] = 'both discriminators, 2 projections each, back-to-back calls on one stream (weights 2 x 44 MB: cache-resident between calls)'
    e0.record()
    for _ in range(a.steps):
        sn.disc_S._sn_ptab.run(); sn.disc_I._sn_ptab.run()
    e1.record()
    torch.cuda.synchronize()
    out['repack_wrapped_us_per_step'] = e0.elapsed_time(e1) * 1e3 / a.steps
    if not a.project_only:
        base = VanGan(dims, batch_size=1, device=dev, seed=0)
        rI, rS = synth_volumes(1, *dims, seed=1234)
        rI, rS = rI.to(dev), rS.to(dev)
        engines = {'default': base, 'spectral_norm': sn}
        for e in engines.values():
            for _ in range(a.warmup):
                e.train_step(rI, rS, sync=False)
        torch.cuda.synchronize()
        per = {k: [] for k in engines}
        for _ in range(a.rounds):
            for k, e in engines.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    e.train_step(rI, rS, sync=False)
                e._join_updates()
                torch.cuda.synchronize()
                per[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for k, v in per.items():
            out[k + '_ms_per_step'] = min(v)
            out[k + '_ms_per_step_rounds'] = v
        res = sn.train_step(rI, rS)
        out['finite'] = all(v == v and abs(v) < 1e6 for v in res.values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
