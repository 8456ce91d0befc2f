"""The selectable loss kernels beside the ones the default step runs, in one process:
  * vg_lp_loss (p = 1, 4; with and without the gradient) beside vg_mse on two 128^3 fp32 volumes -- the same bytes (two reads, and a
    store with the gradient), so the expectation is the same time within the spread; launches alternate, device events around `steps`
    back-to-back launches per variant and round, the minimum over the rounds and every round are printed;
  * vg_logit_loss (both kinds) beside vg_mse_const on the 2 * 16^3 patch logits of a 128^3 step (32 KB: a launch-latency measurement);
  * the flagship train step (128^3, batch 1, bf16, noise + dropout + clDice on) of each non-default configuration of
    tests/test_gpu_losstypes.py beside the default engine, timed alternately like bench.py's headline loop (host clock around `steps`
    unsynchronised steps ending in a device synchronise).
    python tools/bench_losses.py [--size 128] [--steps 20] [--warmup 5] [--rounds 3] [--kernels-only]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.29          # float4 copy on an MI355X (MI355X_MICROARCH.md)
CONFIGS = [('mae', 'L4', None), ('mse', 'bce', 'bce'), ('L4', 'mae', 'bfce')]


def _time_alternating(variants, steps, rounds, warmup):
    """variants: {name: callable}.  us per call: min over rounds, and every round."""
    for f in variants.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    per = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in variants.items():
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            per[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    return {k: dict(us=min(v), rounds=v) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    from van_gan_amd import VanGan, ops
    from van_gan_amd.synth import synth_volumes
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    ops.set_device(0)
    out = {}
    n = a.size ** 3
    g = torch.Generator(device=dev).manual_seed(1)
    x, y = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev)
    gb, acc = torch.zeros(n, device=dev), torch.zeros(8, device=dev)
    ksteps = max(a.steps, 50)
    var = {'vg_mse': lambda: ops.mse(x, y, acc[0:1]), 'vg_lp_loss_p1': lambda: ops.lp_loss(x, y, 1, acc[1:2]),
           'vg_lp_loss_p2': lambda: ops.lp_loss(x, y, 2, acc[1:2]), 'vg_lp_loss_p4': lambda: ops.lp_loss(x, y, 4, acc[2:3]),
           'vg_mse_grad': lambda: ops.mse(x, y, acc[0:1], 0.5, gb), 'vg_lp_loss_p1_grad': lambda: ops.lp_loss(x, y, 1, acc[1:2], 0.5, gb),
           'vg_lp_loss_p2_grad': lambda: ops.lp_loss(x, y, 2, acc[1:2], 0.5, gb), 'vg_lp_loss_p4_grad': lambda: ops.lp_loss(x, y, 4, acc[2:3], 0.5, gb)}
    out['volume_kernels'] = _time_alternating(var, ksteps, a.rounds, a.warmup)
    out['volume_bytes'] = dict(forward=8 * n, with_gradient=12 * n)
    out['volume_hbm_floor_us'] = dict(forward=8 * n / (HBM_ACHIEVABLE_TBS * 1e12) * 1e6, with_gradient=12 * n / (HBM_ACHIEVABLE_TBS * 1e12) * 1e6)
    out['volume_note'] = 'back-to-back launches on the same two %d-MB volumes: cache-resident between calls' % (4 * n >> 20)
    nl = 2 * (a.size // 8) ** 3
    lg = torch.randn(nl, generator=g, device=dev) * 3.0
    gx = torch.zeros(nl, device=dev)
    var = {'vg_mse_const_grad': lambda: ops.mse_const(lg, 1.0, acc[3:4], 0.5, gx),
           'vg_logit_loss_bce_grad': lambda: ops.logit_loss(lg, 1.0, ops.LOGIT_BCE, acc[4:5], 0.5, gx),
           'vg_logit_loss_bfce_grad': lambda: ops.logit_loss(lg, 1.0, ops.LOGIT_FOCAL, acc[5:6], 0.5, gx),
           'vg_mse_const': lambda: ops.mse_const(lg, 1.0, acc[3:4]),
           'vg_logit_loss_bce': lambda: ops.logit_loss(lg, 1.0, ops.LOGIT_BCE, acc[4:5]),
           'vg_logit_loss_bfce': lambda: ops.logit_loss(lg, 1.0, ops.LOGIT_FOCAL, acc[5:6])}
    out['logit_kernels'] = _time_alternating(var, ksteps, a.rounds, a.warmup)
    out['logit_elements'] = nl
    del x, y, gb
    if not a.kernels_only:
        dims = (a.size,) * 3
        rI, rS = synth_volumes(1, *dims, seed=1234)
        rI, rS = rI.to(dev), rS.to(dev)
        names = ['default'] + ['%s/%s/%s' % c for c in CONFIGS]
        kws = [dict()] + [dict(cycle_loss_SIS=c[0], cycle_loss_ISI=c[1], gan_loss=c[2]) for c in CONFIGS]
        per = {k: [] for k in names}
        engines = {}
        for k, kw in zip(names, kws):
            e = engines[k] = VanGan(dims, batch_size=1, device=dev, seed=0, **kw)
            for _ in range(a.warmup):
                e.train_step(rI, rS, sync=False)
            e._join_updates()
            torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, e in engines.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    e.train_step(rI, rS, sync=False)
                e._join_updates()
                torch.cuda.synchronize()
                per[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        out['train_step_ms'] = {k: dict(ms=min(v), rounds=v) for k, v in per.items()}
        out['finite'] = all(all(v == v and abs(v) < 1e6 for v in e.train_step(rI, rS).values()) for e in engines.values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
