"""Attention-gate mode beside the default: the flagship train step (128^3, batch 1, bf16, noise + dropout + clDice on) of
VanGan(attention_gate=True) and of the default engine, timed alternately in one process like bench.py's headline loop (host clock
around `steps` unsynchronised steps ending in a device synchronise), and the gate launches alone at the four level shapes of the patch
(device events around `steps` back-to-back launches) against the bytes they move.  Every launch of a timed loop works on ANOTHER set of
buffers, enough sets to cover 1 GB, so that no launch finds its operands in the 256 MB memory-side cache: the rates are HBM rates.
    python tools/bench_attngate.py [--size 128] [--steps 20] [--warmup 5] [--rounds 3] [--kernels-only]
`--kernels-only --steps N` is the run to put under `rocprofv3 --kernel-trace --stats` (ag_fwd_kernel / ag_bwd_kernel)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

LEVELS = {0: (16, 32), 1: (32, 64), 2: (64, 128), 3: (128, 256)}


def gate_bytes(N, lv, Cs, Ci, esz=2):
    """HBM traffic of one launch if every tensor moves once: forward reads skip and phi, writes gated and h; backward reads dG, skip, h
    and phi, writes d_skip and d_phi (weights and statistics are negligible)."""
    V = N * lv[0] * lv[1] * lv[2]
    fwd = V * (2 * Cs * esz + 4) + (V // 8) * Ci * esz
    bwd = V * (3 * Cs * esz + 4) + 2 * (V // 8) * Ci * esz
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    from van_gan_amd import VanGan, ops
    from van_gan_amd.synth import synth_volumes
    dev = 'cuda:0'
    dims = (a.size,) * 3
    ops.set_device(0)
    out = {'kernels': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for level, (Cs, Ci) in LEVELS.items():
        for N in (1, 2):                      # forward applications are N = 1, the paired backward sweep is N = 2
            lv = tuple(n >> level for n in dims)
            low = tuple(n // 2 for n in lv)
            rn = lambda *s: torch.randn(*s, generator=g, device=dev)
            nb = gate_bytes(N, lv, Cs, Ci)
            nrot = max(2, min(64, -(-(1 << 30) // nb[0])))
            sets = []
            for _ in range(nrot):
                skip, phi, dg = rn(N, *lv, Cs).bfloat16(), rn(N, *low, Ci).bfloat16(), rn(N, *lv, Cs).bfloat16()
                sets.append((skip, phi, dg, torch.empty_like(skip), torch.empty(N, *lv, device=dev), torch.empty_like(skip), torch.empty_like(phi)))
            wt, bt, wp, bp = rn(1, 1, 1, Cs, Ci) * 0.3, rn(Ci) * 0.1, rn(1, 1, 1, Ci, 1) * 0.3, rn(1)
            sums = torch.zeros(ops.STRIPES, N, Cs, 2, device=dev)
            gw = [torch.zeros_like(t) for t in (wt, bt, wp, bp)]
            turn = [0]

            def fwd():
                skip, phi, dg, gated, h, dskip, dphi = sets[turn[0] % nrot]
                turn[0] += 1
                ops.attn_gate_fwd(skip, phi, wt, bt, wp, bp, (N,) + lv, Cs, Ci, gated, h, sums)

            def bwd():
                skip, phi, dg, gated, h, dskip, dphi = sets[turn[0] % nrot]
                turn[0] += 1
                ops.attn_gate_bwd(dg, skip, h, phi, wt, bt, wp, (N,) + lv, Cs, Ci, dskip, False, dphi, *gw)
            for _ in range(nrot):                 # h of every set holds a real gate before the backward is timed
                fwd()
            for name, fn, b in (('fwd', fwd, nb[0]), ('bwd', bwd, nb[1])):
                for _ in range(a.warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / a.steps
                out['kernels']['level%d_N%d_%s' % (level, N, name)] = dict(sets=nrot, us=round(us, 2), MB=round(b / 1e6, 2), TBps=round(b / us / 1e6, 3))
    if not a.kernels_only:
        gated_eng = VanGan(dims, batch_size=1, device=dev, seed=0, attention_gate=True)
        base = VanGan(dims, batch_size=1, device=dev, seed=0)
        rI, rS = synth_volumes(1, *dims, seed=1234)
        rI, rS = rI.to(dev), rS.to(dev)
        engines = {'default': base, 'attention_gate': gated_eng}
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
        res = gated_eng.train_step(rI, rS)
        out['finite'] = all(v == v and abs(v) < 1e6 for v in res.values())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
