"""BASELINE configs 2-5 on the product engine (tests/test_gpu_fp32.py and test_gpu_nets.py cover config 1's 32^3 cube).

  config 2  64^3, batch 2              exact-parity mode vs the committed oracle fixture tests/golden/train_step_64_b2.npz
  config 3  128x128x64, batch 2        the non-cubic shape: fixture at 64x64x32 (train_step_64x64x32_b2.npz) + full-size properties
  config 4  128^3, batch 1 per GPU     full-size properties (the kernels it selects are compared with the oracle one by one at
                                       true layer shapes in tests/test_gpu_layers.py)
  config 5  256x256x128 sliding window product precision (bf16) through the stitch oracle driven by the HIP generator itself
  ragged    32x48x80, batch 1          a legal patch no tile divides: fixture train_step_32x48x80_b1.npz; 48x80x96, batch 1 (no
                                       power-of-two axis): full-size properties (layer by layer: tests/test_gpu_ragged.py)
  batch 3   64^3, batch 3              the reference's own per-GPU batch: full-size properties; 128^3, batch 3 (its training
                                       configuration): three product steps, finite and with a constant workspace peak (layer by
                                       layer: tests/test_gpu_batch3.py)

Full-size properties: finite losses, bf16 engine vs exact-parity (fp32 storage) engine on the same weights and inputs within
the bf16 tolerance of tests/test_gpu_nets.py (3e-2), workspace peak constant from the second step on.
Fixtures are made by tests/golden/make_golden_configs.py from the float32 oracle (the reference cannot run here)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import stitch_oracle as S  # noqa: E402
from oracle import vangan_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize('fixture', ['train_step_64_b2', 'train_step_64x64x32_b2', 'train_step_32x48x80_b1'])
def test_train_step_matches_fixture(fixture):
    from van_gan_amd import VanGan
    f = np.load(os.path.join(GOLD, fixture + '.npz'))
    dims, B = tuple(int(v) for v in f['dims']), int(f['batch'])
    eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32')
    eng.load_weights(O.make_models(int(f['seed'])))
    rI, rS = O.synth_volumes(B, *dims, seed=int(f['data_seed']))
    res = eng.train_step(rI.cuda(), rS.cuda(), noise={}, drop={}, apply=False)
    for i, k in enumerate(O.RESULT_KEYS):
        ref = float(f['losses'][i])
        print('   %-24s hip %.6f  fixture %.6f' % (k, res[k], ref))
        assert abs(res[k] - ref) <= 2e-3 * abs(ref) + 1e-6, k
    got = eng._aux['fake_S'][0].float().cpu().numpy()
    rel = np.linalg.norm(got - f['fake_S0']) / np.linalg.norm(f['fake_S0'])
    assert rel < 2e-3, rel
    grads = eng.export_grads()
    for key in [k for k in f.files if k.startswith('grad:')]:
        net, name = key[5:].split('/')
        g, r = grads[net][name], torch.from_numpy(f[key])
        c = _cos(g, r)
        rl = float((g.double().cpu() - r.double()).norm() / (r.double().norm() + 1e-300))
        print('   %-28s cos %.6f rel %.2e' % (key, c, rl))
        assert c > 0.9995 and rl < 5e-2, key


@pytest.mark.parametrize('dims,B', [((128, 128, 64), 2), ((128, 128, 128), 1), ((48, 80, 96), 1), ((64, 64, 64), 3)],
                         ids=['config3 128x128x64 b2', 'config4 128^3 b1', 'ragged 48x80x96 b1', 'batch3 64^3 b3'])
def test_full_size_properties(dims, B):
    from van_gan_amd import VanGan
    rI, rS = O.synth_volumes(B, *dims, seed=77)
    rI, rS = rI.cuda(), rS.cuda()
    out = {}
    for prec in ('bf16', 'fp32'):
        eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=3, layer_noise=0.0, dropout_rate=0.0, precision=prec)
        res = eng.train_step(rI, rS, noise={}, drop={}, apply=False)
        out[prec] = res
        assert all(math.isfinite(v) for v in res.values()), res
        if prec == 'bf16':               # the product configuration: noise + dropout on, Adam applied, three steps
            eng2 = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=3)
            peaks = []
            for _ in range(3):
                r = eng2.train_step(rI, rS)
                assert all(math.isfinite(v) for v in r.values()), r
                peaks.append(eng2.arena.peak)
            assert peaks[1] == peaks[2], peaks
            del eng2
        del eng
        torch.cuda.empty_cache()
    for k in O.RESULT_KEYS:
        a, b = out['bf16'][k], out['fp32'][k]
        print('   %-24s bf16 %.6f  fp32-mode %.6f' % (k, a, b))
        assert abs(a - b) <= 3e-2 * abs(b) + 1e-5, k


def test_reference_training_configuration_128_b3():
    """128^3 at batch 3 per GPU, the configuration the reference trains with: the bf16 product engine with noise,
    dropout and Adam on, three steps.  All ten losses finite at every step, workspace peak constant from the second step on.  One
    engine only (its arena is B * S * 8000 bytes + 512 MiB, about 50 GB); the kernels it selects are compared with the oracle one by one
    in tests/test_gpu_batch3.py."""
    from van_gan_amd import VanGan
    dims, B = (128, 128, 128), 3
    rI, rS = O.synth_volumes(B, *dims, seed=77)
    rI, rS = rI.cuda(), rS.cuda()
    eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=3)
    try:
        peaks = []
        for step in range(3):
            r = eng.train_step(rI, rS)
            print('   step %d  %s' % (step, '  '.join('%s %.5f' % (k, r[k]) for k in O.RESULT_KEYS)))
            assert len(O.RESULT_KEYS) == 10 and all(math.isfinite(r[k]) for k in O.RESULT_KEYS), r
            assert all(math.isfinite(v) for v in r.values()), r
            peaks.append(eng.arena.peak)
        assert peaks[1] == peaks[2], peaks
    finally:
        del eng
        torch.cuda.empty_cache()


def test_config5_sliding_window_full_size_product_precision():
    """256x256x128 volume, 128^3 windows, stride 50, symmetric pad 0.1, 10 % border crop, per-window min-max
    (post_training.py:38-39): the product path (batched windows on two lanes, GPU overlap-add / divide / crop / min-max)
    against oracle/stitch_oracle.py driven window by window by the SAME bf16 HIP generator."""
    from van_gan_amd import VanGan
    k = (128, 128, 128)
    eng = VanGan(k, batch_size=2, device='cuda:0', seed=5)
    vol = torch.rand(256, 256, 128, 1, generator=torch.Generator().manual_seed(3)) * 2 - 1
    net, ar = eng.gen_IS, eng.arena
    calls = []

    def gen(a):
        ar.reset()
        x = ar.alloc((1,) + k + (1,), torch.float32)
        y = ar.alloc((1,) + k + (1,), torch.float32)
        x.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        net.forward(ar, x, y, save=False)
        torch.cuda.synchronize()
        calls.append(1)
        return y.cpu().numpy()

    kw = dict(stride=(50, 50, 50), complete=True, padFactor=0.1, process_img=True)
    ref = S.stitch_subvolumes(gen, vol.numpy(), (1,) + k + (1,), **kw)
    assert len(calls) == 50                                   # 5 x 5 x 2 windows
    got = eng.stitch_subvolumes('gen_IS', vol, k, window_batch=2, **kw).cpu().numpy()
    assert got.shape == ref.shape == (256, 256, 128, 1) and np.isfinite(got).all()
    assert got.min() == 0.0 and abs(got.max() - 255.0) < 1e-3   # 255 * min-max (custom_callback.py:202); every voxel was covered
    err = np.abs(got - ref)
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print('stitch 256x256x128 bf16: max abs err %.4f, mean %.5f (0..255 scale), rel L2 %.3e' % (err.max(), err.mean(), rel))
    # Same generator, same windows; only the batch composition differs -- but per-sample InstanceNorm sums are float atomics
    # (order varies from launch to launch) and the bf16 generator amplifies one flipped rounding to its noise floor
    # (oracle with jittered roundings: rel 1.8e-2 on a generator output, tests/test_oracle_kat.py::test_bf16_noise_floor).
    # A stitching error (wrong origin / crop / count) would be O(1): a shifted window alone gives rel > 0.3.
    assert rel < 4e-2 and err.mean() < 2.0, (rel, float(err.mean()), float(err.max()))
    # exact-parity storage has no such floor: the same comparison with the fp32-mode generator at one z-slab of windows
    eng32 = VanGan(k, batch_size=2, device='cuda:0', seed=5, precision='fp32')
    net32, ar32 = eng32.gen_IS, eng32.arena

    def gen32(a):
        ar32.reset()
        x = ar32.alloc((1,) + k + (1,), torch.float32)
        y = ar32.alloc((1,) + k + (1,), torch.float32)
        x.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        net32.forward(ar32, x, y, save=False)
        torch.cuda.synchronize()
        return y.cpu().numpy()
    sub = vol[:, :128, :, :]                                    # 256 x 128 x 128: 5 x 2 x 2 = 20 windows
    ref32 = S.stitch_subvolumes(gen32, sub.numpy(), (1,) + k + (1,), **kw)
    got32 = eng32.stitch_subvolumes('gen_IS', sub, k, window_batch=2, **kw).cpu().numpy()
    e32 = np.abs(got32 - ref32).max()
    print('stitch 256x128x128 fp32 mode: max abs err %.5f (0..255 scale)' % e32)
    assert e32 < 0.05
    # fp16 storage (what BASELINE config 5 names): the product stitch with precision='fp16' on the same weights against the
    # fp32-mode stitch of the same sub-volume -- fp16 keeps 11 significand bits, 8x finer than bf16
    got16 = eng32.stitch_subvolumes('gen_IS', sub, k, window_batch=2, precision='fp16', **kw).cpu().numpy()
    rel16 = float(np.linalg.norm(got16 - got32) / np.linalg.norm(got32))
    print('stitch 256x128x128 fp16 vs fp32 mode: rel L2 %.3e, max abs %.4f (0..255 scale)' % (rel16, float(np.abs(got16 - got32).max())))
    assert np.isfinite(got16).all() and rel16 < 1e-2
    got16f = eng.stitch_subvolumes('gen_IS', vol, k, window_batch=2, precision='fp16', **kw).cpu().numpy()
    assert got16f.shape == (256, 256, 128, 1) and np.isfinite(got16f).all() and got16f.min() == 0.0 and abs(got16f.max() - 255.0) < 1e-3


def test_paired_backward_equals_two_sweeps():
    """VG_PAIR_BWD (one 2B-sample backward sweep per generator over paired tensors) against the schedule it replaced (two
    B-sample sweeps per generator): same gradients up to the run-to-run noise of the generator sweeps -- exact-parity mode, 32^3, batch 2,
    no noise / dropout."""
    from van_gan_amd import VanGan, vangan as V
    dims, B = (32, 32, 32), 2
    rI, rS = O.synth_volumes(B, *dims, seed=7)
    grads = {}
    saved = V._PAIR_BWD
    try:
        for pair in (True, False):
            V._PAIR_BWD = pair
            eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=3, layer_noise=0.0, dropout_rate=0.0, precision='fp32')
            res = eng.train_step(rI.cuda(), rS.cuda(), noise={}, drop={}, apply=False)
            torch.cuda.synchronize()
            grads[pair] = ({k: s.g.clone() for k, s in eng.stores.items()}, res)
    finally:
        V._PAIR_BWD = saved
    # The discriminators' sweeps are the same in both schedules: 1e-5 (float atomics).  A generator's gradient bucket is not
    # reproducible to better than ~4e-3 between two runs of the SAME schedule (measured: 1.5e-3 / 3.6e-3; the forward's striped
    # float atomics move the InstanceNorm statistics in the last bit, and ReLU masks / min-max arg-extrema of 60 chained layers
    # flip on that): the two schedules must agree at that level, 2e-2 and a cosine of 0.9998.
    for k in grads[True][0]:
        a, b = grads[True][0][k], grads[False][0][k]
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        print('%s: paired vs two sweeps rel L2 %.3e, cosine %.7f' % (k, rel, _cos(a, b)))
        if k.startswith('disc'):
            assert rel < 1e-4, (k, rel)
        else:
            assert rel < 2e-2 and _cos(a, b) > 0.9998, (k, rel, _cos(a, b))
    for k, v in grads[False][1].items():
        assert abs(grads[True][1][k] - v) <= 1e-4 * abs(v) + 1e-6, k
