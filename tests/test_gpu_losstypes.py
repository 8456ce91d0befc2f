"""Selectable cycle / adversarial loss types on the GPU (VanGan(cycle_loss_SIS=, cycle_loss_ISI=, gan_loss=), vg_lp_loss, vg_logit_loss;
DESIGN.md section 3.10), against the float64 restatement tests/loss_restate.py.

  kernels at true shapes      sums <= 1e-4 relative, gradients <= 1e-5 relative L2 against float64 -- the bounds
                              tests/test_gpu_calls.py::test_loss_chain_at_config_shapes applies to vg_mse / vg_mse_const; no element excluded
  full step, fp32 storage     the bounds of tests/test_gpu_fp32.py::_engine_fp32: outputs 2e-3 relative L2, the ten losses 2e-3 relative,
                              whole-network gradient cosine > 0.9995 (grad_report: per tensor 5e-2 / 0.999), weights after Adam
  full step, 64^3 batch 2     the comparison and bounds of tests/test_gpu_configs.py at that size (test_train_step_matches_fixture: exact-parity
                              engine, losses and fake_S 2e-3, gradient tensors cos > 0.9995 / rel 5e-2) on every tensor of all four networks,
                              with the bf16 engine beside it (test_full_size_properties: finite, losses 3e-2 + 1e-5 of the exact-parity run)
  test_step, replay, defaults see the tests

An 'mae' term's gradient is sign(cycled - real): the restatement takes that sign teacher-forced from the engine's own cycled volume
(loss_restate.cycle_loss); nothing is excluded or capped, and the share of voxels whose sign differs is printed."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_restate as R  # noqa: E402
from oracle import vangan_oracle as O  # noqa: E402
from test_gpu_nets import grad_report, perturb, rel_l2  # noqa: E402

DEV = 'cuda:0'
CONFIGS = [('mae', 'L4', None), ('mse', 'bce', 'bce'), ('L4', 'mae', 'bfce')]
IDS = ['mae-L4-lsgan', 'mse-bce-bce', 'L4-mae-bfce']
SHAPES = {'128^3 B1': (1, (128, 128, 128)), '64^3 B2': (2, (64, 64, 64)), '128x128x64 B2': (2, (128, 128, 64)), 'odd S B2': (2, (33, 35, 37))}


def _report(name, err):
    print('%-70s %s' % (name, '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))


def _sum_err(got, want):
    return abs(float(got) - float(want)) / (abs(float(want)) + 1e-30)


def _rel(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-30))


def _kw(cfg):
    return dict(cycle_loss_SIS=cfg[0], cycle_loss_ISI=cfg[1], gan_loss=cfg[2])


# ----------------------------------------------------------------------------------------------------------------------
# a. kernels at true shapes
# ----------------------------------------------------------------------------------------------------------------------
def _lp_case(a, b, ties, p, tag, err):
    """One (a, b) pair through vg_lp_loss: overwrite, accumulate, forward only; p = 2 beside vg_mse."""
    from van_gan_amd import ops
    dev = a.device
    gs = 0.37
    acc = torch.zeros(8, device=dev)
    g_set = torch.full_like(a, float('nan'))
    ops.lp_loss(a, b, p, acc[0:1], gs, g_set, accumulate=False)
    g0 = torch.randn(a.shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    g_acc = g0.clone()
    ops.lp_loss(a, b, p, acc[1:2], gs, g_acc, accumulate=True)
    ops.lp_loss(a, b, p, acc[2:3])                                    # gb = None
    torch.cuda.synchronize()
    d = b.double() - a.double()
    want = (d.abs() ** p).sum()
    gref = gs * p * d.abs() ** (p - 1) * torch.sign(d)
    err['%s p%d sum' % (tag, p)] = max(_sum_err(acc[i], want) for i in range(3))
    err['%s p%d grad' % (tag, p)] = _rel(g_set, gref)
    err['%s p%d grad+=' % (tag, p)] = _rel(g_acc, g0.double() + gref)
    assert torch.isfinite(g_set).all() and torch.isfinite(g_acc).all()
    assert float(g_set.flatten()[ties].abs().max()) == 0.0, (tag, p, 'a tie must give a gradient of exactly 0')
    assert torch.equal(g_acc.flatten()[ties], g0.flatten()[ties]), (tag, p)
    if p == 2:
        gm = torch.full_like(a, float('nan'))
        ops.mse(a, b, acc[3:4], gs, gm)
        torch.cuda.synchronize()
        err['%s p2 sum vs vg_mse' % tag] = _sum_err(acc[0], acc[3])
        err['%s p2 grad vs vg_mse' % tag] = _rel(g_set, gm.double())


@pytest.mark.parametrize('cfg', sorted(SHAPES))
def test_lp_loss_at_config_shapes(cfg):
    """vg_lp_loss, p = 1, 2, 4, on two [B][S] fp32 volumes with exact ties (first vector, middle, last elements = the scalar tail of an
    odd n); an odd S also runs on sample 1 alone: an unaligned start, so the scalar walk covers everything."""
    from van_gan_amd import ops
    dev = torch.device(DEV)
    B, (D, H, W) = SHAPES[cfg]
    S = D * H * W
    g = torch.Generator(device=dev).manual_seed(43)
    a, b = torch.randn(B, S, generator=g, device=dev), torch.randn(B, S, generator=g, device=dev)
    n = B * S
    ties = torch.tensor([0, 1, 5, n // 2, n // 2 + 3, S - 1, n - 3, n - 2, n - 1], device=dev)
    b.view(-1)[ties] = a.view(-1)[ties]
    err = {}
    for p in (1, 2, 4):
        _lp_case(a, b, ties, p, 'all', err)
    if S % 4:
        a1, b1 = a[1], b[1]
        assert a1.data_ptr() % 16 != 0
        t1 = torch.tensor([0, 2, S // 2, S - 2, S - 1], device=dev)
        b1[t1] = a1[t1]
        for p in (1, 2, 4):
            _lp_case(a1, b1, t1, p, 'unaligned', err)
    _report('vg_lp_loss ' + cfg, err)
    for k, v in err.items():
        assert v <= (1e-4 if 'sum' in k else 1e-5), (k, v)
    with pytest.raises(ops._lib.VgError):
        ops.lp_loss(a, b, 3, torch.zeros(1, device=dev))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n', [2 * 16 ** 3, 4 * 16 ** 3, 2 * 4 ** 3, 4 * 4 ** 3], ids=['2x16^3', '4x16^3', '2x4^3', '4x4^3'])
def test_logit_loss_at_config_shapes(n, dtype):
    """vg_logit_loss on the patch logits of the configurations (2B * 16^3 at 128^3, 2B * 4^3 at 32^3; B = 1, 2), fp32 and 16-bit storage,
    N(0, 3) with values at +-80, both kinds, both targets, overwrite / accumulate / forward only; and on the slice [3:] -- an unaligned
    start and a tail.  Reference: float64 autograd through loss_restate on the values the kernel read."""
    from van_gan_amd import ops
    dev = torch.device(DEV)
    g = torch.Generator(device=dev).manual_seed(44)
    x = (torch.randn(n, generator=g, device=dev) * 3.0)
    x[torch.tensor([0, 7, n // 2, n - 1], device=dev)] = 80.0
    x[torch.tensor([3, 8, n // 2 + 1, n - 2], device=dev)] = -80.0
    x = x.to(dtype)
    gs = 0.61
    err = {}
    for tag, xv in (('all', x), ('slice', x[3:])):
        for kind, f in ((ops.LOGIT_BCE, R.bce_logits), (ops.LOGIT_FOCAL, R.focal_logits)):
            for z in (1.0, 0.0):
                acc = torch.zeros(4, device=dev)
                g_set = torch.full((xv.numel(),), float('nan'), device=dev)
                ops.logit_loss(xv, z, kind, acc[0:1], gs, g_set)
                g0 = torch.randn(xv.numel(), generator=g, device=dev)
                g_acc = g0.clone()
                ops.logit_loss(xv, z, kind, acc[1:2], gs, g_acc, accumulate=True)
                ops.logit_loss(xv, z, kind, acc[2:3])
                torch.cuda.synchronize()
                xr = xv.double().requires_grad_(True)
                want = f(torch.full_like(xr, z).unsqueeze(-1), xr.unsqueeze(-1)).sum()
                (gs * want).backward()
                k = '%s %s z%d' % (tag, 'bce' if kind == ops.LOGIT_BCE else 'bfce', int(z))
                assert torch.isfinite(acc).all() and torch.isfinite(g_set).all() and torch.isfinite(g_acc).all(), k
                err[k + ' sum'] = max(_sum_err(acc[i], want.detach()) for i in range(3))
                err[k + ' grad'] = _rel(g_set, xr.grad)
                err[k + ' grad+='] = _rel(g_acc, g0.double() + xr.grad)
    _report('vg_logit_loss n %d %s' % (n, str(dtype)[6:]), err)
    for k, v in err.items():
        assert v <= (1e-4 if 'sum' in k else 1e-5), (k, v)
    for bad in (dict(target=0.5, kind=0), dict(target=1.0, kind=2)):
        with pytest.raises(ops._lib.VgError):
            ops.logit_loss(x, bad['target'], bad['kind'], torch.zeros(1, device=dev))


# ----------------------------------------------------------------------------------------------------------------------
# b. full step, exact-parity engine
# ----------------------------------------------------------------------------------------------------------------------
def _teacher(eng, cfg, rI, rS):
    """The engine's own cycled volumes for the 'mae' terms of this configuration (loss_restate.cycle_loss)."""
    t = {}
    if cfg[0] == 'mae':
        t['cycled_S'] = eng._aux['cycled_S'].double().cpu()
    if cfg[1] == 'mae':
        t['cycled_I'] = eng._aux['cycled_I'].double().cpu()
    return t


def _sign_share(cfg, teacher, aux, rI, rS):
    for i, (key, real) in enumerate((('cycled_S', rS), ('cycled_I', rI))):
        if cfg[i] == 'mae':
            a, b = torch.sign(teacher[key] - real.double()), torch.sign(aux[key].double() - real.double())
            print('   mae on %s: sign(cycled - real) differs between the engine and the restatement at %.4f %% of the voxels'
                  % (key, 100.0 * float((a != b).double().mean())))


def _engine_fp32(dims, B, cfg):
    from van_gan_amd import VanGan
    dev = torch.device(DEV)
    eng = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32', **_kw(cfg))
    P = {k: perturb(v, 40 + i) for i, (k, v) in enumerate(O.make_models(0).items())}
    eng.load_weights(P)
    rI, rS = O.synth_volumes(B, *dims, seed=1234)
    res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={})
    teacher = _teacher(eng, cfg, rI, rS)
    Pd = {k: {n: t.double() for n, t in v.items()} for k, v in P.items()}
    ref, grads, aux = R.train_step(Pd, {}, rI.double(), rS.double(), O.Cfg(B, 1), teacher=teacher, **_kw(cfg))
    _sign_share(cfg, teacher, aux, rI, rS)
    for k in O.RESULT_KEYS:
        print('   %-24s hip %.6f  restatement %.6f  rel %.2e' % (k, res[k], ref[k], abs(res[k] - ref[k]) / (abs(ref[k]) + 1e-30)))
    for k in ('fake_S', 'fake_I', 'cycled_S', 'cycled_I'):
        r = rel_l2(eng._aux[k], aux[k])
        print('   %-10s rel l2 %.3e' % (k, r))
        assert r < 2e-3, k
    for k in O.RESULT_KEYS:
        assert abs(res[k] - ref[k]) <= 2e-3 * abs(ref[k]) + 1e-6, k
    got = eng.export_grads()
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        cos = grad_report(got[net], grads[net], '%s fp32 %s' % (net, cfg), rel_tol=5e-2, cos_tol=0.999)
        assert cos > 0.9995, (net, cos)
    W = eng.export_weights()
    nbad = ntot = 0
    for net in W:
        for n in W[net]:
            d = (W[net][n].double() - Pd[net][n]).abs()
            nbad += int((d > 1e-4).sum()); ntot += d.numel()
    print('   weights after Adam: %d / %d elements differ by > 1e-4 (|step| <= 6.3e-4)' % (nbad, ntot))
    assert nbad <= 2e-3 * ntot


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_train_step_fp32_32(cfg, B):
    _engine_fp32((32, 32, 32), B, cfg)


# ----------------------------------------------------------------------------------------------------------------------
# c. product path
# ----------------------------------------------------------------------------------------------------------------------
FIXTURE_GRADS = (('gen_IS', 'stem.conv1.w'), ('gen_IS', 'out.w'), ('gen_SI', 'dec0.cb1.conv.w'), ('disc_I', 'conv0.w'), ('disc_S', 'out.w'))


@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_train_step_64_b2(cfg):
    """64^3 batch 2, each configuration, by the comparison tests/test_gpu_configs.py::test_train_step_matches_fixture applies to the default
    configuration at this size -- the exact-parity engine (fp32 storage), weights O.make_models(seed), train_step(apply=False), against the
    float64 reference (there a committed fixture of the oracle; here the restatement, computed in the test, 'mae' sign teacher-forced
    from the engine's cycled volume):
        the ten losses                      2e-3 * |ref| + 1e-6        (test_train_step_matches_fixture)
        fake_S[0]                           2e-3 relative L2           (test_train_step_matches_fixture)
        the five tensors the fixture holds  cos > 0.9995, rel < 5e-2   (test_train_step_matches_fixture)
        EVERY tensor of all four networks   grad_report at rel 5e-2 / cos 0.999, whole network cos > 0.9995
                                            (tests/test_gpu_fp32.py::_engine_fp32; tensors below 1e-2 of the largest norm: absolute, as there)
    -- the new branches act on the generators' gradients (the direct add into d cycled_S, the BCE term in g_ncI, the scales), which this
    asserts.  Beside it the product engine (bf16 storage) on the same weights and inputs, by the comparison test_gpu_configs.py applies to
    a bf16 engine (test_full_size_properties): finite, losses within 3e-2 * |fp32-mode| + 1e-5 of the exact-parity engine's; its
    whole-network gradient cosines against the reference are printed (the project states no bound for bf16 gradients against an
    unrounded reference)."""
    from van_gan_amd import VanGan
    dev = torch.device(DEV)
    dims, B = (64, 64, 64), 2
    P = O.make_models(0)
    rI, rS = O.synth_volumes(B, *dims, seed=4321)
    eng = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32', **_kw(cfg))
    eng.load_weights(P)
    res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={}, apply=False)
    teacher = _teacher(eng, cfg, rI, rS)
    Pd = {k: {n: t.double() for n, t in v.items()} for k, v in P.items()}
    ref, grads, aux = R.train_step(Pd, {}, rI.double(), rS.double(), O.Cfg(B, 1), apply=False, teacher=teacher, **_kw(cfg))
    _sign_share(cfg, teacher, aux, rI, rS)
    for k in O.RESULT_KEYS:
        print('   %-24s hip %.6f  restatement %.6f  rel %.2e' % (k, res[k], ref[k], abs(res[k] - ref[k]) / (abs(ref[k]) + 1e-30)))
    for k in ('fake_S', 'fake_I', 'cycled_S', 'cycled_I'):
        print('   %-10s rel l2 %.3e' % (k, rel_l2(eng._aux[k], aux[k])))
    got = eng.export_grads()
    outs = rel_l2(eng._aux['fake_S'][0], aux['fake_S'][0])
    cos_all = {}
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        cos_all[net] = grad_report(got[net], grads[net], '%s fp32 64^3 b2 %s' % (net, cfg), rel_tol=5e-2, cos_tol=0.999, check=False)
    for net, name in FIXTURE_GRADS:
        g, r = got[net][name].double().cpu().flatten(), grads[net][name].double().flatten()
        c, rl = float(g @ r / (g.norm() * r.norm() + 1e-300)), float((g - r).norm() / (r.norm() + 1e-300))
        print('   %-28s cos %.6f rel %.2e' % (net + '/' + name, c, rl))
    # the product engine beside it
    del eng
    torch.cuda.empty_cache()
    eb = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.0, **_kw(cfg))
    eb.load_weights(P)
    rb = eb.train_step(rI.to(dev), rS.to(dev), noise={}, drop={}, apply=False)
    gb = eb.export_grads()
    for k in O.RESULT_KEYS:
        print('   %-24s bf16 %.6f  fp32-mode %.6f' % (k, rb[k], res[k]))
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        grad_report(gb[net], grads[net], '%s bf16 64^3 b2 %s (printed only)' % (net, cfg), check=False)
    # ---- assertions (after every figure is printed) ----
    for k in O.RESULT_KEYS:
        assert abs(res[k] - ref[k]) <= 2e-3 * abs(ref[k]) + 1e-6, k
    assert outs < 2e-3, outs
    for net, name in FIXTURE_GRADS:
        g, r = got[net][name].double().cpu().flatten(), grads[net][name].double().flatten()
        c, rl = float(g @ r / (g.norm() * r.norm() + 1e-300)), float((g - r).norm() / (r.norm() + 1e-300))
        assert c > 0.9995 and rl < 5e-2, (net, name, c, rl)
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        grad_report(got[net], grads[net], '%s fp32 64^3 b2 %s' % (net, cfg), rel_tol=5e-2, cos_tol=0.999)
        assert cos_all[net] > 0.9995, (net, cos_all[net])
    assert all(math.isfinite(v) for v in rb.values()), rb
    for k in O.RESULT_KEYS:
        assert abs(rb[k] - res[k]) <= 3e-2 * abs(res[k]) + 1e-5, k


# ----------------------------------------------------------------------------------------------------------------------
# d. test_step; the other engine variants
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', [dict(), dict(generator='resnet'), dict(spectral_norm=True), dict(attention_gate=True)],
                         ids=['resUnet', 'resnet', 'spectral_norm', 'attention_gate'])
@pytest.mark.parametrize('cfg', CONFIGS, ids=IDS)
def test_test_step_is_the_forward_of_a_train_step(cfg, variant):
    """test_step (training=False) returns the forward losses of train_step(apply=False) with noise and dropout off on the same inputs --
    the forward-only launches of the selected terms (gb == NULL) against the ones that also write gradients -- for the plain engine and
    with generator='resnet', spectral_norm, attention_gate; fp32 storage: the two differ by the order of float atomics (1e-4, the bound
    tests/test_gpu_fp32.py::test_stream_schedule_does_not_change_gradients puts on losses of two runs).  (spectral_norm: the train step
    projects the wrapped kernels in place before its discriminators run and test_step never projects -- it reads the kernels that step
    left, the ones its forward used.)"""
    from van_gan_amd import VanGan
    dims, B = (32, 32, 32), 2
    eng = VanGan(dims, batch_size=B, device=DEV, seed=3, layer_noise=0.0, dropout_rate=0.0, precision='fp32', **variant, **_kw(cfg))
    rI, rS = O.synth_volumes(B, *dims, seed=99)
    rI, rS = rI.to(DEV), rS.to(DEV)
    tr = eng.train_step(rI, rS, noise={}, drop={}, apply=False)
    te = eng.test_step(rI, rS)
    tol = 1e-4
    for k in O.RESULT_KEYS:
        print('   %-24s train %.6f  test %.6f' % (k, tr[k], te[k]))
        assert math.isfinite(te[k]) and abs(tr[k] - te[k]) <= tol * abs(tr[k]) + 1e-6, (k, tr[k], te[k])
    g = eng.export_grads()
    for net in g:
        assert all(torch.isfinite(t).all() for t in g[net].values()), net


def test_test_step_matches_the_restatement_bf16():
    from van_gan_amd import VanGan
    dims, B = (32, 32, 32), 1
    cfg = CONFIGS[2]
    eng = VanGan(dims, batch_size=B, device=DEV, seed=3, **_kw(cfg))
    P = eng.export_weights()
    rI, rS = O.synth_volumes(B, *dims, seed=99)
    res = eng.test_step(rI.to(DEV), rS.to(DEV))
    ref = R.test_step(P, rI, rS, O.Cfg(B, 1), q=O.bf16_round, **_kw(cfg))
    for k in O.RESULT_KEYS:
        print('   %-24s hip %.6f  restatement %.6f' % (k, res[k], ref[k]))
        assert abs(res[k] - ref[k]) <= 3e-2 * abs(ref[k]) + 1e-4, (k, res[k], ref[k])       # tests/test_gpu_nets.py::test_test_step_matches_forward_losses


# ----------------------------------------------------------------------------------------------------------------------
# e. replay
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['replay', 'graph'])
def test_recorded_step_equals_eager(mode):
    """('mae', 'bce', 'bfce') -- the raw-volume term behind the min-max backward, the BCE term inside the SSIM block, vg_logit_loss --
    through train_step_replay and train_step_graph against the eager step, at the bounds of tests/test_gpu_graph.py (fp32 storage,
    learning rate 0: losses 2e-5, whole-network gradients cos > 0.9999 / rel < 1e-2).  The scales are constants of the engine: nothing
    new is bound per step."""
    from test_gpu_graph import _grads_agree, _pair
    from van_gan_amd.vangan import RESULT_KEYS
    eager, other, rI, rS = _pair('fp32', cycle_loss_SIS='mae', cycle_loss_ISI='bce', gan_loss='bfce')
    if mode == 'graph':
        other.capture_train_step()
    for e in (eager, other):
        e.lr = 0.0
    for step in range(3):
        x, y = (rI, rS) if step % 2 == 0 else (rI.flip(1).contiguous(), rS.flip(2).contiguous())
        re = eager.train_step(x, y)
        ro = other.train_step_replay(x, y) if mode == 'replay' else other.train_step_graph(x, y)
        for k in RESULT_KEYS:
            print('   step %d %-24s eager %.6f  %s %.6f' % (step, k, re[k], mode, ro[k]))
            assert abs(re[k] - ro[k]) <= 2e-5 * abs(re[k]) + 1e-7, (step, k, re[k], ro[k])
        assert other.rng_offset == eager.rng_offset
        _grads_agree(eager, other, '%s step %d' % (mode, step))
    if mode == 'replay':
        names = [getattr(f, '__name__', '') for f, _ in other._rlist]
        assert names.count('vg_lp_loss') == 1 and names.count('vg_logit_loss') == 6 and names.count('vg_bce') == 1
        assert 'vg_mse' not in names and 'vg_mse_const' not in names


# ----------------------------------------------------------------------------------------------------------------------
# the data-parallel path
# ----------------------------------------------------------------------------------------------------------------------
DDP_WORKER = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from van_gan_amd.vangan import VanGan
from oracle.vangan_oracle import synth_volumes
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
torch.cuda.set_device('cuda:0')
dist.init_process_group('gloo', rank=rank, world_size=world)
eng = VanGan(%(dims)r, batch_size=1, n_devices=world, device='cuda:0', seed=rank * 17, layer_noise=0.0, dropout_rate=0.0,
             process_group=dist.group.WORLD, precision='fp32', **%(kw)r)
eng.broadcast_weights(0)
rI, rS = synth_volumes(2, *%(dims)r, seed=5)
res = eng.distributed_train_step(rI[rank:rank + 1].to('cuda:0'), rS[rank:rank + 1].to('cuda:0'))
torch.cuda.synchronize()
torch.save({'w': {k: s.w.cpu() for k, s in eng.stores.items()}, 'res': res}, %(out)r %% rank)
dist.destroy_process_group()
"""


def test_two_ranks_run_the_selected_losses(tmp_path):
    """('mae', 'bce', 'bfce') under world_size 2 (gloo, both ranks on cuda:0), by tests/test_gpu_ddp.py's comparison and bounds: both
    ranks end with identical weights and result dictionaries; against the same engine run as 'rank r of 2' without a process group
    (n_devices=2, gradients summed by hand, one Adam step): summed losses 1e-4, <= 0.2 % of the weights differ by more than 1e-4."""
    import os
    import subprocess
    import sys
    from test_gpu_ddp import DIMS, ROOT, _free_port
    from van_gan_amd.vangan import VanGan
    kw = dict(cycle_loss_SIS='mae', cycle_loss_ISI='bce', gan_loss='bfce')
    out = str(tmp_path / 'rank%d.pt')
    script = tmp_path / 'worker.py'
    script.write_text(DDP_WORKER % dict(root=ROOT, dims=DIMS, out=out, kw=kw))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill(); o, _ = p.communicate()
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), '\n'.join(logs)
    a, b = torch.load(out % 0), torch.load(out % 1)
    for k in a['w']:
        assert torch.equal(a['w'][k], b['w'][k]), k
    assert a['res'] == b['res']
    eng = VanGan(DIMS, batch_size=1, n_devices=2, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32', **kw)
    rI, rS = O.synth_volumes(2, *DIMS, seed=5)
    gsum, rsum = None, None
    for r in range(2):
        res = eng.train_step(rI[r:r + 1].cuda(), rS[r:r + 1].cuda(), apply=False)
        g = {k: s.g.clone() for k, s in eng.stores.items()}
        gsum = g if gsum is None else {k: gsum[k] + g[k] for k in g}
        rsum = res if rsum is None else {k: rsum[k] + res[k] for k in res}
    for k, s in eng.stores.items():
        s.g.copy_(gsum[k])
    eng._apply_adam()
    torch.cuda.synchronize()
    for k, v in rsum.items():
        print('   %-24s two ranks %.6f  by hand %.6f' % (k, a['res'][k], v))
        assert abs(a['res'][k] - v) <= 1e-4 * abs(v) + 1e-6, (k, a['res'][k], v)
    bad = tot = 0
    for k, s in eng.stores.items():
        d = (s.w.cpu() - a['w'][k]).abs()
        bad += int((d > 1e-4).sum()); tot += d.numel()
    print('   weights after Adam: %d / %d differ by > 1e-4' % (bad, tot))
    assert bad <= 2e-3 * tot, (bad, tot)


# ----------------------------------------------------------------------------------------------------------------------
# f. defaults
# ----------------------------------------------------------------------------------------------------------------------
def test_default_values_leave_the_launch_list_alone():
    """An engine built with the default loss types passed explicitly records the launch list of one built without them: same length,
    same entry points in the same order, none of the new ones."""
    from van_gan_amd import VanGan
    from van_gan_amd.synth import synth_volumes
    dims, B = (32, 32, 32), 1
    rI, rS = synth_volumes(B, *dims, seed=7)
    lists = []
    for kw in (dict(), dict(cycle_loss_SIS='bce', cycle_loss_ISI='mse', gan_loss=None)):
        eng = VanGan(dims, batch_size=B, device=DEV, seed=3, **kw)
        eng.train_step_replay(rI.to(DEV), rS.to(DEV))
        lists.append([getattr(f, '__name__', repr(f)) for f, _ in eng._rlist])
    assert len(lists[0]) == len(lists[1]) > 500
    assert lists[0] == lists[1]
    assert 'vg_lp_loss' not in lists[0] and 'vg_logit_loss' not in lists[0]
    assert lists[0].count('vg_mse') == 1 and lists[0].count('vg_mse_const') == 6 and lists[0].count('vg_bce') == 1


def test_engine_rejects_unknown_loss_types():
    from van_gan_amd import VanGan
    for bad in (dict(cycle_loss_SIS='l1'), dict(cycle_loss_ISI='huber'), dict(gan_loss='hinge'), dict(gan_loss='bce', wasserstein=True)):
        with pytest.raises(ValueError):
            VanGan((32, 32, 32), batch_size=1, device=DEV, **bad)
