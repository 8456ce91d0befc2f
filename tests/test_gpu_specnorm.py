"""GPU: spectrally normalised discriminators (VanGan(spectral_norm=True), compat use_SN=True) -- the vg_spectral_norm kernel at the four
true shapes, PatchGAN(spectral_norm=True) against torch autograd through the restated network, the engine's train step (projection
placement, losses, gradients, stale-pack / stale-u over two applied steps, checkpoint, graph entry points), the convergence property
of the power iteration over ten steps, and the product path through the reference-shaped constructor.

The reference of every comparison is tests/sn_restate.py (float64; TensorFlow Addons' semantics restated, TP).  Bounds:
  kernel, fp32         : sigma relative error, rel_l2(u'), rel_l2(W / sigma) <= 5e-5 -- the project's bound for fp32 discriminator
                         contractions (tests/test_gpu_wasserstein.py); worst-case blocked summation at K = 16384:
                         ~73 roundings x 2^-24 x a cancellation ratio of ~12.
  network, fp32        : logits 2e-3, per-tensor gradients 5e-2 / cos 0.999 (tests/test_gpu_fp32.py, as test_gpu_wasserstein.py quotes them)
  network, bf16        : logits 2e-2, dx 8e-2, grad_report defaults (tests/test_gpu_nets.py)
  engine losses, fp32  : 2e-3 |ref| + 1e-6 (tests/test_gpu_wasserstein.py)
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vangan_oracle as O  # noqa: E402
import sn_restate as R  # noqa: E402
from test_gpu_nets import grad_report, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
DROP_CH = (('down0', 128), ('down1', 256), ('down2', 512))


def _table(Ws, us):
    from van_gan_amd import ops
    ops.set_device(0)
    return ops.SpecNormTable(Ws, us, torch.device(DEV))


def _inputs(dev=DEV):
    Ws, us = [], []
    for i, (K, C_) in enumerate(R.SHAPES):
        W, u = R.he_normal(K, C_, 100 + i)
        Ws.append(W); us.append(u)
    return Ws, us


@pytest.mark.parametrize('n', [1, 2])
def test_kernel_matches_float64_at_the_true_shapes(n):
    Ws, us = _inputs()
    dW, du = [w.to(DEV) for w in Ws], [u.to(DEV) for u in us]
    tab = _table(dW, du)
    tab.run(n)
    torch.cuda.synchronize()
    state = tab.state.cpu().double()
    for i, (W, u) in enumerate(zip(Ws, us)):
        Wr, ur = W.double().numpy(), u.double().numpy()
        sig = []
        for _ in range(n):
            Wr, ur, s = R.project(Wr, ur)
            sig.append(s)
        es = max(abs(float(state[i, p]) - sig[p]) / sig[p] for p in range(n))
        eu, ew = rel_l2(du[i], torch.from_numpy(ur)), rel_l2(dW[i], torch.from_numpy(Wr))
        print('vg_spectral_norm n=%d %5dx%-3d sigma %s  rel err sigma %.2e  u %.2e  W %.2e' % (n, W.shape[0], W.shape[1],
                                                                                             ['%.4f' % s for s in sig], es, eu, ew))
        assert es <= 5e-5 and eu <= 5e-5 and ew <= 5e-5, (W.shape, es, eu, ew)
        assert float(state[i, 0]) > 0 and abs(float(state[i, 4]) * float(np.prod(sig)) - 1.0) < 1e-4


def test_kernel_is_bit_reproducible_and_survives_zero_weights():
    Ws, us = _inputs()
    outs = []
    for _ in range(2):
        dW, du = [w.to(DEV) for w in Ws], [u.to(DEV) for u in us]
        tab = _table(dW, du)
        tab.run(2)
        torch.cuda.synchronize()
        outs.append((dW, du, tab.state.clone()))
    for a, b in zip(outs[0][0] + outs[0][1] + [outs[0][2]], outs[1][0] + outs[1][1] + [outs[1][2]]):
        assert torch.equal(a, b)
    # all-zero kernels (one of them beside a regular one): no NaN / Inf, W and u stay as they are, sigma reads 0
    dW = [torch.zeros(K, C_, device=DEV) for K, C_ in R.SHAPES[:3]] + [Ws[3].to(DEV)]
    du = [u.to(DEV) for u in us]
    tab = _table(dW, du)
    tab.run(2)
    torch.cuda.synchronize()
    for i in range(3):
        assert not dW[i].any() and torch.equal(du[i].cpu(), us[i]) and float(tab.state[i, 0]) == 0.0 and float(tab.state[i, 1]) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in dW + du + [tab.state])
    assert torch.equal(dW[3], outs[0][0][3]) and torch.equal(du[3], outs[0][1][3])


def _sn_params(seed, wasserstein_patches=0):
    """he_normal kernels / TruncatedNormal u of the SN discriminator (the engine's initialiser), biases moved off zero."""
    from van_gan_amd.nets import ParamStore, disc_param_specs, init_reference
    st = ParamStore(disc_param_specs(wasserstein_patches, True), 'cpu')
    init_reference(st, seed)
    P = st.export()
    g = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith('.b'):
            P[k].add_(torch.randn(P[k].shape, generator=g) * 0.1)
    return P


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_sn_discriminator_forward_backward_32(precision):
    from van_gan_amd.nets import ParamStore, PatchGAN, disc_param_specs
    from van_gan_amd.ops import Arena
    dev = torch.device(DEV)
    dims, N = (32, 32, 32), 2
    f32 = precision == 'fp32'
    P = _sn_params(21)
    st = ParamStore(disc_param_specs(spectral_norm=True), dev)
    st.load(P)
    net = PatchGAN(st, dims, torch.float32 if f32 else torch.bfloat16, spectral_norm=True)
    net.pack()
    ar = Arena(1 << 30, dev)
    x, _ = O.synth_volumes(N, *dims, seed=6)
    g = torch.Generator().manual_seed(4)
    noise = {k: (torch.randn(shp, generator=g) * 0.1).to(torch.bfloat16) for k, shp in net.noise_shapes(N).items()}
    drop = {k: ((torch.rand(N, c, generator=g) > 0.2).float() / 0.8) for k, c in DROP_CH}
    logits = torch.zeros(N, 4, 4, 4, 1, device=dev)
    nz_dev = {k: v.to(dev) for k, v in noise.items()}          # noise tensors are 16-bit in both storage modes
    ctx = net.forward(ar, x.to(dev), logits, nz_dev, {k: v.to(dev) for k, v in drop.items()})
    torch.cuda.synchronize()
    train = [k for k in P if not k.endswith('sn_u')]
    cast = (lambda t: t.double()) if f32 else (lambda t: t.clone())
    Pr = {k: cast(P[k]).requires_grad_(True) for k in train}
    xr = cast(x).requires_grad_(True)
    lr_ = R.disc_forward(Pr, xr, {k: cast(v.float()) for k, v in noise.items()}, {k: cast(v) for k, v in drop.items()},
                         q=None if f32 else O.bf16_round)
    e = rel_l2(logits, lr_.detach())
    print('SN disc %s logits rel l2 %.3e' % (precision, e))
    assert e < (2e-3 if f32 else 2e-2)
    gl = torch.randn(logits.shape, generator=g)
    (lr_ * cast(gl)).sum().backward()
    st.g.zero_()
    dx = torch.zeros(N, *dims, 1, device=dev)
    net.backward(ar, ctx, gl.to(dev), 0, N, wgrad=True, dx=dx)
    torch.cuda.synchronize()
    kw = dict(rel_tol=5e-2, cos_tol=0.999) if f32 else {}
    grad_report(st.export(st.g), {k: v.grad for k, v in Pr.items()}, 'SN discriminator ' + precision, **kw)
    e = rel_l2(dx, xr.grad)
    print('SN disc %s input gradient rel l2 %.3e' % (precision, e))
    assert e < (5e-2 if f32 else 8e-2)
    before = st.g.clone()
    dx1 = torch.zeros(1, *dims, 1, device=dev)
    net.backward(ar, ctx, gl[1:].to(dev), 1, 2, wgrad=False, dx=dx1)
    torch.cuda.synchronize()
    assert torch.equal(before, st.g)
    assert rel_l2(dx1, xr.grad[1:]) < (5e-2 if f32 else 8e-2)
    # project() repacks: the forward behind it runs on W / sigma, not on the operands packed before
    net.project(2)
    logits2 = torch.zeros_like(logits)
    net.forward(ar, x.to(dev), logits2, nz_dev, {k: v.to(dev) for k, v in drop.items()})
    torch.cuda.synchronize()
    P2, sig = R.project_params(P, 2)
    with torch.no_grad():
        q2 = None if f32 else O.bf16_round
        ref2 = R.disc_forward({k: (P2[k] if f32 else P2[k].float()) for k in train}, cast(x), {k: cast(v.float()) for k, v in noise.items()},
                              {k: cast(v) for k, v in drop.items()}, q=q2)
    e2 = rel_l2(logits2, ref2)
    print('SN disc %s logits after project(2) rel l2 %.3e (stale operands would give %.3e)' % (precision, e2, rel_l2(logits, ref2)))
    assert e2 < (2e-3 if f32 else 2e-2) and rel_l2(logits, ref2) > 0.1
    assert max(abs(float(net.sn_sigma()[i, p]) - sig[k][p]) / sig[k][p] for i, k in enumerate(R.WRAPPED) for p in range(2)) <= 5e-5


def _masks(B, n_head, g, dev):
    """explicit dropout multipliers per discriminator over [real; fake] for the engine, and their halves for the restatement"""
    eng, ref = {}, {}
    for d in ('S', 'I'):
        dp = {k: (torch.rand(2 * B, c, generator=g) >= 0.2).float() / 0.8 for k, c in DROP_CH}
        if n_head:
            dp['head'] = (torch.rand(2 * B, n_head, generator=g) >= 0.2).float() / 0.8
        eng[d] = {k: t.to(dev) for k, t in dp.items()}
        ref[d] = ({k: t[:B].double() for k, t in dp.items()}, {k: t[B:].double() for k, t in dp.items()})
    return eng, ref


def _engine(B, wasserstein=False, **kw):
    from van_gan_amd import VanGan
    extra = dict(wasserstein=True, lr=1e-4, beta_1=0.0, beta_2=0.9, clipnorm=0.0) if wasserstein else {}
    extra.update(kw)
    return VanGan((32, 32, 32), batch_size=B, n_devices=1, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.2, precision='fp32',
                  spectral_norm=True, **extra)


@pytest.mark.parametrize('B,wasserstein', [(1, False), (2, False), (1, True)])
def test_engine_step_projects_twice_and_matches_the_restated_losses(B, wasserstein):
    dev = torch.device(DEV)
    dims = (32, 32, 32)
    eng = _engine(B, wasserstein)
    P = eng.export_weights()
    assert all((k + '.sn_u') in P[d] for d in ('disc_S', 'disc_I') for k in R.WRAPPED) and not [k for k in P['disc_S'] if '.in.' in k]
    rI, rS = O.synth_volumes(B, *dims, seed=21)
    masks, rmasks = _masks(B, 64 if wasserstein else 0, torch.Generator().manual_seed(9), dev)
    res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop=masks, apply=False)
    torch.cuda.synchronize()
    grads = eng.export_grads()
    W = eng.export_weights()
    fake = {'S': eng.generate('gen_IS', rI.to(dev)).cpu().double(), 'I': eng.generate('gen_SI', rS.to(dev)).cpu().double()}
    real = {'S': rS.double(), 'I': rI.double()}
    for net in ('gen_IS', 'gen_SI'):
        assert all(torch.equal(W[net][k], P[net][k]) for k in P[net])
    for d in ('S', 'I'):
        net = 'disc_' + d
        P2, sig = R.project_params(P[net], 2)
        for k in R.WRAPPED:
            ew, eu = rel_l2(W[net][k + '.w'], P2[k + '.w']), rel_l2(W[net][k + '.sn_u'], P2[k + '.sn_u'])
            print('%s %s after the step: W %.2e u %.2e (sigma %.4f, %.4f)' % (net, k, ew, eu, sig[k][0], sig[k][1]))
            assert ew <= 5e-5 and eu <= 5e-5
        for k in P[net]:
            if k.split('.')[0] not in R.WRAPPED or k.endswith('.b'):
                assert torch.equal(W[net][k], P[net][k]), k          # out.w, the biases, the Dense head: bit-unchanged
        train = {k: v.clone().requires_grad_(True) for k, v in P2.items() if not k.endswith('sn_u')}
        d_real = R.disc_forward(train, real[d], None, rmasks[d][0])
        d_fake = R.disc_forward(train, fake[d], None, rmasks[d][1])
        dl, gl = R.disc_losses(d_real, d_fake, float(B), wasserstein)
        for key, ref in (('D_%s_loss' % d, float(dl.detach())), ('gen_%s_loss' % ('IS' if d == 'S' else 'SI'), float(gl.detach()))):
            print('   %-14s hip %.6f  restated %.6f' % (key, res[key], ref))
            assert abs(res[key] - ref) <= 2e-3 * abs(ref) + 1e-6, key
        if not wasserstein:
            names = list(train)
            gs = torch.autograd.grad(dl, [train[n] for n in names])
            grad_report(grads[net], dict(zip(names, gs)), net + ' (spectral norm) fp32', rel_tol=5e-2, cos_tol=0.999)
            assert set(grads[net]) == set(names)


def test_engine_two_applied_steps_test_step_checkpoint_and_graph(tmp_path):
    """The second step's projection must start from the first step's Adam-updated kernels and updated u (stale pack / stale u), followed
    with the restatement driven by the engine's own exported gradients.  Bound: two steps, each a pair of projections within the 5e-5
    of the kernel test plus an elementwise fp32 Adam update of identical gradients (relative error ~1e-7 of a 2e-4 step): 1e-4."""
    from van_gan_amd import VanGan
    dev = torch.device(DEV)
    B, dims = 1, (32, 32, 32)
    eng = _engine(B, output_dir=str(tmp_path))
    P = eng.export_weights()
    ref = {d: {k: v.double().clone() for k, v in P[d].items()} for d in ('disc_S', 'disc_I')}
    opt = {'disc_S': {}, 'disc_I': {}}
    rI, rS = O.synth_volumes(B, *dims, seed=21)
    g = torch.Generator().manual_seed(9)
    for step in range(2):
        masks, _ = _masks(B, 0, g, dev)
        eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop=masks, apply=True)
        grads = eng.export_grads()
        for d in ref:
            ref[d], _ = R.project_params(ref[d], 2)
            train = {k: v for k, v in ref[d].items() if not k.endswith('sn_u')}
            O.adam_step(train, {k: grads[d][k].double() for k in train}, opt[d])
    W = eng.export_weights()
    for d in ref:
        for k in R.WRAPPED:
            ew, eu = rel_l2(W[d][k + '.w'], ref[d][k + '.w']), rel_l2(W[d][k + '.sn_u'], ref[d][k + '.sn_u'])
            print('%s %s after two applied steps: W %.2e u %.2e' % (d, k, ew, eu))
            assert ew <= 1e-4 and eu <= 1e-4
            assert rel_l2(W[d][k + '.w'], P[d][k + '.w']) > 0.1
    # test_step never projects
    eng.test_step(rI.to(dev), rS.to(dev))
    W2 = eng.export_weights()
    assert all(torch.equal(W2[d][k], W[d][k]) for d in W for k in W[d])
    # checkpoint round trip restores sn_u; a checkpoint of the other configuration is refused as a whole
    eng.save_checkpoint(0)
    eng.train_step(rI.to(dev), rS.to(dev), apply=True)
    assert not torch.equal(eng.export_weights()['disc_S']['down2.sn_u'], W['disc_S']['down2.sn_u'])
    assert eng.load_checkpoint(1)
    W3 = eng.export_weights()
    assert all(torch.equal(W3[d][k], W[d][k]) for d in W for k in W[d])
    plain = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, precision='fp32', output_dir=str(tmp_path / 'plain'))
    before = plain.export_weights()
    with pytest.raises(ValueError, match='spectral normalisation'):
        plain.load_checkpoint(1, newpath=eng.checkpoint_dir)
    after = plain.export_weights()
    assert all(torch.equal(before[d][k], after[d][k]) for d in before for k in before[d])
    plain.save_checkpoint(0)
    with pytest.raises(ValueError, match='spectral normalisation'):
        eng.load_checkpoint(1, newpath=plain.checkpoint_dir)
    # a captured / recorded step would have to carry the projection: not built, and loud about it
    for fn in (eng.capture_train_step, lambda: eng.train_step_graph(rI.to(dev), rS.to(dev)), lambda: eng.train_step_replay(rI.to(dev), rS.to(dev))):
        with pytest.raises(NotImplementedError):
            fn()


def test_power_iteration_converges_over_ten_steps():
    """Ten train_step(apply=False) calls = 20 projections, no Adam.  The estimate is a lower bound of the true norm, so the top singular
    value of W / sigma never falls below 1 and never grows."""
    dev = torch.device(DEV)
    B, dims = 1, (32, 32, 32)
    eng = _engine(B)
    rI, rS = O.synth_volumes(B, *dims, seed=21)
    tops = {}
    for call in range(10):
        eng.train_step(rI.to(dev), rS.to(dev), apply=False)
        W = eng.export_weights()
        for d in ('disc_S', 'disc_I'):
            sig = getattr(eng, d).sn_sigma().cpu()
            assert float(sig[:, 1].min()) >= 1 - 1e-5 and (call == 0 or float(sig[:, 0].min()) >= 1 - 1e-5), (d, call, sig[:, :2])
            for k in R.WRAPPED:
                w = W[d][k + '.w']
                tops.setdefault((d, k), []).append(float(torch.linalg.svdvals(w.double().reshape(-1, w.shape[-1]))[0]))
    for key, t in tops.items():
        print('%s %s top singular value over ten calls: %s' % (key + (' '.join('%.5f' % v for v in t),)))
        assert all(b <= a + 1e-5 for a, b in zip(t, t[1:])), key
        assert min(t) >= 1 - 1e-4, key
        assert abs(t[-1] - 1) < abs(t[0] - 1), key


ARGS = dict(N_DEVICES=1, INPUT_IMG_SIZE=(1, 64, 64, 64, 1), CHANNELS=1, GLOBAL_BATCH_SIZE=1, DIMENSIONS=3, SUBVOL_PATCH_SIZE=(32, 32, 32),
            train_steps=5, BATCH_SIZE=1, output_dir=None)


@pytest.mark.parametrize('wasserstein', [False, True])
def test_reference_constructor_use_sn_bf16(wasserstein):
    import argparse
    from van_gan_amd import ops
    from van_gan_amd.compat import VanGan
    from van_gan_amd.synth import synth_volumes
    g = VanGan(argparse.Namespace(**ARGS), None, gen_i2s='resUnet', gen_s2i='resUnet', use_SN=True, wasserstein=wasserstein)
    eng = g.eng
    assert eng.spectral_norm and eng.disc_S.spectral_norm and eng.wasserstein == wasserstein and eng.precision == 'bf16'
    rI, rS = synth_volumes(1, 32, 32, 32, seed=3)
    last = eng.export_weights()['disc_S']
    for _ in range(3):
        r = g.distributed_train_step(rI.numpy(), rS.numpy())
        assert len(r) == 10 and all(v == v and abs(v) < 1e6 for v in r.values()), r
        now = eng.export_weights()['disc_S']
        for k in R.WRAPPED:
            u = now[k + '.sn_u']
            assert not torch.equal(u, last[k + '.sn_u']) and abs(float(u.double().norm()) - 1.0) <= 1e-5, k
        last = now
    # the packed 16-bit operands of every wrapped layer are the packing of the CURRENT fp32 masters (Adam's repack was the last writer)
    torch.cuda.synchronize()
    for d in (eng.disc_S, eng.disc_I):
        items = [it for k in R.WRAPPED for it in d.L[k].pack_items()]
        held = [it[2].clone() for it in items]
        d.pack()
        torch.cuda.synchronize()
        assert all(torch.equal(a, it[2]) for a, it in zip(held, items))
    assert len([l for l in g.disc_S.layers if isinstance(l, type(g.disc_S.layers[1]))]) == 5


RCCL_ONE_SN = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from van_gan_amd.vangan import VanGan
from van_gan_amd.synth import synth_volumes
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
eng = VanGan((32, 32, 32), batch_size=1, n_devices=1, device='cuda:0', seed=4, process_group=dist.group.WORLD, spectral_norm=True)
assert eng.sync.active and eng.sync.forced
assert sorted(k for k in eng.sync.weights if k.endswith('sn_u')) == ['disc_I.sn_u', 'disc_S.sn_u']
u0 = eng.export_weights()['disc_S']['down2.sn_u']
eng.broadcast_weights(0)                                   # carries sn_u: replicas never exchange it again
assert torch.equal(eng.export_weights()['disc_S']['down2.sn_u'], u0)
rI, rS = synth_volumes(1, 32, 32, 32, seed=5)
res = [eng.distributed_train_step(rI.cuda(), rS.cuda()) for _ in range(3)]
eng._join_updates()
torch.cuda.synchronize()
W = eng.export_weights()
ok = all(v == v and abs(v) < 1e6 for r in res for v in r.values())
un = max(abs(float(W[d][k + '.sn_u'].double().norm()) - 1.0) for d in ('disc_S', 'disc_I') for k in ('conv0', 'down0', 'down1', 'down2'))
torch.save({'ok': ok, 'unit': un, 'moved': not torch.equal(W['disc_S']['down2.sn_u'], u0)}, %(out)r)
dist.destroy_process_group()
"""


def test_one_rank_process_group_runs_with_spectral_norm(tmp_path):
    from test_gpu_ddp import _free_port
    out = str(tmp_path / 'rccl1.pt')
    script = tmp_path / 'rccl_one_sn.py'
    script.write_text(RCCL_ONE_SN % dict(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0', VG_DDP_FORCE='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'VG_FAKE_AR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    a = torch.load(out)
    assert a['ok'] and a['moved'] and a['unit'] <= 1e-5, a
