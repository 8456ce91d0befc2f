"""Exact-parity mode (fp32 storage, f32 MFMA): the SAME kernels/schedule as the bf16 product path, instantiated
with float storage, compared with the plain fp32 oracle (no rounding hooks).  This pins the end-to-end wiring of
forward, the four backward sweeps and Adam at fp32 tolerance, which the bf16 path cannot (its noise floor is
~2e-2 forward and cos 0.95 on generator gradients, see test_gpu_nets.py).

Stated tolerances (fp32 arithmetic, different summation orders, two 30-conv generators in series):
  generator / discriminator outputs : relative L2 <= 2e-3
  losses                            : relative error <= 2e-3
  parameter gradients               : whole-network cosine >= 0.9995, per-tensor relative L2 <= 5e-2
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vangan_oracle as O  # noqa: E402
from test_gpu_nets import grad_report, perturb, rel_l2  # noqa: E402


def _dev():
    return torch.device('cuda:0')


def test_generator_fp32_forward_backward():
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs
    from van_gan_amd.ops import Arena
    dev = _dev()
    dims, N = (32, 32, 32), 1
    P = perturb(O.init_params(O.gen_param_specs(), 11), 12)
    st = ParamStore(gen_param_specs(), dev)
    st.load(P)
    net = ResUNet(st, dims, torch.float32)
    net.pack()
    ar = Arena(2 << 30, dev)
    x, _ = O.synth_volumes(N, *dims, seed=5)
    y = torch.zeros(N, *dims, 1, device=dev)
    ctx = net.forward(ar, x.to(dev), y)
    torch.cuda.synchronize()
    Pr = {k: v.clone().double().requires_grad_(True) for k, v in P.items()}
    taps = {}
    yr = O.resunet_forward(Pr, x.double(), taps=taps)
    for name, key in (('stem', 'stem'), ('enc1', 'enc1'), ('enc4', 'enc4'), ('dec0', 'dec0')):
        e = rel_l2(ctx[key]['out'].data, O.to_ndhwc(taps[name]).detach())
        print('tap %-6s rel_l2 %.3e' % (name, e))
        assert e < 1e-3, name
    e = rel_l2(y, yr.detach())
    print('generator fp32 output rel l2 %.3e max abs %.3e' % (e, float((y.cpu().double() - yr.detach()).abs().max())))
    assert e < 1e-3
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(y.shape, generator=g) / y.numel()
    (yr * gy.double()).sum().backward()
    st.g.zero_()
    net.backward(ar, ctx, gy.to(dev))
    torch.cuda.synchronize()
    cos = grad_report(st.export(st.g), {k: v.grad for k, v in Pr.items()}, 'generator fp32', rel_tol=5e-2, cos_tol=0.999)
    assert cos > 0.9995


def _engine_fp32(dims, B):
    from van_gan_amd import VanGan
    dev = _dev()
    eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=0, layer_noise=0.0, dropout_rate=0.0,
                 precision='fp32')
    P = {k: perturb(v, 40 + i) for i, (k, v) in enumerate(O.make_models(0).items())}
    eng.load_weights(P)
    rI, rS = O.synth_volumes(B, *dims, seed=1234)
    res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={})
    Pd = {k: {n: t.double() for n, t in v.items()} for k, v in P.items()}
    ref, grads, aux = O.train_step(Pd, {}, rI.double(), rS.double(), O.Cfg(B, 1))
    for k in O.RESULT_KEYS:
        print('   %-24s hip %.6f  oracle %.6f' % (k, res[k], ref[k]))
    for k in ('fake_S', 'fake_I', 'cycled_S', 'cycled_I'):
        r = rel_l2(eng._aux[k], aux[k])
        print('   %-10s rel l2 %.3e' % (k, r))
        assert r < 2e-3, k
    for k in O.RESULT_KEYS:
        assert abs(res[k] - ref[k]) <= 2e-3 * abs(ref[k]) + 1e-6, k
    got = eng.export_grads()
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        cos = grad_report(got[net], grads[net], net + ' fp32', rel_tol=5e-2, cos_tol=0.999)
        assert cos > 0.9995, (net, cos)
    W = eng.export_weights()
    # Adam: the oracle applied its own gradients; compare updated weights where the update is well defined
    nbad = ntot = 0
    for net in W:
        for n in W[net]:
            d = (W[net][n].double() - Pd[net][n]).abs()
            nbad += int((d > 1e-4).sum()); ntot += d.numel()
    print('   weights after Adam: %d / %d elements differ by > 1e-4 (|step| <= 6.3e-4)' % (nbad, ntot))
    assert nbad <= 2e-3 * ntot


def test_train_step_fp32_32_b1():
    _engine_fp32((32, 32, 32), 1)


def test_train_step_fp32_32_b2():
    _engine_fp32((32, 32, 32), 2)


def test_train_step_fp32_32_b3():
    """The reference's own per-GPU batch: the generators at N = 3 and 6, the discriminators at N = 6 and 9 (backward_both's 3B launch),
    losses divided by the global batch 3 -- against the float64 oracle run live, with the bounds of the two tests above."""
    _engine_fp32((32, 32, 32), 3)


def test_stream_schedule_does_not_change_gradients():
    """The engine's schedule (two lanes + per-lane weight-gradient side streams, van_gan_amd/vangan.py) must only reorder
    independent work.  Same weights and inputs with the lanes on and off: every loss and every gradient buffer has to
    agree to fp32 reordering noise (a shared scratch buffer between lanes once showed up here as rel 0.3-1.4 on
    single tensors)."""
    import os
    from van_gan_amd import VanGan
    dev = _dev()
    dims, B = (32, 32, 32), 2
    P = {k: perturb(v, 40 + i) for i, (k, v) in enumerate(O.make_models(0).items())}
    rI, rS = O.synth_volumes(B, *dims, seed=4321)
    outs = []
    for lanes in ('1', '0', '0'):
        old = {k: os.environ.get(k) for k in ('VG_LANES', 'VG_SIDE_STREAM')}
        os.environ['VG_LANES'], os.environ['VG_SIDE_STREAM'] = lanes, lanes
        try:
            eng = VanGan(dims, batch_size=B, n_devices=1, device='cuda:0', seed=0, layer_noise=0.0, dropout_rate=0.0,
                         precision='fp32')
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        eng.load_weights(P)
        res = None
        for _ in range(3):                      # a race needs a few tries to show
            res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={}, apply=False)
        outs.append((res, eng.export_grads()))
    (r1, g1), (r0, g0), (r0b, g0b) = outs

    def worst(ga, gb):
        # whole-network relative L2 (biases in front of an InstanceNorm have an analytically zero gradient: their
        # per-tensor relative error is pure noise)
        w, where = 0.0, None
        for net in gb:
            num = sum(float((ga[net][n].double() - gb[net][n].double()).pow(2).sum()) for n in gb[net])
            den = sum(float(gb[net][n].double().pow(2).sum()) for n in gb[net])
            e = (num / (den + 1e-300)) ** 0.5
            if e > w:
                w, where = e, net
        return w, where
    floor, wf = worst(g0b, g0)                  # serial vs serial: float-atomic ordering alone
    got, wg = worst(g1, g0)
    print('schedule test: serial-vs-serial worst network rel L2 %.2e (%s); lanes-vs-serial %.2e (%s)' % (floor, wf, got, wg))
    for k in O.RESULT_KEYS:
        assert abs(r1[k] - r0[k]) <= 1e-4 * abs(r0[k]) + 1e-6, k
    # reordered float atomics alone move a network's gradient by the floor printed above; the scratch race moved single
    # large tensors by 0.3-1.4 (whole-network > 1e-1)
    assert got <= max(20.0 * floor, 1e-2), (got, wg, floor)


def test_stem_shortcut_backward_from_the_statistics_pass():
    """The stem shortcut (1x1x1 convolution of the single-channel volume + InstanceNorm, resunet_model.py:96-99) has no data gradient and
    its normalised output does not depend on the kernel's magnitude, only on eps: dL/dw = eps * gamma * rs^3 * sum(d_out * (x - mean x)), a
    closed form in two moments of the block-output gradient against the volume (vg_stem_short_bwd), dL/db = 0.  Against float64 autograd through the oracle, and
    beside the explicit path (apply pass -> gradient tensor -> weight-gradient launch; nets._STEM_AUX = False), fp32 storage, batch 2: the
    closed form must be as close to the oracle as the explicit sum of a million terms, and everything else unchanged."""
    from van_gan_amd import nets
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs
    from van_gan_amd.ops import Arena
    dev = _dev()
    dims, N = (32, 32, 32), 2
    P = perturb(O.init_params(O.gen_param_specs(), 21), 22)
    x, _ = O.synth_volumes(N, *dims, seed=8)
    g = torch.Generator().manual_seed(9)
    gy = torch.randn(N, *dims, 1, generator=g) / (N * 32 ** 3)
    Pr = {k: v.clone().double().requires_grad_(True) for k, v in P.items()}
    (O.resunet_forward(Pr, x.double()) * gy.double()).sum().backward()
    res = {}
    for aux in (True, False):
        nets._STEM_AUX = nets._STEM_FUSED = aux            # the explicit backward needs the materialised branch
        try:
            st = ParamStore(gen_param_specs(), dev)
            st.load(P)
            net = ResUNet(st, dims, torch.float32)
            net.pack()
            ar = Arena(3 << 30, dev)
            y = torch.zeros(N, *dims, 1, device=dev)
            ctx = net.forward(ar, x.to(dev), y)
            st.g.zero_()
            net.backward(ar, ctx, gy.to(dev))
            torch.cuda.synchronize()
            res[aux] = st.export(st.g)
        finally:
            nets._STEM_AUX = nets._STEM_FUSED = True
    err = {aux: rel_l2(res[aux]['stem.short.w'], Pr['stem.short.w'].grad) for aux in (True, False)}
    print('stem.short.w vs float64 autograd: closed form rel %.3e, explicit path rel %.3e' % (err[True], err[False]))
    # measured over runs: both between 2e-4 and 2e-3 (the upstream gradient d_out itself moves by ~1e-3 from run to run: float atomics);
    # the other fp32 gradient checks of this file allow 5e-2 per tensor
    assert err[True] < 1e-2 and err[True] <= 3 * err[False] + 2e-3
    ref = {k: v.grad for k, v in Pr.items()}
    for aux in (True, False):
        cos = grad_report(res[aux], ref, 'generator fp32, stem shortcut %s' % ('closed form' if aux else 'explicit'), rel_tol=5e-2, cos_tol=0.999)
        assert cos > 0.9995
    assert float(res[True]['stem.short.b'].abs().max()) == 0.0          # identically zero; the explicit path leaves rounding noise
