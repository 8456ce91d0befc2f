"""GPU tests of the attention-gated ResUNet (ResUNet(use_attention_gate=True), resunet_model.py:152,178-179; vg_attngate.hip), all
through the C ABI, against the float64 restatement of tests/ag_restate.py (itself checked on the CPU, tests/test_attngate_host.py).

Tolerances are the project's own for the same kinds of quantity:
  kernel level (tests/test_gpu_ops.py): fp32 outputs rel_l2 < 1e-4, per-channel sums < 1e-4, weight / bias gradients < 2e-3, 16-bit outputs
      elementwise 1.2e-2 |ref| + 2e-3 max|ref|, 16-bit data gradients 2.5e-2 |ref| + 6e-3 max|ref|, against a restatement that rounds
      at the engine's storage points (the weights of theta on the matrix pipe, phi, the gated tensor);
  network / engine level, fp32 storage (tests/test_gpu_fp32.py): taps and outputs rel_l2 < 1e-3, scalars 2e-3 relative,
      grad_report(rel_tol=5e-2, cos_tol=0.999), whole-network cosine > 0.9995, Adam <= 2e-3 of the elements off by > 1e-4;
  teacher-forced bf16 (tests/test_gpu_teacher.py): every tensor 8e-2 / 0.997, whole network >= 0.9995; no gate tensor has a bound
      of its own.
Every measured value is printed."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import ag_restate as R  # noqa: E402
from oracle import vangan_oracle as O  # noqa: E402
from test_gpu_nets import grad_report, perturb, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
LEVELS = {0: (16, 32), 1: (32, 64), 2: (64, 128), 3: (128, 256)}          # decoder level -> (Cs, Ci)


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def _ratio16(got, ref, rel, scale):
    return (got - ref).abs() / (rel * ref.abs() + scale + 1e-30)


def _close16(got, ref, name, rel, floor):
    got, ref = got.double().cpu(), ref.double().cpu()
    ratio = _ratio16(got, ref, rel, floor * ref.abs().max())
    worst = float(ratio.max())
    print('   %-22s max err %.3e (max |ref| %.3e), worst err / tolerance %.3f' % (name, float((got - ref).abs().max()), float(ref.abs().max()), worst))
    assert worst <= 1.0, '%s: %d/%d outside %.1e |ref| + %.1e max|ref|' % (name, int((ratio > 1.0).sum()), ratio.numel(), rel, floor)


def _relu_kinks(pre, skip, phi_up, wq, b):
    """(voxel, channel) pairs at which the float64 restatement's gradient is one of TWO equally valid answers: relu's argument
    pre = skip . W + b + phi is closer to 0 than fp32 arithmetic can place it -- the standard forward error bound of an fp32 dot product of
    Cs + 2 terms, tau = (Cs + 2) 2^-24 (|skip| . |W| + |b| + |phi|) -- so the engine (fp32 accumulation) and the restatement (float64) may
    legitimately disagree on [pre > 0] there, and dq of that channel is either 0 or dz w_psi.  Returns (mask [N, D, H, W, Ci], the number of
    such pairs to expect: sum of 2 tau times the density of pre at 0, pre taken as normal).  All NDHWC float64."""
    tau = (skip.shape[-1] + 2) * 2.0 ** -24 * (skip.abs() @ wq.abs() + b.abs() + phi_up.abs())
    expect = float(2.0 * tau.sum() / ((2.0 * torch.pi) ** 0.5 * pre.std()))
    return pre.abs() <= tau, expect


def _subsets(k):
    return [[i for i in range(k) if m >> i & 1] for m in range(1 << k)]


def _close16_two_valued(got, ref, alt_dq, wq, name, rel, floor):
    """EVERY element is held to the bound.  Where relu's decision is two-valued (alt_dq != 0: what dq of that (voxel, channel) changes
    by under the other decision) the reference is the better of the candidates -- one decision per flagged channel, applied to the
    whole voxel (d_skip: wq [Cs, Ci] given, the voxel's Cs values move together by alt_dq * wq[:, ci]) or to the element (d_phi: wq None,
    alt_dq regrouped as [N, LD, LH, LW, 8 children, Ci], element (low voxel, ci) moves by the chosen children's alt_dq)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    scale = floor * ref.abs().max()
    ratio = _ratio16(got, ref, rel, scale)
    n_plain = int((ratio > 1.0).sum())
    if wq is not None:
        for n, d, h, w in alt_dq.ne(0).any(-1).nonzero().tolist():
            cis = alt_dq[n, d, h, w].nonzero().flatten().tolist()
            assert len(cis) <= 8, (name, len(cis))
            best = None
            for sub in _subsets(len(cis)):
                cand = ref[n, d, h, w] + sum((alt_dq[n, d, h, w, cis[i]] * wq[:, cis[i]] for i in sub), torch.zeros_like(ref[n, d, h, w]))
                r = _ratio16(got[n, d, h, w], cand, rel, scale)
                if best is None or float(r.max()) < float(best.max()):
                    best = r
            ratio[n, d, h, w] = best
    else:
        for n, d, h, w, ci in alt_dq.ne(0).any(4).nonzero().tolist():
            ch = alt_dq[n, d, h, w, :, ci]
            kids = ch.nonzero().flatten().tolist()
            cands = [ref[n, d, h, w, ci] + sum(float(ch[kids[i]]) for i in sub) for sub in _subsets(len(kids))]
            ratio[n, d, h, w, ci] = min(float(_ratio16(got[n, d, h, w, ci], c, rel, scale)) for c in cands)
    worst = float(ratio.max())
    print('   %-22s max err %.3e (max |ref| %.3e); %d elements outside the bound against the float64 decision, %d against the better of the '
          'two valid ones; worst err / tolerance %.3f' % (name, float((got - ref).abs().max()), float(ref.abs().max()), n_plain,
                                                          int((ratio > 1.0).sum()), worst))
    assert worst <= 1.0, '%s: %d/%d outside %.1e |ref| + %.1e max|ref|' % (name, int((ratio > 1.0).sum()), ratio.numel(), rel, floor)


def _gate_params(Cs, Ci, g, dev):
    he = lambda fan, *s: torch.randn(*s, generator=g) * (2.0 / fan) ** 0.5
    p = {'g.theta.w': he(Cs, 1, 1, 1, Cs, Ci), 'g.theta.b': torch.randn(Ci, generator=g) * 0.1,
         'g.psi.w': he(Ci, 1, 1, 1, Ci, 1) * 2.0, 'g.psi.b': torch.randn(1, generator=g) * 0.1}
    return {k: v.to(dev) for k, v in p.items()}


class _Fp16Round(torch.autograd.Function):
    """IEEE half-precision storage rounding, straight-through (the fp16 build's counterpart of O.bf16_round)."""
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('N,dims', [(1, (128, 128, 128)), (2, (128, 128, 64))])
@pytest.mark.parametrize('level', [0, 1, 2, 3])
def test_gate_kernels_at_true_shapes(level, N, dims, precision):
    _gate_kernel_case(level, N, dims, precision)


@pytest.mark.parametrize('level', [0, 3])
def test_gate_kernels_fp16_build(level):
    """The same sources compiled with -DVG_FP16 (libvangan_hip_h.so: f16 MFMA, half-precision fragments), 128 x 128 x 64 batch 2: the
    smallest and the largest channel counts, at the 16-bit bounds."""
    from van_gan_amd import ops
    with ops.Fp16():
        _gate_kernel_case(level, 2, (128, 128, 64), 'fp16')


def _gate_kernel_case(level, N, dims, precision):
    from van_gan_amd import ops
    dev = torch.device(DEV)
    ops.set_device(dev.index)
    f32 = precision == 'fp32'
    dt = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[precision]
    q = {'fp32': None, 'bf16': O.bf16_round, 'fp16': _Fp16Round.apply}[precision]
    Cs, Ci = LEVELS[level]
    lv = tuple(n >> level for n in dims)
    low = tuple(n // 2 for n in lv)
    g = torch.Generator().manual_seed(100 + level)
    gd = torch.Generator(device=dev).manual_seed(200 + level)
    rn = lambda *s: torch.randn(*s, generator=gd, device=dev)
    p = _gate_params(Cs, Ci, g, dev)
    skip, phi, dG = rn(N, *lv, Cs).to(dt), (rn(N, *low, Ci) * 0.7).to(dt), rn(N, *lv, Cs).to(dt)
    gated, h = torch.empty_like(skip), torch.empty(N, *lv, device=dev)
    sums = torch.zeros(ops.STRIPES, N, Cs, 2, device=dev)
    args = (p['g.theta.w'], p['g.theta.b'], p['g.psi.w'], p['g.psi.b'])
    ops.attn_gate_fwd(skip, phi, *args, (N,) + lv, Cs, Ci, gated, h, sums)
    torch.cuda.synchronize()
    # float64 restatement (host) on the same, already rounded, operands, rounding where the engine rounds
    p64 = {k: v.cpu().double().requires_grad_(True) for k, v in p.items()}
    s64, f64 = skip.cpu().double().requires_grad_(True), phi.cpu().double().requires_grad_(True)
    taps = {}
    gr, hr = R.attention_gate(p64, 'g', O.to_ncdhw(s64), None, q, phi=O.to_ncdhw(f64), taps=taps)
    gr_n, hr_n = O.to_ndhwc(gr), hr[:, 0]
    with torch.no_grad():
        phi_up = f64.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
        wq = O._q(q, p64['g.theta.w'])[0, 0, 0].detach()
        pre = O.to_ndhwc(taps['g.pre']).detach()
        kink, expect = _relu_kinks(pre, s64.detach(), phi_up, wq, p64['g.theta.b'].detach())
        # what dq changes by under the other relu decision, at the two-valued (voxel, channel) pairs only
        dz = (dG.cpu().double() * s64.detach()).sum(-1) * hr[:, 0].detach() * (1 - hr[:, 0].detach())
        alt_dq = dz[..., None] * p64['g.psi.w'].detach()[0, 0, 0, :, 0] * (1.0 - 2.0 * (pre > 0).double()) * kink
        alt_low = alt_dq.view(N, low[0], 2, low[1], 2, low[2], 2, Ci).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(N, *low, 8, Ci)
    print('   (voxel, channel) pairs with a two-valued relu decision: %d of %d, expected %.1f' % (int(kink.sum()), kink.numel(), expect))
    assert int(kink.sum()) <= 3.0 * expect + 10         # a Poisson count around `expect`: three times it (+ 10 for the small levels)
    print('\ngate level %d N %d %s %s: h in [%.3f, %.3f]' % (level, N, lv, precision, float(hr_n.detach().min()), float(hr_n.detach().max())))
    e_h = _rel(h, hr_n.detach())
    print('   h rel_l2 %.3e' % e_h)
    assert e_h < 1e-4
    if f32:
        e = _rel(gated, gr_n.detach())
        print('   gated rel_l2 %.3e' % e)
        assert e < 1e-4
    else:
        _close16(gated, gr_n.detach(), 'gated', 1.2e-2, 2e-3)
    st = gated.cpu().double()
    ref_sums = torch.stack([st.sum((1, 2, 3)), (st * st).sum((1, 2, 3))], -1)
    e_s = _rel(sums.sum(0), ref_sums)
    print('   sums of the stored gated tensor rel_l2 %.3e' % e_s)
    assert e_s < 1e-4
    # backward
    (gr_n * dG.cpu().double()).sum().backward()
    pg = {k: torch.zeros_like(v) for k, v in p.items()}
    base = rn(N, *lv, Cs).to(dt)
    res = {}
    for acc in (0, 1):
        for v in pg.values():
            v.zero_()
        dskip = base.clone() if acc else torch.full_like(skip, float('nan'))
        dphi = torch.full_like(phi, float('nan'))
        ops.attn_gate_bwd(dG, skip, h, phi, p['g.theta.w'], p['g.theta.b'], p['g.psi.w'], (N,) + lv, Cs, Ci, dskip, bool(acc), dphi,
                          pg['g.theta.w'], pg['g.theta.b'], pg['g.psi.w'], pg['g.psi.b'])
        torch.cuda.synchronize()
        res[acc] = (dskip, dphi, {k: v.clone() for k, v in pg.items()})
    for acc in (0, 1):
        dskip, dphi, grads = res[acc]
        ref_ds = s64.grad + (base.cpu().double() if acc else 0.0)
        tag = 'accumulate' if acc else 'first writer'
        if f32:
            e1, e2 = _rel(dskip, ref_ds), _rel(dphi, f64.grad)
            print('   d_skip (%s) rel_l2 %.3e, d_phi rel_l2 %.3e' % (tag, e1, e2))
            assert e1 < 1e-4 and e2 < 1e-4
        else:
            _close16_two_valued(dskip, ref_ds, alt_dq, wq, 'd_skip (%s)' % tag, 2.5e-2, 6e-3)
            _close16_two_valued(dphi, f64.grad, alt_low, None, 'd_phi', 2.5e-2, 6e-3)
        for k in ('g.theta.w', 'g.theta.b', 'g.psi.w', 'g.psi.b'):
            e = _rel(grads[k], p64[k].grad)
            print('   d %-10s rel_l2 %.3e' % (k[2:], e))
            assert e < 2e-3, (k, e)


def _gated_net(P, dims, dtype, gate=True):
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs
    dev = torch.device(DEV)
    st = ParamStore(gen_param_specs(gate), dev)
    st.load(P)
    net = ResUNet(st, dims, dtype, attention_gate=gate)
    net.pack()
    return st, net


def _gated_params(seed):
    P = perturb(O.init_params(R.gen_ag_param_specs(), seed), seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for d in range(4):                                   # a psi bias away from 0 moves the gate off sigmoid(~0)
        P['dec%d.gate.psi.b' % d].add_(torch.randn(1, generator=g) * 0.5)
    return P


def test_identity_gate_reproduces_the_plain_generator():
    """psi.w = 0, psi.b = 40: h = 1 and h (1 - h) = 0 exactly in fp32, so the gated network computes the plain one (not bitwise: the
    statistics of `gated` are summed in another order than those of `skip`) and all 24 gate gradients are exactly zero."""
    from van_gan_amd.ops import Arena
    dev = torch.device(DEV)
    dims, N = (32, 32, 32), 1
    P = _gated_params(31)
    for d in range(4):
        P['dec%d.gate.psi.w' % d].zero_()
        P['dec%d.gate.psi.b' % d].fill_(40.0)
    x, _ = O.synth_volumes(N, *dims, seed=5)
    gy = torch.randn(N, *dims, 1, generator=torch.Generator().manual_seed(3)) / (N * 32 ** 3)
    out = {}
    for gate in (True, False):
        st, net = _gated_net(P if gate else {k: v for k, v in P.items() if '.gate.' not in k}, dims, torch.float32, gate)
        ar = Arena(2 << 30, dev)
        y = torch.zeros(N, *dims, 1, device=dev)
        ctx = net.forward(ar, x.to(dev), y)
        if gate:
            hs = [ctx['dec%d' % d]['gate']['h'] for d in range(4)]
            assert all(bool((h == 1.0).all()) for h in hs)
        st.g.zero_()
        net.backward(ar, ctx, gy.to(dev))
        torch.cuda.synchronize()
        out[gate] = (y.cpu(), st.export(st.g))
    e = rel_l2(out[True][0], out[False][0])
    print('identity gate: output rel_l2 %.3e to the plain generator' % e)
    assert e < 1e-3
    gate_grads = {k: v for k, v in out[True][1].items() if '.gate.' in k}
    assert len(gate_grads) == 24 and all(float(v.abs().max()) == 0.0 for v in gate_grads.values()), \
        {k: float(v.abs().max()) for k, v in gate_grads.items() if float(v.abs().max()) != 0.0}
    shared = {k: v for k, v in out[True][1].items() if '.gate.' not in k}
    assert len(shared) == 116
    cos = grad_report(shared, {k: v.double() for k, v in out[False][1].items()}, 'identity gate vs plain generator fp32', rel_tol=5e-2, cos_tol=0.999)
    assert cos > 0.9995


def test_gated_generator_fp32_forward_backward():
    from van_gan_amd.ops import Arena
    dev = torch.device(DEV)
    dims, N = (32, 32, 32), 1
    P = _gated_params(11)
    st, net = _gated_net(P, dims, torch.float32)
    ar = Arena(2 << 30, dev)
    x, _ = O.synth_volumes(N, *dims, seed=5)
    y = torch.zeros(N, *dims, 1, device=dev)
    ctx = net.forward(ar, x.to(dev), y)
    torch.cuda.synchronize()
    Pr = {k: v.clone().double().requires_grad_(True) for k, v in P.items()}
    taps = {}
    yr = R.resunet_ag_forward(Pr, x.double(), taps=taps)
    for name, got in (('dec3.gate', ctx['dec3']['inp'][1].data), ('dec0.gate', ctx['dec0']['inp'][1].data), ('dec0', ctx['dec0']['out'].data)):
        e = rel_l2(got, O.to_ndhwc(taps[name]).detach())
        print('tap %-10s rel_l2 %.3e' % (name, e))
        assert e < 1e-3, name
    for d in range(4):
        hr = taps['dec%d.gate.h' % d].detach()
        print('gate h level %d: rel_l2 %.3e, reference range [%.3f, %.3f]' % (d, rel_l2(ctx['dec%d' % d]['gate']['h'], hr[:, 0]), float(hr.min()), float(hr.max())))
    e = rel_l2(y, yr.detach())
    print('gated generator fp32 output rel l2 %.3e' % e)
    assert e < 1e-3
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)) / y.numel()
    (yr * gy.double()).sum().backward()
    st.g.zero_()
    net.backward(ar, ctx, gy.to(dev))
    torch.cuda.synchronize()
    got = st.export(st.g)
    assert len(got) == 140
    cos = grad_report(got, {k: v.grad for k, v in Pr.items()}, 'gated generator fp32', rel_tol=5e-2, cos_tol=0.999)
    assert cos > 0.9995


def _models(seed=0):
    ds = O.disc_param_specs()
    gs = R.gen_ag_param_specs()
    return {'gen_IS': O.init_params(gs, seed), 'gen_SI': O.init_params(gs, seed + 1), 'disc_I': O.init_params(ds, seed + 2),
            'disc_S': O.init_params(ds, seed + 3)}


@pytest.mark.parametrize('B', [1, 2])
def test_gated_train_step_fp32(B, monkeypatch):
    from van_gan_amd import VanGan
    dev = torch.device(DEV)
    dims = (32, 32, 32)
    eng = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32', attention_gate=True)
    P = {k: perturb(v, 40 + i) for i, (k, v) in enumerate(_models(0).items())}
    eng.load_weights(P)
    rI, rS = O.synth_volumes(B, *dims, seed=1234)
    res = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={})
    Pd = {k: {n: t.double() for n, t in v.items()} for k, v in P.items()}
    monkeypatch.setattr(O, 'resunet_forward', R.resunet_ag_forward)
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
    assert len(got['gen_IS']) == 140
    for net in ('disc_I', 'disc_S', 'gen_IS', 'gen_SI'):
        cos = grad_report(got[net], grads[net], net + ' fp32 (attention gate)', rel_tol=5e-2, cos_tol=0.999)
        assert cos > 0.9995, (net, cos)
    W = eng.export_weights()
    nbad = ntot = 0
    for net in W:
        for n in W[net]:
            d = (W[net][n].double() - Pd[net][n]).abs()
            nbad += int((d > 1e-4).sum()); ntot += d.numel()
    print('   weights after Adam: %d / %d elements differ by > 1e-4' % (nbad, ntot))
    assert nbad <= 2e-3 * ntot


@pytest.mark.parametrize('dims,N', [((32, 32, 32), 2), ((128, 128, 64), 1)])
def test_teacher_forced_gated_generator_bf16(dims, N):
    """One gated generator, bf16 product kernels: all 140 parameter gradients against autograd through the teacher-forced restatement
    (the teacher map of tests/test_gpu_teacher.py plus the gate's storage points dec%d.gate.phi and dec%d.gate)."""
    from test_gpu_teacher import STEM_SHORT_E2E, _gen_keys
    from van_gan_amd.ops import Arena
    dev = torch.device(DEV)
    P = _gated_params(11)
    st, net = _gated_net(P, dims, torch.bfloat16)
    S = dims[0] * dims[1] * dims[2]
    ar = Arena(int(N * S * 7000) + (1 << 30), dev)
    x, _ = O.synth_volumes(N, *dims, seed=5)
    y = torch.zeros(N, *dims, 1, device=dev)
    ctx = net.forward(ar, x.to(dev), y)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)) / y.numel()
    st.g.zero_()
    net.backward(ar, ctx, gy.to(dev))
    torch.cuda.synchronize()
    T = {key: O.to_ncdhw(ctx[blk][field].data.float().cpu()) for key, (blk, field) in _gen_keys()}
    for d in range(4):
        T['dec%d.gate' % d] = O.to_ncdhw(ctx['dec%d' % d]['inp'][1].data.float().cpu())
        T['dec%d.gate.phi' % d] = O.to_ncdhw(ctx['dec%d' % d]['gate']['phi'].data.float().cpu())
    T['y'] = O.to_ncdhw(y.float().cpu())
    used, drift = set(), {}

    def teacher(key, t):
        used.add(key)
        drift[key] = float((T[key].double() - t.detach().double()).norm() / (T[key].double().norm() + 1e-30))
        return T[key]

    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    O.TEACHER = teacher
    try:
        yr = R.resunet_ag_forward(Pr, x, q=O.bf16_round)
    finally:
        O.TEACHER = None
    assert used == set(T)
    worst = sorted(drift.items(), key=lambda kv: -kv[1])[:5]
    print('teacher-forced forward: worst per-tensor drift', worst)
    print('gate storage points drift', {k: '%.2e' % v for k, v in drift.items() if '.gate' in k})
    assert worst[0][1] < 2e-2, worst
    (yr * gy).sum().backward()
    # abs_tol (tensors whose reference norm is below 1e-2 of the largest: the analytically zero bias gradients) and the stem.short.w bound
    # are the project's: 5e-3 at 32^3 (test_gpu_teacher.py::_check), 4e-2 where a bias gradient sums a million bf16-stored voxels
    # (::test_teacher_forced_generator_128x128x64)
    got, ref = st.export(st.g), {k: v.grad for k, v in Pr.items()}
    cos = grad_report(got, ref, 'gated generator %s bf16 (teacher-forced)' % (dims,), rel_tol=8e-2, cos_tol=0.997,
                      abs_tol=5e-3 if S <= 32 ** 3 else 4e-2, special={'stem.short.w': STEM_SHORT_E2E})
    assert cos >= 0.9995, cos
    # The gate tensors are held to the common RELATIVE bound whatever their norm: most of them are below 1e-2 of the largest gradient norm
    # and would otherwise pass through grad_report's absolute branch.  The four psi.b gradients are ONE-element tensors -- each a single
    # signed sum over all voxels, which at a given forward state can cancel to any fraction of its terms (measured: dec2.gate.psi.b 2.4e-6
    # beside 1.4e-4 .. 3.1e-4 for the other three levels, its error of 3.9e-7 then reads as 1.7e-1 of itself), so a norm over one element
    # is not a scale; they are compared together, as the 4-vector they form.
    gmax = max(float(v.double().norm()) for v in ref.values())
    gate = [k for k in ref if '.gate.' in k]
    assert len(gate) == 24
    groups = {k: [k] for k in gate if not k.endswith('.psi.b')}
    groups['dec*.gate.psi.b'] = [k for k in gate if k.endswith('.psi.b')]
    assert all(ref[k].numel() == 1 for k in groups['dec*.gate.psi.b']) and all(ref[k].numel() > 1 for k in groups if k in ref)
    bad = []
    for name, ks in groups.items():
        a = torch.cat([got[k].double().cpu().flatten() for k in ks])
        b = torch.cat([ref[k].double().flatten() for k in ks])
        rel, cs = float((a - b).norm() / b.norm()), float((a @ b) / (a.norm() * b.norm() + 1e-30))
        print('   %-22s |ref| %.3e (%.1e of the largest) rel %.3e cos %.5f' % (name, float(b.norm()), float(b.norm()) / gmax, rel, cs))
        if rel > 8e-2 or cs < 0.997:
            bad.append((name, rel, cs))
    for k in groups['dec*.gate.psi.b']:
        print('   %-22s ref %+.3e got %+.3e' % (k, float(ref[k]), float(got[k])))
    assert not bad, bad


def test_engine_two_steps_test_step_generate_checkpoint_and_replay(tmp_path):
    from van_gan_amd import VanGan
    dev = torch.device(DEV)
    B, dims = 1, (32, 32, 32)
    eng = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, precision='fp32', layer_noise=0.0, dropout_rate=0.0, attention_gate=True,
                 output_dir=str(tmp_path))
    P = eng.export_weights()
    assert len(P['gen_IS']) == 140 and sum(v.numel() for v in P['gen_SI'].values()) == 9670933
    # init_reference: he_normal with fan-in Cs, Cx, Ci (truncated normal: std = sqrt(2 / fan_in) after the 0.8796 correction), zero biases
    for d, (cs, ci) in LEVELS.items():
        for k, fan in (('theta', cs), ('phi', ci), ('psi', ci)):
            w = P['gen_IS']['dec%d.gate.%s.w' % (d, k)]
            assert float(P['gen_IS']['dec%d.gate.%s.b' % (d, k)].abs().max()) == 0.0
            if w.numel() >= 2048:
                assert abs(float(w.std()) / (2.0 / fan) ** 0.5 - 1.0) < 0.1, (d, k, float(w.std()))
    rI, rS = O.synth_volumes(B, *dims, seed=21)
    ref = {n: {k: v.double().clone() for k, v in P[n].items()} for n in ('gen_IS', 'gen_SI')}
    opt = {'gen_IS': {}, 'gen_SI': {}}
    for step in range(2):
        r = eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={}, apply=True)
        assert all(v == v and abs(v) < 1e6 for v in r.values()), r
        grads = eng.export_grads()
        for n in ref:
            O.adam_step(ref[n], {k: grads[n][k].double() for k in ref[n]}, opt[n])
    W = eng.export_weights()
    for n in ref:
        # the engine's Adam on its own gradients: every tensor, the 24 gate tensors included, moved as the restated optimizer moves it
        nbad = sum(int(((W[n][k].double() - ref[n][k]).abs() > 1e-6).sum()) for k in ref[n])
        ntot = sum(v.numel() for v in ref[n].values())
        moved = [k for k in ref[n] if '.gate.' in k and torch.equal(W[n][k], P[n][k])]
        print('%s after two applied steps: %d / %d elements differ by > 1e-6 from the restated Adam; unmoved gate tensors %s' % (n, nbad, ntot, moved))
        assert nbad <= 2e-3 * ntot and not moved
    t = eng.test_step(rI.to(dev), rS.to(dev))
    assert len(t) == 10 and all(v == v for v in t.values())
    W2 = eng.export_weights()
    assert all(torch.equal(W2[n][k], W[n][k]) for n in W for k in W[n])
    # generate runs the gated forward: against the restatement on the current weights
    fake = eng.generate('gen_IS', rI.to(dev))
    with torch.no_grad():
        yr = R.resunet_ag_forward({k: v.double() for k, v in W['gen_IS'].items()}, rI.double())
        y_plain = O.resunet_forward({k: v.double() for k, v in W['gen_IS'].items()}, rI.double())
    e = rel_l2(fake, yr)
    print('generate() vs gated restatement rel_l2 %.3e (the ungated network on the same weights: %.3e)' % (e, rel_l2(fake, y_plain)))
    assert e < 1e-3 and rel_l2(fake, y_plain) > 1e-2
    # checkpoint round trip; a checkpoint of the other configuration is refused as a whole
    eng.save_checkpoint(0)
    eng.train_step(rI.to(dev), rS.to(dev), noise={}, drop={}, apply=True)
    assert not torch.equal(eng.export_weights()['gen_IS']['dec0.gate.psi.w'], W['gen_IS']['dec0.gate.psi.w'])
    assert eng.load_checkpoint(1)
    W3 = eng.export_weights()
    assert all(torch.equal(W3[n][k], W[n][k]) for n in W for k in W[n])
    plain = VanGan(dims, batch_size=B, n_devices=1, device=DEV, seed=0, precision='fp32', output_dir=str(tmp_path / 'plain'))
    before = plain.export_weights()
    with pytest.raises(ValueError, match='attention gate'):
        plain.load_checkpoint(1, newpath=eng.checkpoint_dir)
    after = plain.export_weights()
    assert all(torch.equal(before[n][k], after[n][k]) for n in before for k in before[n])
    plain.save_checkpoint(0)
    with pytest.raises(ValueError, match='attention gate'):
        eng.load_checkpoint(1, newpath=plain.checkpoint_dir)
    with pytest.raises(ValueError):
        VanGan(dims, batch_size=B, device=DEV, generator='resnet', attention_gate=True)


@pytest.mark.parametrize('mode', ['replay', 'graph'])
def test_recorded_step_equals_eager(mode):
    """The gate adds plain launches with no per-step host scalars: a launch-list replay and a captured HIP graph of a gated step are the
    eager step, held to the bounds tests/test_gpu_graph.py applies to the plain engine (fp32 storage, learning rate 0 so that the weights
    stay put: losses 2e-5, gradients cos > 0.9999 / rel < 1e-2 -- the order of the float atomics).  The gate's 24 tensors on their own
    (1.4 % of a generator's parameters, behind the longest chains of the step) are compared the way
    test_gpu_fp32.py::test_stream_schedule_does_not_change_gradients compares schedules: against the floor a SECOND eager engine measures
    in the same test, got <= max(20 * floor, 1e-2); a replay that dropped a gate launch would be off by O(1)."""
    from test_gpu_graph import _pair
    from van_gan_amd.vangan import RESULT_KEYS
    from van_gan_amd import VanGan
    eager, other, rI, rS = _pair('fp32', attention_gate=True)
    eager2 = VanGan((32, 32, 32), batch_size=1, device=DEV, seed=3, precision='fp32', attention_gate=True)
    eager2.load_weights(eager.export_weights())
    if mode == 'graph':
        other.capture_train_step()
    for e in (eager, other, eager2):
        e.lr = 0.0
    for step in range(3):
        x, y = (rI, rS) if step % 2 == 0 else (rI.flip(1).contiguous(), rS.flip(2).contiguous())
        re = eager.train_step(x, y)
        eager2.train_step(x, y)
        ro = other.train_step_replay(x, y) if mode == 'replay' else other.train_step_graph(x, y)
        for k in RESULT_KEYS:
            print('   step %d %-24s eager %.6f  %s %.6f' % (step, k, re[k], mode, ro[k]))
            assert abs(re[k] - ro[k]) <= 2e-5 * abs(re[k]) + 1e-7, (step, k, re[k], ro[k])
        # Whole-network gradients.  test_gpu_graph.py holds the plain engine to cos > 0.9999 / rel < 1e-2 between an eager and a recorded
        # engine.  For the gated engine at these weights TWO EAGER engines miss that themselves in some runs (measured, printed below:
        # gen_IS cos 0.99984, rel 1.8e-2, always the same size -- one discrete route of the clDice soft skeleton / min-max taken the other
        # way after a last-bit difference of the forward; other runs 0.99997), so the reference's own spread is measured here by the second
        # eager engine and the recorded step is bounded against it as test_gpu_fp32.py bounds schedules: rel <= max(20 * floor, 1e-2).
        from test_gpu_graph import _cos
        from van_gan_amd.vangan import NETS
        ga, gb, gc = eager.export_grads(), eager2.export_grads(), other.export_grads()
        for n in NETS:
            fa, fb, fc = (torch.cat([t.flatten() for t in g[n].values()]).double() for g in (ga, gb, gc))
            floor, got = float((fa - fb).norm() / fa.norm()), float((fa - fc).norm() / fa.norm())
            print('   step %d %-7s whole network: eager2 vs eager cos %.6f rel %.3e; %s vs eager cos %.6f rel %.3e'
                  % (step, n, _cos(fa, fb), floor, mode, _cos(fa, fc), got))
            assert got <= max(20.0 * floor, 1e-2), (mode, step, n, got, floor)
        ge, go, g2 = eager.export_grads(), other.export_grads(), eager2.export_grads()
        for n in ('gen_IS', 'gen_SI'):
            gate = [k for k in ge[n] if '.gate.' in k]
            assert len(gate) == 24
            fe, fo, f2 = (torch.cat([g[n][k].flatten() for k in gate]).double() for g in (ge, go, g2))
            e, floor = float((fe - fo).norm() / fe.norm()), float((fe - f2).norm() / fe.norm())
            print('   step %d %s gate gradients, %s vs eager: rel %.3e; a second eager engine vs eager: rel %.3e' % (step, n, mode, e, floor))
            assert e <= max(20.0 * floor, 1e-2), (step, n, e, floor)


ARGS = dict(N_DEVICES=1, INPUT_IMG_SIZE=(1, 64, 64, 64, 1), CHANNELS=1, GLOBAL_BATCH_SIZE=1, DIMENSIONS=3, SUBVOL_PATCH_SIZE=(32, 32, 32),
            train_steps=5, BATCH_SIZE=1, output_dir=None)


def test_reference_constructor_use_attention_gate_bf16():
    import argparse
    from van_gan_amd.compat import VanGan
    from van_gan_amd.synth import synth_volumes
    g = VanGan(argparse.Namespace(**ARGS), None, gen_i2s='resUnet', gen_s2i='resUnet', use_attention_gate=True)
    eng = g.eng
    assert eng.attention_gate and eng.gen_IS.attention_gate and eng.gen_SI.attention_gate and eng.precision == 'bf16' and g.use_attention_gate
    rI, rS = synth_volumes(1, 32, 32, 32, seed=3)
    W0 = eng.export_weights()['gen_IS']
    for _ in range(3):
        r = g.distributed_train_step(rI.numpy(), rS.numpy())
        assert len(r) == 10 and all(v == v and abs(v) < 1e6 for v in r.values()), r
    t = g.distributed_test_step(rI.numpy(), rS.numpy())
    assert all(v == v for v in t.values())
    W1 = eng.export_weights()['gen_IS']
    assert all(not torch.equal(W0[k], W1[k]) for k in W0 if '.gate.' in k and k.endswith('.w'))
    # sliding-window inference in both 16-bit storage formats runs the gated forward
    vol = torch.rand(48, 40, 32, 1, generator=torch.Generator().manual_seed(5)) * 2 - 1
    kw = dict(stride=(16, 16, 16), complete=True, padFactor=0.25, process_img=True, window_batch=3)
    outs = {}
    for prec in (None, 'fp16'):
        o = eng.stitch_subvolumes('gen_IS', vol, (32, 32, 32), precision=prec, **kw).float().cpu()
        assert tuple(o.shape[:3]) == (48, 40, 32) and bool(torch.isfinite(o).all())
        outs[prec] = o
    # (the gated forward of generate() / the windows is held to the restatement in fp32 storage by
    #  test_engine_two_steps_test_step_generate_checkpoint_and_replay; here: both 16-bit builds run it and agree within the bound
    #  tests/test_gpu_nets.py states for free-running 16-bit forward volumes, rel_l2 <= 4e-2)
    e = rel_l2(outs['fp16'], outs[None])
    print('sliding-window inference, gated generator: fp16 vs bf16 storage rel_l2 %.3e (0 .. 255 scale)' % e)
    assert e <= 4e-2


RCCL_ONE_AG = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from van_gan_amd.vangan import VanGan
from van_gan_amd.synth import synth_volumes
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
eng = VanGan((32, 32, 32), batch_size=1, n_devices=1, device='cuda:0', seed=4, process_group=dist.group.WORLD, attention_gate=True)
assert eng.sync.active and eng.sync.forced
W0 = eng.export_weights()['gen_IS']
eng.broadcast_weights(0)
rI, rS = synth_volumes(1, 32, 32, 32, seed=5)
res = [eng.distributed_train_step(rI.cuda(), rS.cuda()) for _ in range(3)]
eng._join_updates()
torch.cuda.synchronize()
W = eng.export_weights()['gen_IS']
ok = all(v == v and abs(v) < 1e6 for r in res for v in r.values())
moved = all(not torch.equal(W[k], W0[k]) for k in W if '.gate.' in k and k.endswith('.w'))
torch.save({'ok': ok, 'moved': moved, 'n': len(W)}, %(out)r)
dist.destroy_process_group()
"""


def test_one_rank_process_group_runs_with_the_gate(tmp_path):
    from test_gpu_ddp import _free_port
    out = str(tmp_path / 'rccl1.pt')
    script = tmp_path / 'rccl_one_ag.py'
    script.write_text(RCCL_ONE_AG % dict(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0', VG_DDP_FORCE='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'VG_FAKE_AR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    a = torch.load(out)
    assert a['ok'] and a['moved'] and a['n'] == 140, a
