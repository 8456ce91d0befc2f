"""GPU parity of the non-convolution kernels at TRUE SHAPES: one case per InstanceNorm-backward regime, two-job apply, decoder fused
launch, stem shortcut and tanh call that BASELINE configs 2, 3 and 4 make, one per (forward variant, finalisation-tail job shape)
(tests/call_recipes.py; tests/test_call_coverage.py proves the list complete), the finalisation tail under load, the loss chain at the
configs' (B, dims), Adam over the real parameter tables -- each against a float64 restatement on the same rounded operands, computed
with plain torch on the device (the host where the device has no float64 kernel).  Tolerances of tests/test_gpu_ops.py: close_bf16 for
bf16 outputs, relative L2 <= 1e-4 for fp32 outputs, relative error <= 1e-4 for scalar sums, unless stated otherwise.
The recorded calls, the tails under load, the InstanceNorm-backward edges, the loss chain, the skeleton and Adam run inside a guarded
arena (tests/guarded.py): after their parity assertions every guard byte is intact and every input unchanged."""
import math

import pytest
import torch
import torch.nn.functional as F

import call_recipes as CR
import guarded
import layer_recipes as LR

pytestmark = pytest.mark.gpu

_CASES = CR.call_cases()
_IDS = sorted(_CASES, key=lambda k: (_CASES[k]['kind'], k))


def _dev():
    return torch.device('cuda:0')


def _report(name, err):
    print('%-70s %s' % (name, '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))


def _sum_err(got, want):
    return abs(float(got) - float(want)) / (abs(float(want)) + 1e-30)


# ----------------------------------------------------------------------------------------------------------------------
# the recorded calls
# ----------------------------------------------------------------------------------------------------------------------
def _decoder_bytes(blk) -> int:
    """Guarded-arena bytes of _decoder: the concat-wide tensors (the padded gradient, two concat gradients) and, no wider together, dY,
    the sources and their gradients -- budgeted as eight bf16 tensors on the padded grid with all channels -- and 32 small slots."""
    N, (D, H, W) = blk['N'], blk['dims']
    big = 2 * N * (D + 2) * (H + 2) * (W + 2) * (blk['c_low'] + blk['c_skip'])
    return 8 * guarded.slot_cost(big) + 32 * guarded.slot_cost(1 << 20)


def _decoder(blk, dev, arena=None):
    """vg_shortcut_dgrad_concat_norm (served where the split kernel has the shape, else the step's fall-back), vg_shortcut_dgrad_concat and vg_concat_bwd with every accumulate combination, at the
    block's true shape, against float64 (the formulas of tests/test_gpu_ops.py's small-shape cases).
    arena (tests/guarded.py): every tensor a launch reads is a sealed slot of it; dlow / dskip / the concat gradient the fall-back adds
    into are one slot each, reloaded for every launch; verified after each group of launches."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore
    from van_gan_amd.ops import ConvLayer
    N, (D, H, W), cl, cs, cout = blk['N'], blk['dims'], blk['c_low'], blk['c_skip'], blk['cout']
    C_ = cl + cs
    S = D * H * W
    g = torch.Generator(device=dev).manual_seed(17)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    ru = lambda *s: torch.rand(*s, generator=g, device=dev)
    b16 = lambda t: t.to(torch.bfloat16)
    st = ParamStore([('c.w', (1, 1, 1, C_, cout), 'x'), ('c.b', (cout,), 'x')], dev)
    if arena is not None:               # before ConvLayer takes its views
        st.w = arena.out((st.total,), torch.float32, 0.0, name='weights')
        st.g = arena.out((st.total,), torch.float32, 0.0, name='weight gradients')
    st.param('c.w').copy_(rn(1, 1, 1, C_, cout) / math.sqrt(C_))
    lay = ConvLayer(st, 'c', 1, C_, cout, 1, 'same', True, blk['dims'])
    lay.pack()
    put = lambda t, name: t if arena is None else arena.put(t, name=name)
    fresh = lambda t0, name: t0.clone() if arena is None else arena.put(t0, name=name, mutable=True)      # an in/out operand
    reload = lambda t, t0: t0.clone() if arena is None else t.copy_(t0)
    if arena is not None:
        arena.seal(st.w)
    wT = st.param('c.w').to(torch.bfloat16).double().view(C_, cout).t()
    dy = put(b16(rn(N, D, H, W, cout)), 'dy')
    dp1 = put(b16(rn(N, D + 2, H + 2, W + 2, C_)), 'padded gradient')
    low, skip = put(b16(rn(N, D // 2, H // 2, W // 2, cl)), 'low'), put(b16(rn(N, D, H, W, cs)), 'skip')
    gamma, beta = put(ru(C_) + 0.5, 'gamma'), rn(C_) * 0.2
    mean, rstd = put(rn(N, C_) * 0.3, 'mean'), put(ru(N, C_) + 0.5, 'rstd')
    scale = put(gamma.view(1, C_) * rstd, 'scale')
    shift = put(beta.view(1, C_) - mean * scale, 'shift')
    dlow0, dskip0 = b16(rn(N, D // 2, H // 2, W // 2, cl)), b16(rn(N, D, H, W, cs))
    pool = lambda t: t.view(N, D // 2, 2, H // 2, 2, W // 2, 2, -1).sum(dim=(2, 4, 6))
    err = {}
    # 1. the fused launch with the IN backward folded in (as the step runs it: statistics first)
    dgamma, dbeta = LR.dev_out(arena, (C_,), torch.float32, dev, 0.0, 'dgamma'), LR.dev_out(arena, (C_,), torch.float32, dev, 0.0, 'dbeta')
    red = LR.dev_out(arena, (ops.STRIPES * N * C_ * 2 + 4,), torch.float32, dev, 0.0, 'red')
    dlow, dskip = fresh(dlow0, 'dlow'), fresh(dskip0, 'dskip')
    nd = ops.actnorm_desc(dp1, True, low, (N, D, H, W), C_, None, scale=scale, shift=shift, act=ops.ACT_RELU, norm=True, gamma=gamma,
                          mean=mean, rstd=rstd, red=red, accumulate=False, x1=skip, c_x0=cl, x0_shift=1, dgamma=dgamma, dbeta=dbeta)
    ops.actnorm_stats(nd)
    served = lay.dgrad_concat_norm(dy, N, nd, cl, dlow, dskip, acc_low=True, acc_skip=False)
    assert served == blk['served'], 'vg_shortcut_dgrad_concat_norm served: %s' % served
    if not served:              # the step's fall-back: apply pass into a concat-gradient buffer, then the shortcut's data gradient + split
        dcat = LR.dev_out(arena, (N, D, H, W, C_), torch.bfloat16, dev, 7.0, 'concat gradient (fall-back)', must_write=True)
        ops.actnorm_set_dx(nd, dcat)
        ops.actnorm_run(nd, stats_done=True)
        lay.dgrad_concat(dy, N, dcat, cl, dlow, dskip, acc_low=True, acc_skip=False)
    torch.cuda.synchronize()
    x = torch.cat([low.double().repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3), skip.double()], dim=-1)
    z = torch.zeros(N, C_, D, H, W, dtype=torch.float64, device=dev, requires_grad=True)
    (O.reflect_pad1(z) * dp1.double().permute(0, 4, 1, 2, 3)).sum().backward()
    gf = z.grad.permute(0, 2, 3, 4, 1)
    v = lambda t: t.double().view(N, 1, 1, 1, C_)
    dn = gf * ((x * v(scale) + v(shift)) > 0)
    xh = (x - v(mean)) * v(rstd)
    r0, r1 = dn.sum(dim=(1, 2, 3), keepdim=True), (dn * xh).sum(dim=(1, 2, 3), keepdim=True)
    dx = gamma.double().view(1, 1, 1, 1, C_) * v(rstd) * (dn - r0 / S - xh * r1 / S)
    full = dx + dy.double() @ wT
    if not served:              # the fall-back stores the IN backward and then the sum in the bf16 concat gradient
        full = LR.bf(LR.bf(dx) + dy.double() @ wT)
    LR.close_bf16(dlow, pool(full[..., :cl]) + dlow0.double(), 'norm-fused dlow')
    LR.close_bf16(dskip, full[..., cl:], 'norm-fused dskip')
    err['norm_dgamma'], err['norm_dbeta'] = LR.rel_l2(dgamma, r1.sum(0).flatten()), LR.rel_l2(dbeta, r0.sum(0).flatten())
    assert err['norm_dgamma'] <= 1e-4 and err['norm_dbeta'] <= 1e-4, err
    if arena is not None:
        arena.verify()
    del x, z, gf, dn, xh, dx, full
    # 2. the fused shortcut data gradient + concat backward (the fall-back of 1): dcat is only read
    dcat0 = b16(rn(N, D, H, W, C_))
    dcat = fresh(dcat0, 'concat gradient')
    full = dcat.double() + dy.double() @ wT
    for acc_low, acc_skip in ((False, False), (True, True)):
        dlow, dskip, dcat = reload(dlow, dlow0), reload(dskip, dskip0), reload(dcat, dcat0)
        lay.dgrad_concat(dy, N, dcat, cl, dlow, dskip, acc_low=acc_low, acc_skip=acc_skip)
        torch.cuda.synchronize()
        assert torch.equal(dcat, dcat0) == blk['served'], 'the fused launch only reads the concat gradient; the fall-back adds into it'
        LR.close_bf16(dlow, pool(full[..., :cl]) + (dlow0.double() if acc_low else 0), 'concat-fused dlow')
        LR.close_bf16(dskip, full[..., cl:] + (dskip0.double() if acc_skip else 0), 'concat-fused dskip')
    if arena is not None:
        arena.verify()
    # 3. vg_concat_bwd on its own, every accumulate combination
    dcat = dcat0 if arena is None else arena.seal(reload(dcat, dcat0))           # only read from here on
    for acc in range(4):
        dlow, dskip = reload(dlow, dlow0), reload(dskip, dskip0)
        ops.concat_bwd(dcat, (N, D, H, W), cl, cs, dlow, dskip, acc_low=bool(acc & 1), acc_skip=bool(acc & 2))
        torch.cuda.synchronize()
        LR.close_bf16(dlow, pool(dcat.double()[..., :cl]) + (dlow0.double() if acc & 1 else 0), 'concat_bwd dlow')
        LR.close_bf16(dskip, dcat.double()[..., cl:] + (dskip0.double() if acc & 2 else 0), 'concat_bwd dskip')
    if arena is not None:
        arena.verify()
    return err


def _stem_fwd(N, S, C_, dev, x=None, seed=21, arena=None):
    from van_gan_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    if x is None:
        x = torch.rand(N, S, 1, generator=g, device=dev) * 2 - 1
        x[N - 1] = x[N - 1] * 0.3 + 0.5
    w = torch.randn(C_, generator=g, device=dev) * 0.4
    w[3] = 0.01
    gam, bet = torch.rand(C_, generator=g, device=dev) + 0.5, torch.randn(C_, generator=g, device=dev) * 0.1
    sc, sh = (LR.dev_out(arena, (N, C_), torch.float32, dev, 0.0, k, must_write=True) for k in ('scale', 'shift'))
    if arena is not None:               # the kernel's own partial sums stay in the ops.Arena it takes them from
        x, w, gam, bet = arena.put(x, name='x'), arena.put(w, name='w'), arena.put(gam, name='gamma'), arena.put(bet, name='beta')
    ar = ops.Arena(64 << 20, dev)
    ops.stem_short_fwd(ar, x, N, C_, w, gam, bet, sc, sh, round16=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
    xd = x.double().view(N, S)
    mu, var = xd.mean(1), xd.var(1, unbiased=False)
    wq = w.to(torch.bfloat16).double()
    rs = (wq[None] ** 2 * var[:, None] + ops.IN_EPS).rsqrt()
    ref_sc = gam.double()[None] * wq[None] * rs
    ref_sh = bet.double()[None] - ref_sc * mu[:, None]
    err = dict(scale=LR.rel_l2(sc, ref_sc), shift=LR.rel_l2(sh, ref_sh))
    assert err['scale'] <= 1e-5 and err['shift'] <= 1e-5, err
    if arena is not None:
        arena.verify()
    return err


def _stem_bwd(N, S, C_, dev, seed=22, arena=None):
    """vg_stem_short_bwd (d/dw, d/dgamma, d/dbeta of  IN(w x + b)  in two moments) against float64 autograd of the same expression."""
    from van_gan_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(N, S, 1, generator=g, device=dev) * 2 - 1
    gy = torch.randn(N, S, C_, generator=g, device=dev).to(torch.bfloat16)
    w = torch.randn(C_, generator=g, device=dev) * 0.4
    gam = torch.rand(C_, generator=g, device=dev) + 0.5
    dw, dgam, dbet = (LR.dev_out(arena, (C_,), torch.float32, dev, 0.0, k) for k in ('dw', 'dgamma', 'dbeta'))
    if arena is not None:
        x, gy, w, gam = arena.put(x, name='x'), arena.put(gy, name='gy'), arena.put(w, name='w'), arena.put(gam, name='gamma')
    ar = ops.Arena(64 << 20, dev)
    ops.stem_short_bwd(ar, gy, x, N, C_, w, gam, dw, dgam, dbet, round16=True)
    torch.cuda.synchronize()
    wr = w.to(torch.bfloat16).double().requires_grad_(True)
    gr = gam.double().requires_grad_(True)
    br = torch.zeros(C_, dtype=torch.float64, device=dev, requires_grad=True)
    y = x.double() * wr.view(1, 1, C_)
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    out = (y - mu) * (var + ops.IN_EPS).rsqrt() * gr.view(1, 1, C_) + br.view(1, 1, C_)
    (out * gy.double()).sum().backward()
    err = dict(dw=LR.rel_l2(dw, wr.grad), dgamma=LR.rel_l2(dgam, gr.grad), dbeta=LR.rel_l2(dbet, br.grad))
    assert max(err.values()) <= 1e-4, err
    if arena is not None:
        arena.verify()
    return err


def _flat_arena(nbytes, slots, dev):
    """A guarded arena for `slots` tensors of `nbytes` bytes together."""
    return guarded.GuardedArena(nbytes + slots * guarded.slot_cost(0), dev)


def run_case(c, cid, dev):
    """One case of call_recipes.cases_of on the device (tests/test_gpu_ragged.py and tests/test_gpu_batch3.py run their own lists through
    here too), inside a guarded arena (tests/guarded.py): the parity assertions of the case, then every guard intact and every input
    unchanged."""
    from van_gan_amd import ops
    kind = c['kind']
    if kind == 'anb':
        r = dict(c['regime'])
        err = CR.run_anb(r, dev, name=cid, arena=guarded.GuardedArena(CR.anb_bytes(r), dev))
    elif kind == 'apply2':
        r1, r2 = dict(c['regime'][0][1]), dict(c['regime'][1][1])
        err = CR.run_apply2(r1, r2, dev, name=cid, arena=guarded.GuardedArena(CR.anb_bytes(r1) + CR.anb_bytes(r2), dev))
    elif kind == 'decoder':
        err = _decoder(c['block'], dev, arena=guarded.GuardedArena(_decoder_bytes(c['block']), dev))
    elif kind == 'fin':
        err = dict(fin=CR.run_fin(c['recipe'], c['variant'], dev, arena=LR.guarded_for(c['recipe'], dev)))
    elif kind == 'stem_short_fwd':
        r = dict(c['regime'])
        assert r['G'] == int(ops.lib.vg_stem_short_fwd_workgroups(r['N'], r['S']))
        err = _stem_fwd(r['N'], r['S'], r['C'], dev, arena=_flat_arena(4 * r['N'] * r['S'] + 64 * r['N'] * r['C'], 8, dev))
    elif kind == 'stem_short_bwd':
        r = dict(c['regime'])
        assert r['G'] == int(ops.lib.vg_stem_short_bwd_workgroups(r['N'], r['S'], r['C']))
        err = _stem_bwd(r['N'], r['S'], r['C'], dev, arena=_flat_arena(4 * r['N'] * r['S'] * (1 + r['C']), 8, dev))
    else:
        assert kind == 'tanh_bwd'
        n = dict(c['regime'])['n']
        ga = _flat_arena(12 * n, 3, dev)
        g = torch.Generator(device=dev).manual_seed(23)
        y, dy = torch.tanh(torch.randn(n, generator=g, device=dev) * 2), torch.randn(n, generator=g, device=dev)
        y, dy = ga.put(y, name='y'), ga.put(dy, name='dy')
        dp = ga.out((n,), torch.float32, None, name='dpre')           # 0xFF bytes: NaN, as before
        ops.tanh_bwd(dy, y, dp)
        torch.cuda.synchronize()
        err = dict(dpre=LR.rel_l2(dp, dy.double() * (1 - y.double() ** 2)))
        assert err['dpre'] <= 1e-6
        ga.verify()
    _report(cid, err)
    return err


@pytest.mark.parametrize('cid', _IDS)
def test_recorded_call_matches_float64(cid):
    run_case(_CASES[cid], cid, _dev())


@pytest.mark.parametrize('fam', sorted(CR.fin_stress_cases()))
def test_finalisation_tail_under_load(fam):
    c = CR.fin_stress_cases()[fam]
    w = CR.stress_fin(c['recipe'], c['variant'], _dev(), launches=200, arena=LR.guarded_for(c['recipe'], _dev()))
    _report('fin under load %s %s' % (fam, c['variant']), dict(worst=w))


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm backward beyond the configs
# ----------------------------------------------------------------------------------------------------------------------
def _anb(**kw):
    r = dict(N=2, D=8, H=8, W=8, C=16, g_padded=1, f32=0, x_f32=0, c_x0=0, x0_shift=0, act=1, norm=1, alias_n0=0, alias_shift=0, pgrad_n=0,
             dx_f32=0, accumulate=0, dx_cstride=0, dx_coff=0, has_x=1, has_x1=0, has_scale=1, has_mult=0, has_dgamma=1)
    r.update(kw)
    return r


_ANB_EXTRA = {
    'double mirror 3x3x3': _anb(D=3, H=3, W=3, C=24),
    'double mirror 2x3x2 C8': _anb(D=2, H=3, W=2, C=8, act=2, has_mult=1),
    'padded 4x2x6 concat': _anb(D=4, H=2, W=6, C=48, c_x0=32, x0_shift=1, has_x1=1),
    'ragged 37x19x9': _anb(D=37, H=19, W=9, C=32, act=2),
    'ragged 37x19x9 unpadded alias': _anb(N=3, D=37, H=19, W=9, C=64, g_padded=0, act=2, has_mult=1, alias_n0=2, alias_shift=1, pgrad_n=2),
    'fp32 C=1 (VEC=1)': _anb(N=2, D=33, H=20, W=17, C=1, f32=1, x_f32=1, dx_f32=1, norm=0, act=0, has_x=0, has_scale=0, has_dgamma=0),
    'fp32 C=1 IN + LeakyReLU': _anb(N=2, D=17, H=20, W=33, C=1, f32=1, x_f32=1, dx_f32=1, act=2),
    'capped grid, many voxels per thread': _anb(N=1, D=96, H=128, W=160, C=64, act=2),
    'accumulate into bf16, strided dx': _anb(N=2, D=24, H=20, W=28, C=16, accumulate=1, dx_cstride=48, dx_coff=16),
    'accumulate into bf16': _anb(N=2, D=64, H=64, W=64, C=32, accumulate=1),
}


@pytest.mark.parametrize('name', sorted(_ANB_EXTRA))
def test_instance_norm_backward_edges(name):
    err = CR.run_anb(_ANB_EXTRA[name], _dev(), seed=3, name=name, arena=guarded.GuardedArena(CR.anb_bytes(_ANB_EXTRA[name]), _dev()))
    _report('anb ' + name, err)


def test_apply2_jobs_of_different_grids():
    """The two jobs of one apply2 launch with different grids (job 2 strides by its own workgroup count)."""
    r1 = _anb(N=2, D=40, H=24, W=16, C=32, g_padded=0, act=0)
    r2 = _anb(N=2, D=40, H=24, W=16, C=96, g_padded=1)
    err = CR.run_apply2(r1, r2, _dev(), seed=4, name='apply2 C32 + C96', arena=guarded.GuardedArena(CR.anb_bytes(r1) + CR.anb_bytes(r2), _dev()))
    _report('apply2 C32 unpadded + C96 padded', err)


# ----------------------------------------------------------------------------------------------------------------------
# small ones: in_finalize with two sources and dropout, affine_add at the ResNet generator's shapes
# ----------------------------------------------------------------------------------------------------------------------
def test_in_finalize_two_sources_and_mult():
    from van_gan_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(31)
    N, c0, c1, cnt0, cnt1 = 3, 32, 16, 4096.0, 512.0
    sums0 = torch.rand(8, N, c0, 2, generator=g, device=dev)
    sums0[..., 0] = sums0[..., 0] * 200 - 100
    sums0[..., 1] = sums0[..., 1] * 4000 + 4000
    sums1 = torch.rand(8, N, c1, 2, generator=g, device=dev)
    sums1[..., 0] = sums1[..., 0] * 40 - 20
    sums1[..., 1] = sums1[..., 1] * 500 + 300
    gam, bet = torch.rand(c0 + c1, generator=g, device=dev) + 0.5, torch.randn(c0 + c1, generator=g, device=dev) * 0.2
    mult = (torch.rand(N, c0 + c1, generator=g, device=dev) > 0.3).float() * 2.0
    ga = _flat_arena(1 << 20, 9, dev)                 # operands sealed, the four outputs 0xFF bytes (NaN, as before)
    sums0, sums1, gam, bet, mult = (ga.put(t, name=k) for k, t in (('sums0', sums0), ('sums1', sums1), ('gamma', gam), ('beta', bet), ('mult', mult)))
    out = [ga.out((N, c0 + c1), torch.float32, None, name=k) for k in ('scale', 'shift', 'mean', 'rstd')]
    ops.in_finalize(sums0, c0, cnt0, gam, bet, N, *out, sums1=sums1, c1=c1, count1=cnt1, mult=mult)
    torch.cuda.synchronize()
    s = torch.cat([sums0.double().sum(0) / cnt0, sums1.double().sum(0) / cnt1], dim=1)
    mean, var = s[..., 0], (s[..., 1] - s[..., 0] ** 2).clamp_min(0)
    rstd = (var + ops.IN_EPS).rsqrt()
    sc = gam.double() * rstd
    ref = (sc * mult, (bet.double() - mean * sc) * mult, mean, rstd)
    err = {k: LR.rel_l2(o, r) for k, o, r in zip(('scale', 'shift', 'mean', 'rstd'), out, ref)}
    _report('in_finalize two sources + mult', err)
    assert max(err.values()) <= 1e-5, err
    ga.verify()


@pytest.mark.parametrize('dims,C_,act,f32', [((32, 32, 32), 256, 0, False), ((32, 32, 32), 256, 1, False), ((64, 64, 64), 128, 1, False),
                                             ((16, 16, 16), 256, 1, True)])
def test_affine_add_at_resnet_shapes(dims, C_, act, f32):
    """out = act(a * sa + ha) + (b * sb + hb): the residual Add of the ResNet generator's trunk (256 channels at a quarter of the patch)."""
    from van_gan_amd import ops
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(32)
    N, S = 1, math.prod(dims)
    dt = torch.float32 if f32 else torch.bfloat16
    ga = _flat_arena(3 * 4 * N * S * C_ + (1 << 20), 7, dev)
    a, b = ga.put(torch.randn(N, S, C_, generator=g, device=dev).to(dt), name='a'), ga.put(torch.randn(N, S, C_, generator=g, device=dev).to(dt), name='b')
    sa, ha, sb, hb = [ga.put(torch.randn(N, C_, generator=g, device=dev), name=k) for k in ('sa', 'ha', 'sb', 'hb')]
    out = ga.out((N, S, C_), dt, None, name='out')                    # 0xFF bytes: NaN, as before
    ops.affine_add(a, sa, ha, act, b, sb, hb, N, S, C_, out)
    torch.cuda.synchronize()
    pa = a.double() * sa.double().view(N, 1, C_) + ha.double().view(N, 1, C_)
    ref = (F.relu(pa) if act == ops.ACT_RELU else pa) + b.double() * sb.double().view(N, 1, C_) + hb.double().view(N, 1, C_)
    if f32:
        assert LR.rel_l2(out, ref) <= 1e-6
    else:
        LR.close_bf16(out, ref, 'affine_add')
    ga.verify()


# ----------------------------------------------------------------------------------------------------------------------
# stem shortcut: near-constant volumes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['1 + 1e-3 noise', 'constant'])
def test_stem_shortcut_on_a_near_constant_volume(kind):
    """the variance of the volume is E[x^2] - mu^2 of fp32 wave partials; on a (near-)constant volume the scale and shift
    must stay finite and match float64 (IN_EPS keeps the constant case well defined)."""
    dev = _dev()
    N, S = 2, 128 ** 3
    g = torch.Generator(device=dev).manual_seed(24)
    x = torch.ones(N, S, 1, device=dev)
    if kind != 'constant':
        x = x + 1e-3 * torch.randn(N, S, 1, generator=g, device=dev)
    err = _stem_fwd(N, S, 16, dev, x=x, arena=_flat_arena(4 * N * S + 64 * N * 16, 8, dev))
    _report('stem_short_fwd ' + kind, err)


# ----------------------------------------------------------------------------------------------------------------------
# the loss chain at the configs' (B, dims)
# ----------------------------------------------------------------------------------------------------------------------
_LOSS_SHAPES = {'128^3 B1': (1, (128, 128, 128)), '64^3 B2': (2, (64, 64, 64)), '128x128x64 B2': (2, (128, 128, 64)),
                '32^3 B1': (1, (32, 32, 32)), 'odd S B2': (2, (33, 35, 37)),
                # the reference's own per-GPU batch: samples 1 and 2 of an odd S start on different alignments (S and 2S are no multiples of 4)
                '32^3 B3': (3, (32, 32, 32)), 'odd S B3': (3, (33, 35, 37))}


def _ssim_ref(t, p):
    """float64 SSIM loss and its gradient through the oracle (on the device; the host if the device has no float64 convolution)."""
    from oracle import vangan_oracle as O
    for dev in (t.device, torch.device('cpu')):
        try:
            pr = p.double().to(dev).requires_grad_(True)
            ls = O.ssim_loss_3d(t.double().to(dev), pr).sum()
            ls.backward()
            return float(ls), pr.grad
        except RuntimeError:
            if dev.type == 'cpu':
                raise
    raise AssertionError


@pytest.mark.parametrize('cfg', sorted(_LOSS_SHAPES))
def test_loss_chain_at_config_shapes(cfg):
    """min-max (two ties of the min and of the max further apart than the reduction grid, so the tie counts add across workgroups; an odd
    S puts samples 1 and 2 on unaligned starts and their extrema in the scalar tail) -> BCE (p exactly 0 and 1 at the arg-extrema: clipped,
    zero gradient) -> min-max backward; MSE, MSE against a constant on bf16 logits; SSIM loss and gradient (faces and edges included).
    Every device tensor is a slot of a guarded arena (tests/guarded.py), filled as before (zeros stay zeros, NaN is 0xFF bytes): after
    each group of launches every guard intact and every input unchanged."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    dev = _dev()
    B, (D, H, W) = _LOSS_SHAPES[cfg]
    S = D * H * W
    g = torch.Generator(device=dev).manual_seed(41)
    x = torch.tanh(torch.randn(B, S, generator=g, device=dev) * 2)
    for b in range(B):
        hi, lo = float(x[b].max()) + 0.25, float(x[b].min()) - 0.25
        far = (S - 1, 5) if (b >= 1 and S % 4) else (3, S - 700)              # samples >= 1 of an odd S: extrema in the scalar tail
        x[b, far[0]] = hi; x[b, far[1]] = hi
        x[b, S // 2 + 1] = lo; x[b, S - 2 if b >= 1 else 1] = lo
    ga = _flat_arena(24 * 4 * B * S, 32, dev)
    vol = (B, D, H, W, 1)
    zeros = lambda shape, name: ga.out(shape, torch.float32, 0.0, name=name)
    x = ga.put(x.view(vol).contiguous(), name='x')
    t = ga.put((torch.rand(vol, generator=g, device=dev) > 0.7).float(), name='t')
    mm, y = zeros((B, 4), 'mm'), zeros(vol, 'y')
    ops.minmax(x, B, S, mm)
    ops.minmax_apply(x, mm, B, S, y)
    acc = zeros((8,), 'acc')
    gy = zeros(vol, 'gy')
    ops.bce(t, y, acc[0:1], 0.37, gy)
    dx, tmp2 = zeros(vol, 'dx'), zeros((B, 2), 'tmp2')
    ops.minmax_bwd(x, y, gy, mm, B, S, tmp2, dx)
    torch.cuda.synchronize()
    assert mm[:, 2].tolist() == [2.0] * B and mm[:, 3].tolist() == [2.0] * B, mm       # tie counts
    xr = x.double().requires_grad_(True)
    yr = O.min_max_norm(xr)
    lb = O.keras_bce(t.double(), yr).sum()
    (0.37 * lb).backward()
    err = dict(minmax=LR.rel_l2(y, yr.detach()), bce=_sum_err(acc[0], lb), minmax_bwd=LR.rel_l2(dx, xr.grad))
    assert float(y.min()) == 0.0 and float(y.max()) == 1.0
    assert err['minmax'] <= 1e-6 and err['bce'] <= 1e-4, err
    assert err['minmax_bwd'] <= 5e-3, err           # the bound the 480-voxel case meets (tests/test_gpu_ops.py)
    ga.verify()
    del xr, yr
    # MSE and the LSGAN constant
    a, b_ = ga.put(torch.randn(B, S, generator=g, device=dev), name='a'), ga.put(torch.randn(B, S, generator=g, device=dev), name='b')
    gb = ga.out((B, S), torch.float32, None, name='gb')                 # 0xFF bytes: NaN
    ops.mse(a, b_, acc[1:2], 0.5, gb)
    bl = ga.put(b_.to(torch.bfloat16), name='b (bf16)')
    gx = ga.out((B, S), torch.float32, None, name='gx')
    ops.mse_const(bl, 1.0, acc[2:3], 2.0, gx)
    torch.cuda.synchronize()
    ga.verify()
    ad, bd, bld = a.double(), b_.double(), bl.double()
    err.update(mse=_sum_err(acc[1], ((ad - bd) ** 2).sum()), mse_grad=LR.rel_l2(gb, 0.5 * 2 * (bd - ad)),
               mse_const=_sum_err(acc[2], ((bld - 1) ** 2).sum()), mse_const_grad=LR.rel_l2(gx, 4 * (bld - 1)))
    assert err['mse'] <= 1e-4 and err['mse_const'] <= 1e-4 and err['mse_grad'] <= 1e-5 and err['mse_const_grad'] <= 1e-5, err
    # SSIM
    p, tt = ga.put(torch.rand(vol, generator=g, device=dev), name='p'), ga.put(torch.rand(vol, generator=g, device=dev), name='tt')
    part, gp = zeros((3,) + vol, 'part'), zeros(vol, 'gp')
    ops.ssim_fwd(tt, p, (B, D, H, W), acc[3:4], part)
    ops.ssim_bwd(tt, p, part, (B, D, H, W), 1.0, gp)
    torch.cuda.synchronize()
    ga.verify()
    ls, gref = _ssim_ref(tt, p)
    gref = gref.to(dev)
    err['ssim'] = _sum_err(acc[3], ls)
    err['ssim_grad'] = LR.rel_l2(gp, gref)
    face = torch.zeros(B, D, H, W, 1, dtype=torch.bool, device=dev)
    face[:, [0, -1]] = True; face[:, :, [0, -1]] = True; face[:, :, :, [0, -1]] = True
    err['ssim_grad_faces'] = LR.rel_l2(gp[face], gref[face])
    _report('losses ' + cfg, err)
    assert err['ssim'] <= 1e-4 and err['ssim_grad'] <= 1e-3 and err['ssim_grad_faces'] <= 1e-3, err


@pytest.mark.parametrize('cfg', ['128^3 B1', '64^3 B2', '128x128x64 B2', '32^3 B1', '32^3 B3'])
def test_skeleton_and_cldice_at_config_shapes(cfg):
    """soft skeleton (15 iterations, with and without the aux codes) -> dot_sums -> clDice coefficients and gradients, against float64
    autograd through the oracle on continuous data; and an all-zero target (empty skeleton: only the smooth terms).
    Every device tensor of the launches is a slot of a guarded arena (tests/guarded.py), filled as before; guards and inputs are verified
    after the launches of each target."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    dev = _dev()
    B, dims = _LOSS_SHAPES[cfg]
    D, H, W = dims
    it = 15
    vol = (B, D, H, W, 1)
    g = torch.Generator(device=dev).manual_seed(42)
    p = torch.rand(vol, generator=g, device=dev)
    t_ = (F.avg_pool3d(torch.rand(B, 1, D, H, W, generator=g, device=dev), 3, 1, 1) > 0.52).float().permute(0, 2, 3, 4, 1).contiguous()
    for empty in (False, True):
        nv = B * D * H * W
        n_aux = ops.skel_aux_bytes((B, D, H, W), it)
        ga = _flat_arena(4 * nv * (2 * (2 * it + 3) + 7 + 6) + n_aux, 24, dev)
        zeros = lambda shape, name: ga.out(shape, torch.float32, 0.0, name=name)
        t = ga.put(torch.zeros_like(t_) if empty else t_, name='t')
        pa = ga.put(p, name='p')
        imgs_p, skels_p = zeros((it + 2,) + vol, 'imgs_p'), zeros((it + 1,) + vol, 'skels_p')
        imgs_t, skels_t = zeros((it + 2,) + vol, 'imgs_t'), zeros((it + 1,) + vol, 'skels_t')
        aux = ga.out((n_aux,), torch.uint8, 0, name='aux')
        ops.soft_skel_fwd(pa, (B, D, H, W), it, imgs_p, skels_p, aux)
        ops.soft_skel_fwd(t, (B, D, H, W), it, imgs_t, skels_t)
        sums, coef = zeros((9,), 'sums'), zeros((8,), 'coef')
        ops.dot_sums(skels_p[it], t, sums[0:3]); ops.dot_sums(skels_t[it], pa, sums[3:6]); ops.dot_sums(t, pa, sums[6:9])
        w = 5.0
        ops.cldice_coef(sums, w, 0.5, coef)
        gskel, gp = zeros(vol, 'gskel'), zeros(vol, 'gp')
        ops.cldice_grads(t, skels_t[it], coef, gskel, gp)
        torch.cuda.synchronize()
        for k in (imgs_p, skels_p, imgs_t, skels_t, aux, coef, gskel):            # written above, only read from here on
            ga.seal(k)
        gp0 = ga.put(gp, name='gp0', mutable=True)
        work = ga.out((4,) + vol, torch.float32, None, name='work')              # 0xFF bytes: NaN
        ops.soft_skel_bwd(imgs_p, skels_p, gskel, (B, D, H, W), it, work, gp, aux)
        work3 = zeros((3,) + vol, 'work3')
        ops.soft_skel_bwd(imgs_p, skels_p, gskel, (B, D, H, W), it, work3, gp0)
        torch.cuda.synchronize()
        ga.verify()
        pr = p.double().requires_grad_(True)
        sk_p = O.soft_skel(pr[..., 0], it)
        sk_t = O.soft_skel(t.double()[..., 0], it)
        td, pd = t.double()[..., 0], p.double()[..., 0]
        ref_sums = [(sk_p * td).sum(), sk_p.sum(), td.sum(), (sk_t * pd).sum(), sk_t.sum(), pd.sum(), (td * pd).sum(), td.sum(), pd.sum()]
        loss = O.soft_dice_cldice(t.double(), pr, it) * w
        loss.backward()
        err = dict(skel=LR.rel_l2(skels_p[it][..., 0], sk_p.detach()), coef=_sum_err(coef[5], loss), grad_aux=LR.rel_l2(gp, pr.grad),
                   grad_scan=LR.rel_l2(gp0, pr.grad))
        err['dot_sums'] = max(_sum_err(sums[i], ref_sums[i]) for i in range(9) if abs(float(ref_sums[i])) > 0)
        if empty:
            assert float(sums[0]) == 0.0 and float(sums[3]) == 0.0 and float(sums[4]) == 0.0
        _report('skeleton + clDice %s%s' % (cfg, ' empty target' if empty else ''), err)
        assert err['skel'] <= 1e-6 and err['coef'] <= 1e-4 and err['dot_sums'] <= 1e-4, err
        assert err['grad_aux'] <= 1e-3 and err['grad_scan'] <= 1e-3, err


# ----------------------------------------------------------------------------------------------------------------------
# Adam over the real parameter tables
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', ['gen', 'disc', 'resnet'])
def test_adam_over_the_real_tables(net):
    """vg_adam_clip / vg_adam_clip_dev over a network's flat table as ParamStore lays it out (4096-element spans that start inside, at
    the start of and at the end of tensors), 3 steps with some tensors clipped and grad_scale != 1, against float64; and the fixed-order
    norm sums: a repeat reproduces the result bit for bit."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, disc_param_specs, gen_param_specs, resnet_param_specs
    dev = _dev()
    specs = {'gen': gen_param_specs, 'disc': disc_param_specs, 'resnet': resnet_param_specs}[net]()
    st = ParamStore(specs, dev)
    # the store's tables as slots of a guarded arena (tests/guarded.py): weights, gradients, both Adam slots, the segment table and the
    # norms[T + 2 * ceil(total / 4096)] block at exactly its documented length
    assert st.norms.numel() == st.T + 2 * ((st.total + 4095) // 4096)
    ga = _flat_arena(16 * st.total + 8 * (st.T + 1) + 4 * st.norms.numel(), 8, dev)
    st.w, st.g, st.m, st.v = (ga.out((st.total,), torch.float32, 0.0, name=k) for k in ('w', 'g', 'm', 'v'))
    st.seg_off, st.norms = ga.put(st.seg_off, name='seg_off'), ga.out((st.norms.numel(),), torch.float32, 0.0, name='norms')
    off = st.seg_off.cpu().tolist()
    assert any(o % 4096 for o in off[1:-1]) and any((a // 4096) != ((b - 1) // 4096) for a, b in zip(off[:-1], off[1:]))
    assert net != 'disc' or any(o % 4096 == 0 for o in off[1:-1])        # spans inside, across and (disc) at the start of tensors
    g = torch.Generator().manual_seed(51)
    P = {n: torch.randn(sh, generator=g) * 0.05 for n, sh, _ in specs}
    G = {n: torch.randn(sh, generator=g) * 0.01 for n, sh, _ in specs}
    big = sorted(P, key=lambda n: -P[n].numel())
    for n in big[:3] + big[-3:]:
        G[n] = G[n] * (400.0 / float(G[n].norm()))                         # norm 400 * grad_scale > 100: clipped (large and small tensors)
    scale = 0.75
    lr_dev = torch.zeros(1, device=dev)

    def run(use_dev):
        st.load(P); st.m.zero_(); st.v.zero_()
        for step in range(1, 4):
            for n in P:
                st.grad(n).copy_(G[n])
            lr_t = 2e-4 * math.sqrt(1 - 0.9 ** step) / (1 - 0.5 ** step)
            if use_dev:
                lr_dev.fill_(lr_t)
                ops.adam_clip_dev(st.w, st.g, st.m, st.v, st.seg_off, st.T, st.norms, lr_dev.data_ptr(), 0.5, 0.9, 1e-7, 100.0, grad_scale=scale)
            else:
                ops.adam_clip(st.w, st.g, st.m, st.v, st.seg_off, st.T, st.norms, lr_t, 0.5, 0.9, 1e-7, 100.0, grad_scale=scale)
        torch.cuda.synchronize()
        return st.w.clone()

    w_host = run(False)
    got = st.export()
    Pd, state = {n: v.double() for n, v in P.items()}, {}
    for step in range(3):
        O.adam_step(Pd, {n: v.double() * scale for n, v in G.items()}, state)
    clipped = sum(1 for n in P if float((G[n].double() * scale).norm()) > 100.0)
    assert clipped >= 6
    e = max(float((got[n].double().cpu() - Pd[n]).abs().max()) for n in P)
    _report('adam %s (%d tensors, %d clipped)' % (net, len(specs), clipped), dict(max_abs=e))
    assert e < 1e-6
    w_dev = run(True)
    assert torch.equal(w_dev, w_host), 'adam_clip_dev (rate from device memory) differs from adam_clip'
    assert torch.equal(run(False), w_host), 'not reproducible bit for bit'
    ga.verify()
