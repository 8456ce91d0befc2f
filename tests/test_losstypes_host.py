"""Host-side (no GPU) checks of the selectable loss types: known answers of the float64 restatement the GPU tests compare with
(tests/loss_restate.py), the reference-shaped keywords and their validation, and the two entry points' declaration / export / argument
checks."""
import argparse
import math
import os
import re

import pytest
import torch

import loss_restate as R
from oracle import vangan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def _args(**kw):
    d = dict(N_DEVICES=1, INPUT_IMG_SIZE=(1, 64, 64, 64, 1), CHANNELS=1, GLOBAL_BATCH_SIZE=1, DIMENSIONS=3, SUBVOL_PATCH_SIZE=(32, 32, 32),
             train_steps=5, BATCH_SIZE=1, output_dir=None)
    d.update(kw)
    return argparse.Namespace(**d)


def test_entry_points_declared_and_exported():
    from van_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    for name in ('vg_lp_loss', 'vg_logit_loss'):
        assert re.search(r'^int\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name) and name in _lib.EXPORTS


def test_argument_validation_without_gpu():
    from van_gan_amd._lib import lib
    a, b, acc = 1 << 20, 2 << 20, 3 << 20
    for p in (0, 3, 5, -1):
        assert lib.vg_lp_loss(a, b, 64, p, acc, 1.0, None, 0, None) == -1, p
    assert lib.vg_lp_loss(None, b, 64, 1, acc, 1.0, None, 0, None) == -1
    assert lib.vg_lp_loss(a, None, 64, 1, acc, 1.0, None, 0, None) == -1
    assert lib.vg_lp_loss(a, b, 64, 1, None, 1.0, None, 0, None) == -1
    assert lib.vg_lp_loss(a, b, 0, 1, acc, 1.0, None, 0, None) == -1
    for kind in (-1, 2):
        assert lib.vg_logit_loss(a, 1, 1.0, kind, 64, acc, 1.0, None, 0, None) == -1, kind
    for target in (0.5, -1.0, 2.0, float('nan')):
        assert lib.vg_logit_loss(a, 1, target, 0, 64, acc, 1.0, None, 0, None) == -1, target
    assert lib.vg_logit_loss(None, 1, 1.0, 0, 64, acc, 1.0, None, 0, None) == -1
    assert lib.vg_logit_loss(a, 1, 1.0, 0, 64, None, 1.0, None, 0, None) == -1
    assert lib.vg_logit_loss(a, 1, 1.0, 0, 0, acc, 1.0, None, 0, None) == -1


def test_known_answers_of_the_cycle_terms_and_their_scalings():
    """Constant offset c between the volumes, B = 2, global batch size 2, lambda_cycle 10: reduce_mean(axis=list) is a mean per sample,
    summed over the batch, over GBS -- lambda * c^p * B / GBS; reduce_mean(axis=None) includes the batch in the mean -- lambda * v / GBS."""
    cfg = O.Cfg(2, 1)
    g = torch.Generator().manual_seed(1)
    real = torch.rand(2, 4, 4, 4, 1, generator=g, dtype=torch.float64)
    c = 0.3
    cyc = real + c
    assert abs(float(R.cycle_loss(real, cyc, 'mae', cfg)) - 10.0 * c) < 1e-12
    assert abs(float(R.cycle_loss(real, cyc, 'mse', cfg)) - 10.0 * c ** 2) < 1e-12
    assert abs(float(R.cycle_loss(real, cyc, 'L4', cfg)) - 10.0 * c ** 4) < 1e-12
    assert float(R.cycle_loss(real, cyc, 'mse', cfg)) == float(O.mse(real, cyc, cfg.gbs) * cfg.lambda_cycle)
    # a different offset per sample: the per-sample means are summed, not averaged
    cyc2 = real + torch.tensor([0.1, 0.5], dtype=torch.float64).view(2, 1, 1, 1, 1)
    assert abs(float(R.cycle_loss(real, cyc2, 'mae', cfg)) - 10.0 * (0.1 + 0.5) / 2.0) < 1e-12
    assert abs(float(R.cycle_loss(real, cyc2, 'L4', cfg)) - 10.0 * (0.1 ** 4 + 0.5 ** 4) / 2.0) < 1e-12
    # 'bce': min-max normalised volumes, mean over everything INCLUDING the batch, over GBS (the oracle's own SIS term)
    want = O.reduce_mean(O.keras_bce(O.min_max_norm(real), O.min_max_norm(cyc2 * cyc2)), cfg.gbs) * cfg.lambda_cycle
    got = R.cycle_loss(real, cyc2 * cyc2, 'bce', cfg)
    assert float(got) == float(want)
    el = O.keras_bce(O.min_max_norm(real), O.min_max_norm(cyc2 * cyc2))
    assert abs(float(got) - 10.0 * float(el.sum()) / (2 * 64 * 2.0)) < 1e-12
    # global batch size 4 (two replicas): every term halves
    cfg4 = O.Cfg(4, 2)
    for typ in R.CYCLE_TYPES:
        assert abs(float(R.cycle_loss(real, cyc2, typ, cfg4)) - 0.5 * float(R.cycle_loss(real, cyc2, typ, cfg))) < 1e-12
    with pytest.raises(ValueError):
        R.cycle_loss(real, cyc, 'huber', cfg)


def test_sign_of_zero_is_zero_and_the_teacher_forced_mae():
    cfg = O.Cfg(1, 1)
    real = torch.tensor([0.0, 1.0, -1.0, 2.0], dtype=torch.float64).view(1, 4, 1, 1, 1)
    cyc = torch.tensor([0.0, 1.5, -1.0, 1.0], dtype=torch.float64).view(1, 4, 1, 1, 1).requires_grad_(True)
    R.cycle_loss(real, cyc, 'mae', cfg).backward()
    assert cyc.grad.flatten().tolist() == [0.0, 10.0 / 4, 0.0, -10.0 / 4]             # ties: exactly 0
    assert R.sign0(torch.zeros(3)).tolist() == [0.0, 0.0, 0.0]
    # teacher forced: the VALUE is that of the restatement's own volume, the gradient's sign is the teacher's
    teacher = torch.tensor([0.2, 0.5, -1.0, 3.0], dtype=torch.float64).view(1, 4, 1, 1, 1)
    c2 = cyc.detach().clone().requires_grad_(True)
    v = R.cycle_loss(real, c2, 'mae', cfg, teacher=teacher)
    assert float(v.detach()) == float(R.cycle_loss(real, cyc.detach(), 'mae', cfg))
    v.backward()
    assert c2.grad.flatten().tolist() == [10.0 / 4, -10.0 / 4, 0.0, 10.0 / 4]
    # teacher == own volume: the plain gradient
    c3 = cyc.detach().clone().requires_grad_(True)
    R.cycle_loss(real, c3, 'mae', cfg, teacher=cyc.detach()).backward()
    assert torch.equal(c3.grad, cyc.grad)


def test_known_answers_of_the_adversarial_terms():
    z0 = torch.zeros(2, 2, 2, 2, 1, dtype=torch.float64)
    one, zero = torch.ones_like(z0), torch.zeros_like(z0)
    for z in (one, zero):
        assert abs(float(R.bce_logits(z, z0).mean()) - LN2) < 1e-15                       # BCE-from-logits at 0 = ln 2
        assert abs(float(R.focal_logits(z, z0).mean()) - LN2 / 4) < 1e-15                 # focal at 0 = (1/2)^2 ln 2, both targets
    xs = torch.linspace(-90.0, 90.0, 361, dtype=torch.float64)
    assert float((R.softplus(xs) - (torch.clamp(xs, min=0) + torch.log1p(torch.exp(-xs.abs())))).abs().max()) < 1e-13      # the stated form
    # large logits: finite, and the asymptotes (softplus(80) = 80, softplus(-80) = e^-80)
    x = torch.tensor([80.0, -80.0], dtype=torch.float64).view(1, 2, 1, 1, 1)
    for f in (R.bce_logits, R.focal_logits):
        for z in (torch.ones_like(x), torch.zeros_like(x)):
            assert torch.isfinite(f(z, x)).all()
    assert abs(float(R.bce_logits(torch.ones_like(x), x)[0, 1]) - 80.0) < 1e-12
    assert abs(float(R.focal_logits(torch.zeros_like(x), x)[0, 0]) - 80.0) < 1e-12
    # reduce_mean scalings at B = 2, GBS = 2: LSGAN through axis=list (sum of per-sample means / GBS), bce / bfce through axis=None
    cfg = O.Cfg(2, 1)
    d, gl = R.gan_losses(z0, z0, None, cfg)
    assert abs(float(gl) - 1.0) < 1e-15 and abs(float(d) - 0.5) < 1e-15                   # (1-0)^2 per sample, 2 samples / 2; 0.5 (1 + 0)
    d, gl = R.gan_losses(z0, z0, 'bce', cfg)
    assert abs(float(gl) - LN2 / 2) < 1e-15 and abs(float(d) - LN2 / 2) < 1e-15
    d, gl = R.gan_losses(z0, z0, 'bfce', cfg)
    assert abs(float(gl) - LN2 / 8) < 1e-15 and abs(float(d) - LN2 / 8) < 1e-15
    # the default is the oracle's LSGAN pair
    g = torch.Generator().manual_seed(2)
    dr, df = torch.randn(2, 2, 2, 2, 1, generator=g, dtype=torch.float64), torch.randn(2, 2, 2, 2, 1, generator=g, dtype=torch.float64)
    d, gl = R.gan_losses(dr, df, None, cfg)
    assert float(gl) == float(O.mse(torch.ones_like(df), df, cfg.gbs))
    assert float(d) == float(0.5 * (O.mse(torch.ones_like(dr), dr, cfg.gbs) + O.mse(torch.zeros_like(df), df, cfg.gbs)))
    with pytest.raises(ValueError):
        R.gan_losses(dr, df, 'hinge', cfg)


def test_closed_form_gradients_match_autograd():
    """The gradients the kernel evaluates in closed form, against float64 autograd through the restated losses on a grid in [-30, 30]."""
    x = torch.linspace(-30.0, 30.0, 241, dtype=torch.float64)
    for z in (1.0, 0.0):
        xr = x.clone().requires_grad_(True)
        R.focal_logits(torch.full_like(xr, z).unsqueeze(-1), xr.unsqueeze(-1)).sum().backward()
        cf = R.focal_grad_closed_form(x, z)
        err = float((cf - xr.grad).abs().max())
        assert err < 1e-13, (z, err)
        xr = x.clone().requires_grad_(True)
        R.bce_logits(torch.full_like(xr, z).unsqueeze(-1), xr.unsqueeze(-1)).sum().backward()
        assert float((torch.sigmoid(x) - z - xr.grad).abs().max()) < 1e-13                # BCE: s - z


def test_constructor_validation_and_defaults():
    from van_gan_amd import compat
    from van_gan_amd.losstypes import check_loss_types
    a = _args()
    base = compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet')
    same = compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', cycle_loss_SIS='bce', cycle_loss_ISI='mse', gan_loss=None)
    assert same == base and not {'cycle_loss_SIS', 'cycle_loss_ISI', 'gan_loss'} & set(base)      # defaults: the kwargs of before
    kw = compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', cycle_loss_SIS='mae', cycle_loss_ISI='L4', gan_loss='bfce')
    assert (kw['cycle_loss_SIS'], kw['cycle_loss_ISI'], kw['gan_loss']) == ('mae', 'L4', 'bfce')
    assert {k: v for k, v in kw.items() if k in base} == base
    for bad in (dict(cycle_loss_SIS='l1'), dict(cycle_loss_SIS=None), dict(cycle_loss_ISI='MSE'), dict(cycle_loss_ISI='l4'), dict(gan_loss='lsgan'),
                dict(gan_loss='BCE'), dict(gan_loss=0)):
        with pytest.raises(ValueError):
            compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', **bad)
    with pytest.raises(ValueError, match='wasserstein'):
        compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', wasserstein=True, gan_loss='bce')
    with pytest.raises(ValueError, match='wasserstein'):
        check_loss_types('bce', 'mse', 'bfce', wasserstein=True)
    with pytest.raises(ValueError, match='silently'):
        check_loss_types('huber', 'mse', None)
    assert check_loss_types() == ('bce', 'mse', None)
    compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', wasserstein=True, cycle_loss_SIS='mae')      # cycle types combine with it
    with pytest.raises(TypeError):                                    # keyword-only
        compat.engine_kwargs_from_args(a, 10.0, 5, 5, 5, 'resUnet', 'resUnet', False, False, 5, 10.0, False, False, 'mae')
    seen = {}

    class Eng:
        layer_noise, lr, current_epoch, checkpoint_loaded = 0.1, 2e-4, 0, False

        def __init__(self, **k):
            seen.update(k)
            self.gen_IS = self.gen_SI = self.disc_I = self.disc_S = object()
    g = compat.VanGan(a, None, gen_i2s='resUnet', gen_s2i='resUnet', cycle_loss_SIS='L4', cycle_loss_ISI='bce', gan_loss='bce', engine_factory=Eng)
    assert (seen['cycle_loss_SIS'], seen['cycle_loss_ISI'], seen['gan_loss']) == ('L4', 'bce', 'bce')
    assert (g.cycle_loss_SIS, g.cycle_loss_ISI, g.gan_loss) == ('L4', 'bce', 'bce')
    seen.clear()
    compat.VanGan(a, None, gen_i2s='resUnet', gen_s2i='resUnet', engine_factory=Eng)
    assert not {'cycle_loss_SIS', 'cycle_loss_ISI', 'gan_loss'} & set(seen)
    with pytest.raises(ValueError):
        compat.VanGan(a, None, gen_i2s='resUnet', gen_s2i='resUnet', gan_loss='focal', engine_factory=Eng)


def test_default_switches_return_the_oracles_results_exactly():
    dims, B = (32, 32, 32), 1          # the smallest cube the generators' four stride-2 levels take
    P = O.make_models(3, dtype=torch.float64)
    rI, rS = O.synth_volumes(B, *dims, seed=9, dtype=torch.float64)
    cfg = O.Cfg(B, 1, skel_iters=3)
    Pa = {k: {n: t.clone() for n, t in v.items()} for k, v in P.items()}
    Pb = {k: {n: t.clone() for n, t in v.items()} for k, v in P.items()}
    ra, ga, xa = O.train_step(Pa, {}, rI, rS, cfg)
    rb, gb, xb = R.train_step(Pb, {}, rI, rS, cfg, cycle_loss_SIS='bce', cycle_loss_ISI='mse', gan_loss=None)
    assert ra == rb
    for net in ga:
        for n in ga[net]:
            assert torch.equal(ga[net][n], gb[net][n]), (net, n)
            assert torch.equal(Pa[net][n], Pb[net][n]), (net, n)                          # the weights after Adam
    for k in xa:
        assert torch.equal(xa[k], xb[k]), k
    assert R.test_step(P, rI, rS, cfg) == O.test_step(P, rI, rS, cfg)
    # a non-default configuration changes exactly the terms it names
    rc = R.test_step(P, rI, rS, cfg, cycle_loss_SIS='mae', cycle_loss_ISI='bce', gan_loss='bfce')
    ro = O.test_step(P, rI, rS, cfg)
    assert rc['seg_loss'] == ro['seg_loss'] and rc['reconstruction_loss_I'] == ro['reconstruction_loss_I']
    for k in ('cycle_gen_SIS_loss', 'cycle_gen_ISI_loss', 'gen_IS_loss', 'gen_SI_loss', 'D_I_loss', 'D_S_loss'):
        assert rc[k] != ro[k] and math.isfinite(rc[k]), k
