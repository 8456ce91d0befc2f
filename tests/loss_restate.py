"""Restatement of the reference's selectable loss types in torch -- test infrastructure only, composed from the oracle's own pieces
(oracle.vangan_oracle: reduce_mean, min_max_norm, keras_bce, mse, ssim_loss_3d, soft_dice_cldice, the network forwards).  The oracle
states the one configuration the reference's VanGan hard-codes (vangan.py:302,306,329-332); this file states the other live branches:

    cycle_loss(typ=None | "mse" | "L4" | "bce")                       loss_functions.py:163-190   (None is spelt 'mae' here)
    generator_loss_fn / discriminator_loss_fn(typ=None | "bce" | "bfce", from_logits=True)   :255-322

MAE / MSE / L4 take the RAW volumes through reduce_mean(axis=list); 'bce' min-max normalises both volumes and goes through
reduce_mean(axis=None); the adversarial 'bce' / 'bfce' go through reduce_mean(axis=None) as well.

TP (Keras 2.10, restated from its definition -- TensorFlow is not available to check against), per element, then the mean over the
channel axis that Reduction.NONE leaves to the loss object:
    BinaryCrossentropy(from_logits=True)(z, x)      = max(x, 0) - x z + log1p(exp(-|x|))
    BinaryFocalCrossentropy(from_logits=True)(z, x) = (1 - p_t)^2 * bce,  p_t = z s + (1 - z)(1 - s),  s = sigmoid(x)  (gamma 2, no balancing)
With the default switches compute_losses / train_step perform the oracle's operations in the oracle's order: the same numbers.
"""
from typing import Dict, Optional

import torch

from oracle import vangan_oracle as O

Tensor = torch.Tensor
CYCLE_TYPES = ('mae', 'mse', 'L4', 'bce')
GAN_TYPES = (None, 'bce', 'bfce')


def sign0(d: Tensor) -> Tensor:
    """TP: the gradient of tf.abs is sign(x) with sign(0) = 0 (torch.sign agrees)."""
    return torch.sign(d)


def _axes(x: Tensor):
    return tuple(range(1, x.dim()))


def cycle_loss(real: Tensor, cycled: Tensor, typ: str, cfg, teacher: Optional[Tensor] = None) -> Tensor:
    """cycle_loss(self, real, cycled, typ) times lambda_cycle.  teacher (only read for 'mae'): the cycled volume of the implementation
    under test; the term's VALUE stays mean |real - cycled|, its backward uses sign(teacher - real) as a constant instead of
    sign(cycled - real) -- two cycled volumes that agree to 1e-3 disagree on that sign wherever |cycled - real| is smaller than their
    difference, and one flipped sign is an error of 2 on a magnitude of 1."""
    if typ not in CYCLE_TYPES:
        raise ValueError(typ)
    if typ == 'mae':
        e = cycled - real
        if teacher is None:
            a = (real - cycled).abs()
        else:
            g = sign0(teacher.to(e.dtype) - real).detach()
            a = e.abs().detach() + (g * e - (g * e).detach())
        return O.reduce_mean(a, cfg.gbs, axis=_axes(real)) * cfg.lambda_cycle
    if typ == 'mse':
        return O.mse(real, cycled, cfg.gbs) * cfg.lambda_cycle
    if typ == 'L4':
        return O.reduce_mean((real - cycled) ** 4, cfg.gbs, axis=_axes(real)) * cfg.lambda_cycle
    return O.reduce_mean(O.keras_bce(O.min_max_norm(real), O.min_max_norm(cycled)), cfg.gbs) * cfg.lambda_cycle


def softplus(x: Tensor) -> Tensor:
    """max(x, 0) + log1p(exp(-|x|)), written as -log(sigmoid(-x)): the same number (tests/test_losstypes_host.py), stable for every x and
    smooth at x = 0, where autograd through max(x, 0) and |x| would return a one-sided derivative."""
    return -torch.nn.functional.logsigmoid(-x)


def bce_logits(z: Tensor, x: Tensor) -> Tensor:
    """TP: Keras BinaryCrossentropy(from_logits=True, reduction=NONE) -- tf.nn.sigmoid_cross_entropy_with_logits, channel mean."""
    return (softplus(x) - x * z).mean(dim=-1)


def focal_logits(z: Tensor, x: Tensor, gamma: float = 2.0) -> Tensor:
    """TP: Keras 2.10 BinaryFocalCrossentropy(from_logits=True, reduction=NONE), gamma 2, no class balancing.  1 - sigmoid(x) is taken
    as sigmoid(-x): the same number, without the cancellation at large x."""
    one_minus_pt = z * torch.sigmoid(-x) + (1.0 - z) * torch.sigmoid(x)
    el = one_minus_pt ** gamma * (softplus(x) - x * z)
    return el.mean(dim=-1)


def focal_grad_closed_form(x: Tensor, z: float) -> Tensor:
    """d focal / d x as the kernel evaluates it: z = 1: -(1-s)^3 - 2 s (1-s)^2 softplus(-x);  z = 0: s^3 + 2 s^2 (1-s) softplus(x)."""
    s, c = torch.sigmoid(x), torch.sigmoid(-x)
    sp = softplus
    if z == 1:
        return -c ** 3 - 2 * s * c ** 2 * sp(-x)
    return s ** 3 + 2 * s ** 2 * c * sp(x)


def gan_losses(d_real: Tensor, d_fake: Tensor, typ: Optional[str], cfg):
    """(discriminator loss, generator loss) of discriminator_loss_fn(real, fake, typ) / generator_loss_fn(fake, typ), from_logits=True."""
    if typ not in GAN_TYPES:
        raise ValueError(typ)
    if typ is None:
        d = 0.5 * (O.mse(torch.ones_like(d_real), d_real, cfg.gbs) + O.mse(torch.zeros_like(d_fake), d_fake, cfg.gbs))
        return d, O.mse(torch.ones_like(d_fake), d_fake, cfg.gbs)
    f = bce_logits if typ == 'bce' else focal_logits
    d = O.reduce_mean((f(torch.ones_like(d_real), d_real) + f(torch.zeros_like(d_fake), d_fake)) * 0.5, cfg.gbs)
    return d, O.reduce_mean(f(torch.ones_like(d_fake), d_fake), cfg.gbs)


def compute_losses(P: Dict[str, Dict[str, Tensor]], real_I: Tensor, real_S: Tensor, cfg, noise=None, drop=None, q=None,
                   cycle_loss_SIS: str = 'bce', cycle_loss_ISI: str = 'mse', gan_loss: Optional[str] = None,
                   teacher: Optional[Dict[str, Tensor]] = None, gen_forward=None, disc_forward=None):
    """O.compute_losses (vangan.py:270-353) with the three switches.  teacher: {'cycled_S': ..., 'cycled_I': ...} of the implementation
    under test, for the teacher-forced sign of an 'mae' term (cycle_loss).  gen_forward / disc_forward: other network forwards with the
    oracle's signatures (p, x, q) / (p, x, noise, drop, q)."""
    noise, drop, teacher = noise or {}, drop or {}, teacher or {}
    napp = {'G_IS': 0, 'G_SI': 0}

    def G(name, x):
        tag = 'G_' + name[4:]
        O._PREFIX = '%s.%s/' % (tag, 'ab'[napp[tag]]); napp[tag] += 1
        try:
            if gen_forward is not None:
                return gen_forward(P[name], x, q)
            if 'c7.w' in P[name]:
                return O.resnet_forward(P[name], x, q, drop=drop.get(O._PREFIX[:-1]))
            return O.resunet_forward(P[name], x, q)
        finally:
            O._PREFIX = ''
    fake_S = G('gen_IS', real_I)
    fake_I = G('gen_SI', real_S)
    cycled_S = G('gen_IS', fake_I)
    rS, cS = O.min_max_norm(real_S), O.min_max_norm(cycled_S)
    if cycle_loss_SIS == 'bce':
        cycle_loss_I = O.reduce_mean(O.keras_bce(rS, cS), cfg.gbs) * cfg.lambda_cycle
    else:
        cycle_loss_I = cycle_loss(real_S, cycled_S, cycle_loss_SIS, cfg, teacher.get('cycled_S'))
    seg_loss = O.soft_dice_cldice(rS, cS, cfg.skel_iters) * (cfg.lambda_topology / cfg.n_devices)
    cycled_I = G('gen_SI', fake_S)
    cycle_loss_S = cycle_loss(real_I, cycled_I, cycle_loss_ISI, cfg, teacher.get('cycled_I'))
    rec = O.reduce_mean(O.ssim_loss_3d(O.min_max_norm(real_I), O.min_max_norm(cycled_I)), cfg.gbs) * cfg.lambda_reconstruction

    def D(name, x, tag):
        O._PREFIX = 'D_%s.%s/' % (tag[0], tag[2:])
        try:
            return (disc_forward or O.disc_forward)(P[name], x, noise.get(tag), drop.get(tag), q)
        finally:
            O._PREFIX = ''
    d_real_S, d_fake_S = D('disc_S', real_S, 'S_real'), D('disc_S', fake_S, 'S_fake')
    d_real_I, d_fake_I = D('disc_I', real_I, 'I_real'), D('disc_I', fake_I, 'I_fake')
    disc_S_loss, gen_IS_loss = gan_losses(d_real_S, d_fake_S, gan_loss, cfg)
    disc_I_loss, gen_SI_loss = gan_losses(d_real_I, d_fake_I, gan_loss, cfg)
    total_I = gen_IS_loss + cycle_loss_I + seg_loss
    total_S = gen_SI_loss + cycle_loss_S + rec
    result = dict(zip(O.RESULT_KEYS, [total_I, total_S, disc_I_loss, disc_S_loss, gen_IS_loss, gen_SI_loss, cycle_loss_I, cycle_loss_S,
                                      seg_loss, rec]))
    aux = dict(fake_S=fake_S, fake_I=fake_I, cycled_S=cycled_S, cycled_I=cycled_I, d_real_S=d_real_S, d_fake_S=d_fake_S,
               d_real_I=d_real_I, d_fake_I=d_fake_I)
    return result, aux


def train_step(P, opt_state, real_I, real_S, cfg, noise=None, drop=None, q=None, lr=None, apply=True, **switches):
    """O.train_step over compute_losses above: four gradient sweeps on pre-update weights, then four Adam updates."""
    for net in P.values():
        for t in net.values():
            t.requires_grad_(True)
    result, aux = compute_losses(P, real_I, real_S, cfg, noise, drop, q, **switches)
    pairs = [('gen_IS', 'total_IS_loss'), ('gen_SI', 'total_SI_loss'), ('disc_I', 'D_I_loss'), ('disc_S', 'D_S_loss')]
    grads = {}
    for i, (net, key) in enumerate(pairs):
        names = list(P[net].keys())
        gs = torch.autograd.grad(result[key], [P[net][n] for n in names], retain_graph=(i < len(pairs) - 1), allow_unused=True)
        grads[net] = {n: (g if g is not None else torch.zeros_like(P[net][n])) for n, g in zip(names, gs)}
    for net in P.values():
        for t in net.values():
            t.requires_grad_(False)
    if apply:
        with torch.no_grad():
            for net, _ in pairs:
                hp = dict(getattr(cfg, 'adam', dict(lr=2e-4, beta1=0.5, beta2=0.9, clipnorm=100.0)))
                if lr is not None:
                    hp['lr'] = lr
                O.adam_step(P[net], grads[net], opt_state.setdefault(net, {}), **hp)
    return {k: float(v.detach()) for k, v in result.items()}, grads, {k: v.detach() for k, v in aux.items()}


def test_step(P, real_I, real_S, cfg, q=None, **switches):
    with torch.no_grad():
        result, _ = compute_losses(P, real_I, real_S, cfg, None, None, q, **switches)
    return {k: float(v) for k, v in result.items()}


test_step.__test__ = False          # not a pytest test: the restatement of VanGan.test_step
