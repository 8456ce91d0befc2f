"""CPU tests of the attention-gated ResUNet (ResUNet(use_attention_gate=True), resunet_model.py:152,178-179): the restatement the GPU
tests compare against (tests/ag_restate.py) is checked against an independent formulation and its hand-derived backward against
autograd; parameter specs; the compat keyword; the launches a gated generator makes (dry-run walk); the C ABI."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import ag_restate as R
from oracle import vangan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = {0: (16, 32), 1: (32, 64), 2: (64, 128), 3: (128, 256)}          # decoder level -> (Cs, Ci)


def _second_formulation(p, x):
    """The gated network once more, independently: NDHWC einsums, the low-resolution tensor upsampled EXPLICITLY before phi (the
    reference's order of operations), no shared gate code with ag_restate."""
    t = O.to_ncdhw(x)
    c1 = O.conv3d(O.reflect_pad1(t), p['stem.conv1.w'], p['stem.conv1.b'], 1, 'valid')
    sc = O.instance_norm(O.conv3d(t, p['stem.short.w'], p['stem.short.b'], 1, 'same'), p['stem.short.in.gamma'], p['stem.short.in.beta'])
    h = O._conv_block(p, 'stem.cb', c1, 1, None) + sc
    skips = [h]
    for e in range(1, 5):
        h = O._res_block(p, 'enc%d' % e, h, 2, None)
        skips.append(h)
    h = O._conv_block(p, 'bridge.cb1', h, 1, None)
    h = O._conv_block(p, 'bridge.cb2', h, 1, None)
    for d in (3, 2, 1, 0):
        up = O.to_ndhwc(h).repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
        sk = O.to_ndhwc(skips[d])
        g = 'dec%d.gate.' % d
        theta = torch.einsum('ndhwc,ci->ndhwi', sk, p[g + 'theta.w'][0, 0, 0]) + p[g + 'theta.b']
        phi = torch.einsum('ndhwc,ci->ndhwi', up, p[g + 'phi.w'][0, 0, 0]) + p[g + 'phi.b']
        z = torch.einsum('ndhwi,io->ndhwo', torch.clamp(theta + phi, min=0), p[g + 'psi.w'][0, 0, 0]) + p[g + 'psi.b']
        gated = sk * (1.0 / (1.0 + torch.exp(-z)))
        h = O._res_block(p, 'dec%d' % d, O.to_ncdhw(torch.cat([up, gated], dim=-1)), 1, None)
    return O.to_ndhwc(torch.tanh(O.conv3d(h, p['out.w'], p['out.b'], 1, 'same')))


def _params64(seed):
    P = O.init_params(R.gen_ag_param_specs(), seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in P.items():                      # the zero-initialised biases would hide a missing bias
        if k.endswith('.b') or k.endswith('.beta'):
            v.add_(torch.randn(v.shape, generator=g) * 0.1)
    return {k: v.double() for k, v in P.items()}


def test_restatement_against_a_second_formulation():
    P = _params64(3)
    x, _ = O.synth_volumes(1, 32, 32, 32, seed=5)
    taps = {}
    y1 = R.resunet_ag_forward(P, x.double(), taps=taps)
    y2 = _second_formulation(P, x.double())
    err = float((y1 - y2).abs().max())
    print('gated network, low-grid phi vs explicit upsampling, float64 32^3: max abs difference %.3e' % err)
    assert err < 1e-12
    hs = [taps['dec%d.gate.h' % d] for d in range(4)]
    assert all(float(h.min()) > 0 and float(h.max()) < 1 for h in hs)
    assert float((y1 - O.resunet_forward(P, x.double())).abs().max()) > 1e-3          # the gate does something


def test_identity_gate_reproduces_the_plain_network_bit_for_bit():
    """psi.w = 0, psi.b = 40: sigmoid(40) rounds to 1 in float64 (and fp32), so the gated restatement IS the plain oracle."""
    P = _params64(7)
    for d in range(4):
        P['dec%d.gate.psi.w' % d].zero_()
        P['dec%d.gate.psi.b' % d].fill_(40.0)
    x, _ = O.synth_volumes(1, 32, 32, 32, seed=6)
    assert torch.equal(R.resunet_ag_forward(P, x.double()), O.resunet_forward(P, x.double()))


def test_backward_formulas_against_autograd():
    g = torch.Generator().manual_seed(11)
    N, S, Cs, Ci = 2, 8, 16, 32
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    skip, phi, dG = rn(N, S, S, S, Cs), rn(N, S // 2, S // 2, S // 2, Ci), rn(N, S, S, S, Cs)
    p = {'g.theta.w': rn(1, 1, 1, Cs, Ci) * 0.3, 'g.theta.b': rn(Ci) * 0.1, 'g.psi.w': rn(1, 1, 1, Ci, 1) * 0.3, 'g.psi.b': rn(1) * 0.1}
    leaves = [skip, phi] + list(p.values())
    for t in leaves:
        t.requires_grad_(True)
    gated, h = R.attention_gate(p, 'g', O.to_ncdhw(skip), None, None, phi=O.to_ncdhw(phi))
    (O.to_ndhwc(gated) * dG).sum().backward()
    got = R.gate_backward_formulas(skip.detach(), phi.detach(), h.detach()[:, 0], dG, p['g.theta.w'].detach()[0, 0, 0], p['g.theta.b'].detach(),
                                   p['g.psi.w'].detach()[0, 0, 0, :, 0])
    ref = dict(d_skip=skip.grad, d_phi=phi.grad, dw_theta=p['g.theta.w'].grad[0, 0, 0], db_theta=p['g.theta.b'].grad,
               dw_psi=p['g.psi.w'].grad[0, 0, 0, :, 0], db_psi=p['g.psi.b'].grad[0])
    for k in ref:
        err = float((got[k] - ref[k]).abs().max())
        print('%-9s max abs difference to autograd %.3e (|ref| max %.3e)' % (k, err, float(ref[k].abs().max())))
        assert err < 1e-9, k


def test_param_specs():
    from van_gan_amd.nets import gen_param_specs
    n = lambda sp: sum(int(torch.tensor(s).prod()) for _, s, _ in sp)
    plain, gated = gen_param_specs(), gen_param_specs(True)
    assert (len(plain), n(plain)) == (116, 9538929) and gen_param_specs(False) == plain
    assert (len(gated), n(gated)) == (140, 9670933)
    assert [(a, tuple(b)) for a, b, _ in gated] == [(a, tuple(b)) for a, b, _ in R.gen_ag_param_specs()]
    assert [(a, tuple(b)) for a, b, _ in plain] == [(a, tuple(b)) for a, b, _ in O.gen_param_specs()]
    names = [a for a, _, _ in gated]
    for d, (cs, ci) in LEVELS.items():
        i = names.index('dec%d.cb1.in.gamma' % d)
        assert names[i - 6:i] == ['dec%d.gate.%s' % (d, k) for k in ('theta.w', 'theta.b', 'phi.w', 'phi.b', 'psi.w', 'psi.b')]
        shapes = dict((a, tuple(b)) for a, b, _ in gated)
        assert shapes['dec%d.gate.theta.w' % d] == (1, 1, 1, cs, ci) and shapes['dec%d.gate.phi.w' % d] == (1, 1, 1, ci, ci)
        assert shapes['dec%d.gate.psi.w' % d] == (1, 1, 1, ci, 1) and shapes['dec%d.gate.psi.b' % d] == (1,)
    assert n(gated) - n(plain) == 1633 + 6337 + 24961 + 99073
    # the suffix that data parallelism reduces early (enc4 ... out) stays one contiguous range behind the same first parameter
    assert names.index('enc4.cb1.in.gamma') == [a for a, _, _ in plain].index('enc4.cb1.in.gamma')
    assert [x for x in names if '.gate.' not in x] == [a for a, _, _ in plain]


def test_store_and_network_must_agree():
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs
    with pytest.raises(ValueError):
        ResUNet(ParamStore(gen_param_specs(), 'cpu'), (32, 32, 32), attention_gate=True)
    with pytest.raises(ValueError):
        ResUNet(ParamStore(gen_param_specs(True), 'cpu'), (32, 32, 32))


def test_compat_keyword():
    import argparse
    from van_gan_amd.compat import engine_kwargs_from_args
    a = argparse.Namespace(DIMENSIONS=3, CHANNELS=1, SUBVOL_PATCH_SIZE=(64, 64, 64, 1), N_DEVICES=1, BATCH_SIZE=1, GLOBAL_BATCH_SIZE=1)
    kw = engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', use_attention_gate=True)
    assert kw['attention_gate'] is True and kw['generator'] == 'resUnet'
    assert 'attention_gate' not in engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet')
    with pytest.raises(ValueError):
        engine_kwargs_from_args(a, gen_i2s='resnet', gen_s2i='resnet', use_attention_gate=True)


def _walk(dims, B, gate):
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs, pair_ctx
    G = ResUNet(ParamStore(gen_param_specs(gate), 'cpu'), dims, torch.bfloat16, attention_gate=gate)
    ar = ops.Arena(int(B * dims[0] * dims[1] * dims[2] * 5200 * 2) + (512 << 20), 'cpu')
    with ops.DryRun() as dry:
        x2 = ar.alloc((2 * B,) + dims + (1,), torch.float32)
        y, yb = ar.alloc((B,) + dims + (1,), torch.float32), ar.alloc((B,) + dims + (1,), torch.float32)
        ar.pair_begin('g', 0)
        ctx = G.forward(ar, x2[:B], y)
        ar.pair_end()
        n0, c0 = len(dry.records), len(dry.calls)
        ar.pair_begin('g', 1)
        G.forward(ar, x2[B:], yb)
        ar.pair_end()
        assert dry.calls[c0:] == dry.calls[:c0]             # the second application repeats the first one's calls
        del dry.records[n0:]; del dry.calls[c0:]
        G.backward(ar, pair_ctx(ar, ctx, x2, (y, yb), G.lv[0]), x2)
    return dry.records, dry.calls


@pytest.mark.parametrize('dims,B', [((32, 32, 32), 2), ((128, 128, 128), 1)])
def test_dry_walk_records_the_gate_launches(dims, B):
    recs, calls = _walk(dims, B, True)
    fwd = [dict(r) for n, r in calls if n == 'vg_attn_gate_fwd']
    bwd = [dict(r) for n, r in calls if n == 'vg_attn_gate_bwd']
    assert len(fwd) == 4 and len(bwd) == 4
    for d, (cs, ci) in LEVELS.items():
        lv = tuple(n >> d for n in dims)
        want = dict(N=B, D=lv[0], H=lv[1], W=lv[2], Cs=cs, Ci=ci, f32=0)
        assert want in fwd, (d, fwd)
        # ONE backward sweep over both applications (2B samples); the gate is the first writer of the encoder activation's gradient
        assert dict(want, N=2 * B, acc=0) in bwd, (d, bwd)
    phi = {(k, n) for k, n, _ in recs if '.gate.phi' in n}
    assert phi == {(k, 'dec%d.gate.phi' % d) for d in range(4) for k in ('fwd', 'wgrad', 'dgrad')}
    # the skip half of each decoder block's first norm: one finalisation launch per level from (low.sums, gated.sums)
    fin = [dict(r) for n, r in calls if n == 'vg_in_finalize']
    assert sorted((r['c0'], r['c1']) for r in fin) == sorted((ci, cs) for cs, ci in LEVELS.values())
    # without the switch: none of them, and nothing else changes among the shared launches
    recs0, calls0 = _walk(dims, B, False)
    assert not [n for n, _ in calls0 if n.startswith('vg_attn_gate')] and not [n for _, n, _ in recs0 if '.gate.' in n]
    assert [(k, n) for k, n, _ in recs if '.gate.' not in n] == [(k, n) for k, n, _ in recs0]


def test_header_declares_the_gate_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    declared = set(re.findall(r'^(?:int|int64_t|const char\*)\s+(vg_[a-z0-9_]+)\s*\(', hdr, flags=re.M))
    assert {'vg_attn_gate_fwd', 'vg_attn_gate_bwd'} <= declared
    from van_gan_amd import _lib, build
    assert 'vg_attngate.hip' in build.SOURCES
    assert hasattr(_lib.lib, 'vg_attn_gate_fwd') and hasattr(_lib.lib_fp16(), 'vg_attn_gate_bwd')
    # invalid shapes are refused on the host, before any launch
    assert _lib.lib.vg_attn_gate_fwd(*([1 << 20] * 6), 1, 8, 8, 8, 16, 48, 0, *([1 << 20] * 4)) == -1
    assert _lib.lib.vg_attn_gate_fwd(*([1 << 20] * 6), 1, 8, 7, 8, 16, 32, 0, *([1 << 20] * 4)) == -1

