"""Restatement of ResUNet(use_attention_gate=True) (resunet_model.py:152,178-179; attention_gate / attention_concat of
vnet_model.py:24-77, Oktay et al., Attention U-Net) in torch -- test infrastructure only, composed from the oracle's own pieces
(oracle.vangan_oracle: conv3d, instance_norm through _conv_block / _res_block, _store).

Per decoder level d, skip = skips[d] (Cs channels), x = the previous decoder / bridge output (Cx channels, half the grid), Ci = Cx:
    theta = Conv1x1x1(Cs -> Ci)(skip);  phi = Conv1x1x1(Cx -> Ci)(UpSampling3D(2)(x));  q = relu(theta + phi)
    h = sigmoid(Conv1x1x1(Ci -> 1)(q));  gated = skip * h;  block input = concatenate([up, gated])
A 1x1x1 convolution commutes with nearest-neighbour upsampling, so phi is evaluated on the low grid and upsampled (the engine's form;
tests/test_attngate_host.py checks it against the explicit-upsampling form).  Storage points of the engine (rounded by `q`, teacher
forced by O.TEACHER): 'dec%d.gate.phi' (phi on the low grid) and 'dec%d.gate' (the gated skip tensor).  theta's operands are rounded
like every convolution's (the matrix pipe reads 16-bit operands); psi runs in fp32 on the engine: nothing is rounded there.
"""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import vangan_oracle as O

Tensor = torch.Tensor


def gen_ag_param_specs():
    """O.gen_param_specs() with the gate's three convolutions (theta, phi, psi: creation order) in front of each decoder block."""
    f = O.GEN_F
    out = []
    for name, shape, init in O.gen_param_specs():
        for d in range(4):
            if name == 'dec%d.cb1.in.gamma' % d:
                for k, ci, co in (('theta', f[d], f[d + 1]), ('phi', f[d + 1], f[d + 1]), ('psi', f[d + 1], 1)):
                    out.append(('dec%d.gate.%s.w' % (d, k), (1, 1, 1, ci, co), 'he_normal'))
                    out.append(('dec%d.gate.%s.b' % (d, k), (co,), 'zeros'))
        out.append((name, shape, init))
    return out


def upsample2(x: Tensor) -> Tensor:
    """UpSampling3D(2) on NCDHW."""
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)


def attention_gate(p: Dict[str, Tensor], name: str, skip: Tensor, x_low: Optional[Tensor], q: O.Q = None, phi: Optional[Tensor] = None,
                   taps: Optional[dict] = None):
    """skip NCDHW [N, Cs, D, H, W], x_low NCDHW [N, Cx, D/2, H/2, W/2] -> (gated, h [N, 1, D, H, W]).  name = 'dec%d.gate'.
    phi given (NCDHW on the low grid, a kernel-level test's input): used as it is instead of phi's convolution."""
    theta = O.conv3d(skip, p[name + '.theta.w'], p[name + '.theta.b'], 1, 'same', q)
    if phi is None:
        phi = O._store(q, name + '.phi', O.conv3d(x_low, p[name + '.phi.w'], p[name + '.phi.b'], 1, 'same', q))
    pre = theta + upsample2(phi)
    a = F.relu(pre)
    h = torch.sigmoid(O.conv3d(a, p[name + '.psi.w'], p[name + '.psi.b'], 1, 'same', None))
    gated = O._store(q, name, skip * h)
    if taps is not None:
        taps[name], taps[name + '.h'], taps[name + '.phi'], taps[name + '.pre'] = gated, h, phi, pre
    return gated, h


def resunet_ag_forward(p: Dict[str, Tensor], x_ndhwc: Tensor, q: O.Q = None, taps: Optional[dict] = None) -> Tensor:
    """O.resunet_forward with every decoder level's skip tensor gated (same signature: O.compute_losses can call it)."""
    x = O.to_ncdhw(x_ndhwc)
    c1 = O._store(q, 'stem.conv1', O.conv3d(O.reflect_pad1(x), p['stem.conv1.w'], p['stem.conv1.b'], 1, 'valid', q))
    if taps is not None:
        taps['stem.conv1'] = c1
    sc = O.conv3d(x, p['stem.short.w'], p['stem.short.b'], 1, 'same', q)
    scn = O.instance_norm(sc, p['stem.short.in.gamma'], p['stem.short.in.beta'])
    h = O._store(q, 'stem', O._conv_block(p, 'stem.cb', c1, 1, q) + scn)
    if taps is not None:
        taps['stem'] = h
    skips = [h]
    for e in range(1, 5):
        h = O._res_block(p, 'enc%d' % e, h, 2, q, taps)
        skips.append(h)
    h = O._store(q, 'bridge.cb1', O._conv_block(p, 'bridge.cb1', h, 1, q))
    h = O._store(q, 'bridge.cb2', O._conv_block(p, 'bridge.cb2', h, 1, q))
    if taps is not None:
        taps['bridge'] = h
    for d in (3, 2, 1, 0):
        gated, _ = attention_gate(p, 'dec%d.gate' % d, skips[d], h, q, taps=taps)
        h = torch.cat([upsample2(h), gated], dim=1)
        h = O._res_block(p, 'dec%d' % d, h, 1, q, taps)
    y = O._store(None, 'y', torch.tanh(O.conv3d(h, p['out.w'], p['out.b'], 1, 'same', q)))
    return O.to_ndhwc(y)


def gate_backward_formulas(skip: Tensor, phi_low: Tensor, h: Tensor, dG: Tensor, w_theta: Tensor, b_theta: Tensor, w_psi: Tensor):
    """The hand-derived backward of the gate on NDHWC tensors (skip / dG [N, D, H, W, Cs], phi_low [N, D/2, H/2, W/2, Ci], h [N, D, H, W],
    w_theta [Cs, Ci], w_psi [Ci]) -- the formulas vg_attn_gate_bwd implements:
      dh = sum_c dG_c skip_c;  dz = dh h (1 - h);  dq = dz w_psi [q > 0];  d_skip = dG h + dq W_theta^T;
      d_phi(low voxel) = sum of dq over its 8 children;  dW_theta = skip^T dq;  db_theta = sum dq;  dw_psi = sum dz q;  db_psi = sum dz."""
    up = phi_low.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
    qv = F.relu(skip @ w_theta + b_theta + up)
    dh = (dG * skip).sum(-1)
    dz = dh * h * (1 - h)
    dq = dz[..., None] * w_psi * (qv > 0).to(skip.dtype)
    N, D, H, W, Ci = dq.shape
    return dict(d_skip=dG * h[..., None] + dq @ w_theta.t(),
                d_phi=dq.view(N, D // 2, 2, H // 2, 2, W // 2, 2, Ci).sum((2, 4, 6)),
                dw_theta=torch.einsum('ndhwc,ndhwi->ci', skip, dq), db_theta=dq.sum((0, 1, 2, 3)),
                dw_psi=(dz[..., None] * qv).sum((0, 1, 2, 3)), db_psi=dz.sum())
