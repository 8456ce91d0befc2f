"""The non-convolution calls of BASELINE configs 2, 3 and 4, and a GPU parity case at a TRUE SHAPE for each of them.

The same dry-run walk as tests/layer_recipes.py (layer_recipes.walk_config) records, besides the convolution launches, every call of the
InstanceNorm backward (vg_actnorm_bwd / _stats / _apply / _apply2), vg_concat_bwd, vg_stem_short_fwd / _bwd and vg_tanh_bwd with a
shape-level regime (ops.DryRun.calls: the descriptor's fields, no pointers), and every forward launch that carries the InstanceNorm
finalisation tail (recipe['fin']: its jobs).  call_cases() turns those into GPU cases; tests/test_call_coverage.py (CPU) proves that
they cover every recorded (entry point, regime) and every (forward variant, tail job shape), tests/test_gpu_calls.py replays them
against float64 references on the device.

The decoder blocks' fused backward launches (vg_shortcut_dgrad_concat_norm / vg_shortcut_dgrad_concat) are not taken in dry-run mode
(ops.ConvLayer.dgrad_concat_norm / dgrad_concat): decoder_blocks() lists them explicitly per config.

cases_of() is the one loop that turns walks into cases: call_cases() feeds it the three BASELINE walks, ragged_call_cases() the walks
of layer_recipes.RAGGED_CONFIGS / RAGGED_INFER_CONFIGS (tests/test_gpu_ragged.py, tests/test_ragged_coverage.py), batch3_call_cases()
the walks of layer_recipes.BATCH3_CONFIGS (tests/test_gpu_batch3.py, tests/test_batch3_coverage.py).

Helper module (no tests in here)."""
from __future__ import annotations

import functools
from typing import Dict, List

import torch

import layer_recipes as LR

ANB_ENTRIES = ('vg_actnorm_bwd', 'vg_actnorm_bwd_stats', 'vg_actnorm_bwd_apply')


@functools.lru_cache(maxsize=None)
def all_walks():
    """config -> (conv records, non-convolution calls) of one train step (layer_recipes.walk_config)."""
    return {cfg: LR.walk_config(*LR.CONFIGS[cfg]) for cfg in LR.NEEDED}


def needed_calls():
    """Every (entry point, regime) the walks of BASELINE configs 2-4 record."""
    return sorted({c for cfg in LR.NEEDED for c in all_walks()[cfg][1]}, key=repr)


def fin_shape(recipe) -> tuple:
    """The job shape of a forward launch's finalisation tail: per job (has mult, writes at a channel offset)."""
    return tuple((bool(j['mult']), j['c_off'] > 0) for j in recipe['fin']['jobs'])


def needed_fin():
    """Every (forward variant, tail job shape) the walks record."""
    return sorted({(v, fin_shape(r)) for cfg in LR.NEEDED for k, _, v, r in all_walks()[cfg][0] if k == 'fwd' and r.get('fin')})


def inference_needed_fin():
    """Every (forward variant, tail job shape) of the two NEEDED inference walks (layer_recipes.INFER_NEEDED)."""
    walks = LR.all_inference_walks()
    return sorted({(v, fin_shape(r)) for cfg in LR.INFER_NEEDED for k, _, v, r in walks[cfg][0] if k == 'fwd' and r.get('fin')})


@functools.lru_cache(maxsize=None)
def inference_fin_cases() -> Dict[str, dict]:
    """case id -> run_fin case for every (forward variant, tail job shape) of the inference walks that the train steps' needed_fin() does
    not have: the cheapest recorded call with that tail over all inference walks, shrunk like its convolution's representative
    (layer_recipes.shrink_recipe: identical variant string, the tail's voxel count follows the grid)."""
    have = set(needed_fin())
    want = [k for k in inference_needed_fin() if k not in have]
    cases: Dict[str, dict] = {}
    for cfg, (recs, _) in LR.all_inference_walks().items():
        for kind, layer, v, r in recs:
            if kind != 'fwd' or not r.get('fin') or (v, fin_shape(r)) not in want:
                continue
            cid = 'fin %s jobs=%s' % (v, fin_shape(r))
            m = LR.recipe_macs(r)
            if cid not in cases or m < cases[cid]['macs']:
                cases[cid] = dict(kind='fin', recipe=r, variant=v, config=cfg, layer=layer, macs=m, covers=[('fin', v, fin_shape(r))])
    for c in cases.values():
        c['recipe'] = LR.shrink_recipe(c['recipe'], c['variant'])
        c['macs'] = LR.recipe_macs(c['recipe'])
    return cases


def decoder_blocks(cfg, configs=None) -> List[dict]:
    """The decoder blocks' fused backward launches of one config: dec0-dec3 with the shortcut's c_low (upsampled source), c_skip, cout,
    the block's level dims and the 2B samples of the generator's backward sweep (the two applications are one sweep).  configs: the
    table `cfg` is a key of (layer_recipes.CONFIGS unless given)."""
    from van_gan_amd.nets import GEN_F
    dims, B = (LR.CONFIGS if configs is None else configs)[cfg]
    out = []
    for d in range(4):
        lv = tuple(n >> d for n in dims)
        # served: the split kernel of vg_pointwise.hip has (dY channels / 32, concat channels / 16) = (1, 3) and (1, 6), i.e. dec0 and dec1;
        # dec2 and dec3 take the step's fall-back (apply pass into a concat gradient, then dgrad + concat backward)
        out.append(dict(block='dec%d' % d, config=cfg, N=2 * B, dims=lv, c_low=GEN_F[d + 1], c_skip=GEN_F[d], cout=GEN_F[d], served=d < 2))
    return out


def _rd(regime) -> dict:
    return dict(regime)


def cases_of(walks, configs) -> Dict[str, dict]:
    """The case list of a set of walks ({config: (conv records, non-convolution calls)}, in order): case id -> {'kind', ..., 'covers':
    [(entry point, regime)]}.  One case per recorded InstanceNorm-backward regime (statistics then apply: covers the three
    single-descriptor entry points), per recorded apply2 pair (statistics of both jobs, then the two-job launch), per decoder block of
    each config in `configs` (a train config: covers its vg_concat_bwd), per stem shortcut / tanh call, and per (forward variant, tail
    job shape): the cheapest call with that tail."""
    cases: Dict[str, dict] = {}
    for cfg, (recs, calls) in walks.items():
        for name, reg in calls:
            if name in ANB_ENTRIES:
                r = _rd(reg)
                cid = 'anb N%(N)d %(D)dx%(H)dx%(W)d C%(C)d' % r + ' ' + ' '.join('%s=%d' % kv for kv in reg[5:] if kv[1])
                c = cases.setdefault(cid, dict(kind='anb', regime=reg, config=cfg, covers=[]))
                c['covers'] += [(e, reg) for e in ANB_ENTRIES]
            elif name == 'vg_actnorm_bwd_apply2':
                r1, r2 = _rd(reg[0][1]), _rd(reg[1][1])
                cid = 'apply2 N%(N)d %(D)dx%(H)dx%(W)d' % r1 + ' C%d+C%d pad%d/%d' % (r1['C'], r2['C'], r1['g_padded'], r2['g_padded'])
                c = cases.setdefault(cid, dict(kind='apply2', regime=reg, config=cfg, covers=[]))
                c['covers'] += [(name, reg), ('vg_actnorm_bwd_stats', reg[0][1]), ('vg_actnorm_bwd_stats', reg[1][1])]
            elif name == 'vg_stem_short_fwd' or name == 'vg_stem_short_bwd' or name == 'vg_tanh_bwd':
                cid = '%s %s' % (name[3:], ' '.join('%s=%d' % kv for kv in reg))
                cases.setdefault(cid, dict(kind=name[3:], regime=reg, config=cfg, covers=[(name, reg)]))
        for blk in (decoder_blocks(cfg, configs) if cfg in configs else []):
            cid = 'decoder %s %s' % (blk['block'], cfg)
            reg = (('N', blk['N']), ('D', blk['dims'][0]), ('H', blk['dims'][1]), ('W', blk['dims'][2]), ('Cu', blk['c_low']),
                   ('Cs', blk['c_skip']), ('has_dskip', 1), ('f32', 0))
            cases[cid] = dict(kind='decoder', block=blk, config=cfg,
                              covers=[('vg_concat_bwd', reg + (('acc', acc),)) for acc in range(4)])
        for kind, layer, v, r in recs:
            if kind != 'fwd' or not r.get('fin'):
                continue
            key = (v, fin_shape(r))
            cid = 'fin %s jobs=%s' % key
            m = LR.recipe_macs(r)
            if cid not in cases or m < cases[cid]['macs']:
                cases[cid] = dict(kind='fin', recipe=r, variant=v, config=cfg, layer=layer, macs=m, covers=[('fin',) + key])
    return cases


@functools.lru_cache(maxsize=None)
def call_cases() -> Dict[str, dict]:
    """cases_of the train steps of BASELINE configs 2, 3 and 4: what tests/test_gpu_calls.py replays."""
    return cases_of({cfg: all_walks()[cfg] for cfg in LR.NEEDED}, {cfg: LR.CONFIGS[cfg] for cfg in LR.NEEDED})


# ----------------------------------------------------------------------------------------------------------------------
# ragged patches (layer_recipes.RAGGED_CONFIGS / RAGGED_INFER_CONFIGS)
# ----------------------------------------------------------------------------------------------------------------------
def ragged_needed_calls():
    """Every (entry point, regime) the ragged walks record, train and inference."""
    return sorted({c for _, calls in LR.all_ragged_walks().values() for c in calls}, key=repr)


def ragged_needed_fin():
    """Every (forward variant, tail job shape) the ragged walks record, train and inference."""
    return sorted({(v, fin_shape(r)) for recs, _ in LR.all_ragged_walks().values() for k, _, v, r in recs if k == 'fwd' and r.get('fin')})


@functools.lru_cache(maxsize=None)
def ragged_call_cases() -> Dict[str, dict]:
    """cases_of the ragged walks.  A non-convolution case is dropped only if every (entry point, regime) it covers is, field for field,
    one call_cases() covers (regimes carry N and the grid, so that is the exception).  A tail case is never dropped: its key has no
    grid in it, and the recorded call -- the voxel count of the statistics and the kernel's last, partial tiles -- is a ragged one."""
    have = {c for case in call_cases().values() for c in case['covers']}
    cases = cases_of(LR.all_ragged_walks(), LR.RAGGED_CONFIGS)
    return {cid: c for cid, c in cases.items() if c['kind'] == 'fin' or not all(cv in have for cv in c['covers'])}


# ----------------------------------------------------------------------------------------------------------------------
# batch 3 (layer_recipes.BATCH3_CONFIGS)
# ----------------------------------------------------------------------------------------------------------------------
def batch3_needed_calls():
    """Every (entry point, regime) the batch-3 walks record."""
    return sorted({c for _, calls in LR.all_batch3_walks().values() for c in calls}, key=repr)


def batch3_needed_fin():
    """Every (forward variant, tail job shape) the batch-3 walks record."""
    return sorted({(v, fin_shape(r)) for recs, _ in LR.all_batch3_walks().values() for k, _, v, r in recs if k == 'fwd' and r.get('fin')})


@functools.lru_cache(maxsize=None)
def batch3_call_cases() -> Dict[str, dict]:
    """cases_of the batch-3 walks, filtered as ragged_call_cases() is: a non-convolution case is dropped only if call_cases() or
    ragged_call_cases() covers every (entry point, regime) it covers, field for field (regimes carry N: none is); a tail case never (its
    key has no N in it, and the recorded call -- three samples' statistics, the kernel's tile walk over 3 samples -- is a batch-3 one).
    A tail whose recorded call costs more than layer_recipes.macs_cap() is shrunk like its convolution's representative."""
    have = {c for cases in (call_cases(), ragged_call_cases()) for case in cases.values() for c in case['covers']}
    cases = cases_of(LR.all_batch3_walks(), LR.BATCH3_CONFIGS)
    cases = {cid: c for cid, c in cases.items() if c['kind'] == 'fin' or not all(cv in have for cv in c['covers'])}
    cap = LR.macs_cap()
    for c in cases.values():
        if c['kind'] == 'fin' and c['macs'] > cap:
            r = LR.shrink_call(c['recipe'], c['variant'], cap)
            if r is not c['recipe']:
                c.update(recipe=r, macs=LR.recipe_macs(r), shrunk=True, recorded=c['recipe'])
    return cases


def fin_stress_cases() -> Dict[str, dict]:
    """The largest tail-carrying forward call of each kernel family that carries the tail (vg_conv_thin.hip, vg_conv.hip, vg_c1k3.hip,
    vg_pointwise.hip) -- for 200 launches on two streams."""
    fam = {'conv_thin': 'vg_conv_thin', 'conv_thin2': 'vg_conv_thin', 'conv': 'vg_conv', 'c1m_fwd': 'vg_c1k3', 'pw_gemm': 'vg_pointwise'}
    best: Dict[str, dict] = {}
    for cfg in LR.NEEDED:
        for kind, layer, v, r in all_walks()[cfg][0]:
            f = fam.get(v.split('<')[0])
            if kind != 'fwd' or not r.get('fin') or f is None:
                continue
            m = LR.recipe_macs(r)
            if f not in best or m > best[f]['macs']:
                best[f] = dict(recipe=r, variant=v, config=cfg, layer=layer, macs=m)
    return best


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm backward: random operands for a regime and its float64 reference (plain torch on the device)
# ----------------------------------------------------------------------------------------------------------------------
def anb_bytes(r: dict) -> int:
    """Upper bound of the guarded-arena bytes of one regime's operands: g, x (+ x1) and dx on the padded grid at four bytes an element,
    one more for slack, and 32 slots of up to 1 MiB for the per-(sample, channel) arrays."""
    import guarded
    cs = max(r['C'], r['dx_cstride'])
    big = 4 * r['N'] * (r['D'] + 2) * (r['H'] + 2) * (r['W'] + 2) * cs
    return 4 * guarded.slot_cost(big) + 32 * guarded.slot_cost(1 << 20)


def anb_operands(r: dict, dev, seed=0, arena=None):
    """Random tensors for an InstanceNorm-backward regime (dict of its fields).  Samples >= alias_n0 read the forward tensors and
    per-(sample, channel) constants of sample n - alias_shift: those have alias_n0 samples.
    arena (tests/guarded.py): every tensor a descriptor points at is a slot of it -- what the kernels only read sealed, a dx that is
    overwritten 0xFF bytes, one that is accumulated into (or written in a channel slice) its random contents, sums and gamma / beta
    gradients zeros.  t['dx0'] stays a plain copy."""
    g = torch.Generator(device=dev).manual_seed(seed)
    N, D, H, W, C = r['N'], r['D'], r['H'], r['W'], r['C']
    Nx = r['alias_n0'] if r['alias_n0'] > 0 else N
    bf = torch.float32 if r['f32'] else torch.bfloat16
    rn = lambda *s, dt=torch.float32: torch.randn(*s, generator=g, device=dev).to(dt)
    ru = lambda *s: torch.rand(*s, generator=g, device=dev)
    gd = (D + 2, H + 2, W + 2) if r['g_padded'] else (D, H, W)
    t = dict(g=rn(N, *gd, C, dt=bf))
    if r['has_x']:
        if C == 1:
            t['x'] = rn(Nx, D, H, W, 1, dt=torch.float32 if r['x_f32'] else bf)
        elif r['has_x1']:
            sh = r['x0_shift']
            t['x'] = rn(Nx, D >> sh, H >> sh, W >> sh, r['c_x0'], dt=bf)
            t['x1'] = rn(Nx, D, H, W, C - r['c_x0'], dt=bf)
        else:
            t['x'] = rn(Nx, D, H, W, C, dt=torch.float32 if r['x_f32'] else bf)
    if r['has_scale']:
        t['scale'], t['shift'] = ru(Nx, C) + 0.5, rn(Nx, C) * 0.3
    if r['norm']:
        t['mean'], t['rstd'] = rn(Nx, C) * 0.2, ru(Nx, C) + 0.5
        t['gamma'] = ru(C) + 0.5
    if r['has_mult']:
        t['mult'] = (ru(Nx, C) > 0.3).float() * 2.0          # SpatialDropout3D: 0 or 1 / (1 - rate)
    cs = r['dx_cstride'] if r['dx_cstride'] > 0 else C
    dxdt = torch.float32 if (r['dx_f32'] or r['f32']) else torch.bfloat16
    t['dx'] = (rn(N, D, H, W, cs, dt=dxdt) if (r['accumulate'] or cs != C) else torch.full((N, D, H, W, cs), 7.0, dtype=dxdt, device=dev))
    t['dx0'] = t['dx'].clone()
    if r['has_dgamma']:
        t['dgamma'], t['dbeta'] = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    from van_gan_amd import ops
    t['red'] = torch.zeros(ops.STRIPES * N * C * 2 + 4, device=dev)
    if arena is not None:
        for k in ('g', 'x', 'x1', 'scale', 'shift', 'mean', 'rstd', 'gamma', 'mult'):
            if k in t:
                t[k] = arena.put(t[k], name=k)
        if r['accumulate'] or cs != C:
            t['dx'] = arena.put(t['dx'], name='dx', mutable=True)
        else:
            t['dx'] = arena.out(t['dx'].shape, dxdt, None, name='dx')
        for k in ('dgamma', 'dbeta', 'red'):
            if k in t:
                t[k] = arena.out(t[k].shape, torch.float32, 0.0, name=k)
    return t


def anb_desc(r: dict, t: dict):
    from van_gan_amd import ops
    N, D, H, W, C = r['N'], r['D'], r['H'], r['W'], r['C']
    return ops.actnorm_desc(t['g'], bool(r['g_padded']), t.get('x'), (N, D, H, W), C, t['dx'], scale=t.get('scale'), shift=t.get('shift'),
                            mult=t.get('mult'), act=r['act'], norm=bool(r['norm']), gamma=t.get('gamma'), mean=t.get('mean'), rstd=t.get('rstd'),
                            red=t['red'] if r['norm'] else None, accumulate=bool(r['accumulate']), x1=t.get('x1'), c_x0=r['c_x0'],
                            x0_shift=r['x0_shift'], dx_cstride=r['dx_cstride'], dx_coff=r['dx_coff'], dgamma=t.get('dgamma'),
                            dbeta=t.get('dbeta'), alias_n0=r['alias_n0'], alias_shift=r['alias_shift'], pgrad_n=r['pgrad_n'])


def anb_reference(r: dict, t: dict):
    """float64: (red [N, C, 2], dx written slice [N, D, H, W, C], dgamma, dbeta) of  a = mult * act(x * scale + shift)  ->  IN backward."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    N, C = r['N'], r['C']
    g = t['g'].double()
    if r['g_padded']:           # transpose of the reflection pad
        z = torch.zeros(N, C, r['D'], r['H'], r['W'], dtype=torch.float64, device=g.device, requires_grad=True)
        (O.reflect_pad1(z) * g.permute(0, 4, 1, 2, 3)).sum().backward()
        g = z.grad.permute(0, 2, 3, 4, 1)
    nx = torch.arange(N, device=g.device)
    if r['alias_n0'] > 0:
        nx = torch.where(nx >= r['alias_n0'], nx - r['alias_shift'], nx)
    per = lambda k: t[k].double()[nx].view(N, 1, 1, 1, C)
    if r['has_mult']:
        g = g * per('mult')
    dn, xh = g, torch.zeros_like(g)
    if r['has_x']:
        x = t['x'].double()
        if r['has_x1']:
            if r['x0_shift']:
                x = x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
            x = torch.cat([x, t['x1'].double()], dim=-1)
        x = x[nx]
        pre = x * per('scale') + per('shift') if r['has_scale'] else x
        if r['act'] != ops.ACT_NONE:
            slope = 0.0 if r['act'] == ops.ACT_RELU else 0.2
            dn = torch.where(pre > 0, g, g * slope)
        if r['norm']:
            xh = (x - per('mean')) * per('rstd')
    red = torch.stack([dn.sum(dim=(1, 2, 3)), (dn * xh).sum(dim=(1, 2, 3))], dim=-1)
    if r['norm']:
        S = r['D'] * r['H'] * r['W']
        k0 = t['gamma'].double().view(1, 1, 1, 1, C) * per('rstd')
        dx = k0 * (dn - red[..., 0].view(N, 1, 1, 1, C) / S - xh * red[..., 1].view(N, 1, 1, 1, C) / S)
    else:
        dx = dn
    pn = r['pgrad_n'] if r['pgrad_n'] > 0 else N
    return red, dx, red[:pn, :, 1].sum(0), red[:pn, :, 0].sum(0)


def anb_check(r: dict, t: dict, ref, name: str, stats: bool = True) -> dict:
    """Compare the kernel's striped sums, dx (the written channel slice; the rest of the row untouched) and gamma / beta gradients with
    the float64 reference.  Returns the measured errors."""
    from van_gan_amd import ops
    red, dx, dgam, dbet = ref
    N, C = r['N'], r['C']
    err = {}
    if r['norm'] and stats:
        got = t['red'][:ops.STRIPES * N * C * 2].view(ops.STRIPES, N, C, 2).sum(0)
        err['red'] = LR.rel_l2(got, red)
        assert err['red'] <= 1e-4, '%s: striped sums rel %.2e' % (name, err['red'])
    if r['has_dgamma'] and r['norm']:
        err['dgamma'], err['dbeta'] = LR.rel_l2(t['dgamma'], dgam), LR.rel_l2(t['dbeta'], dbet)
        assert err['dgamma'] <= 1e-4 and err['dbeta'] <= 1e-4, '%s: gamma / beta gradients %s' % (name, err)
    cs = t['dx'].shape[-1]
    lo, hi = r['dx_coff'], r['dx_coff'] + C
    want = dx + (t['dx0'][..., lo:hi].double() if r['accumulate'] else 0.0)
    got = t['dx'][..., lo:hi]
    if got.dtype == torch.float32:
        err['dx'] = LR.rel_l2(got, want)
        assert err['dx'] <= 1e-4, '%s: dx rel %.2e' % (name, err['dx'])
    else:
        err['dx'] = float((got.double() - want).abs().max() / want.abs().max())
        LR.close_bf16(got, want, name + ' dx')
    if cs != C:
        rest = torch.ones(cs, dtype=torch.bool, device=got.device)
        rest[lo:hi] = False
        assert torch.equal(t['dx'][..., rest], t['dx0'][..., rest]), '%s: channels outside [dx_coff, dx_coff + C) written' % name
    return err


def run_anb(r: dict, dev, seed=0, name='', arena=None) -> dict:
    """Statistics (when norm) then apply, as the step runs them.  arena: operands from it, verified after the parity assertions."""
    from van_gan_amd import ops
    t = anb_operands(r, dev, seed, arena)
    d = anb_desc(r, t)
    if r['norm']:
        ops.actnorm_stats(d)
    ops.actnorm_run(d, stats_done=True)
    torch.cuda.synchronize()
    err = anb_check(r, t, anb_reference(r, t), name)
    if arena is not None:
        arena.verify()
    return err


def run_apply2(r1: dict, r2: dict, dev, seed=0, name='', arena=None) -> dict:
    from van_gan_amd import ops
    t1, t2 = anb_operands(r1, dev, seed, arena), anb_operands(r2, dev, seed + 1, arena)
    d1, d2 = anb_desc(r1, t1), anb_desc(r2, t2)
    for r, d in ((r1, d1), (r2, d2)):
        if r['norm']:
            ops.actnorm_stats(d)
    ops.actnorm_apply2(d1, d2)
    torch.cuda.synchronize()
    e1 = anb_check(r1, t1, anb_reference(r1, t1), name + ' job 1')
    e2 = anb_check(r2, t2, anb_reference(r2, t2), name + ' job 2')
    if arena is not None:
        arena.verify()
    return {k + '1': v for k, v in e1.items()} | {k + '2': v for k, v in e2.items()}


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm finalisation tail
# ----------------------------------------------------------------------------------------------------------------------
def fin_build(recipe, N, cout, dev, seed=0, arena=None):
    """A FinDesc for the recorded jobs with random gamma / beta / mult and a zeroed ticket -> (FinDesc, job tensors).  arena: the ticket
    word, gamma / beta / mult (sealed) and the four output arrays (0xFF bytes: NaN, as without it) are slots of it."""
    from van_gan_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(seed)
    f = _lib.FinDesc()
    tk = LR.dev_out(arena, (4,), torch.int32, dev, 0, 'ticket')
    f.ticket, f.count, f.eps, f.njobs = tk.data_ptr(), float(recipe['fin']['count']), ops.IN_EPS, len(recipe['fin']['jobs'])
    jobs = []
    for j, q in enumerate(recipe['fin']['jobs']):
        ct = q['c_tot']
        jt = dict(c_off=q['c_off'], c_tot=ct, gamma=torch.rand(ct, generator=g, device=dev) + 0.5 if q['gamma'] else None,
                  beta=torch.randn(ct, generator=g, device=dev) * 0.3 if q['beta'] else None,
                  mult=(torch.rand(N, ct, generator=g, device=dev) > 0.3).float() * 2.0 if q['mult'] else None)
        for k in ('gamma', 'beta', 'mult'):
            if arena is not None and jt[k] is not None:
                jt[k] = arena.put(jt[k], name='job %d %s' % (j, k))
        for k in ('scale', 'shift', 'mean', 'rstd'):
            jt[k] = LR.dev_out(arena, (N, ct), torch.float32, dev, float('nan'), 'job %d %s' % (j, k), must_write=True)
        fq = f.job[j]
        fq.gamma, fq.beta, fq.mult = [None if jt[k] is None else jt[k].data_ptr() for k in ('gamma', 'beta', 'mult')]
        fq.scale, fq.shift, fq.mean, fq.rstd = [jt[k].data_ptr() for k in ('scale', 'shift', 'mean', 'rstd')]
        fq.c_off, fq.c_tot = q['c_off'], ct
        jobs.append(jt)
    f._keep = (tk, jobs)
    return f, tk, jobs


def fin_reference(out, count):
    """float64 mean / rstd per (sample, channel) of the stored output, in_finalize's formula (biased variance, IN_EPS inside rsqrt)."""
    from van_gan_amd import ops
    o = out.double()
    N, C = o.shape[0], o.shape[-1]
    o = o.reshape(N, -1, C)
    assert o.shape[1] == count
    mean = o.mean(1)
    var = ((o ** 2).sum(1) / count - mean ** 2).clamp_min(0.0)
    return mean, (var + ops.IN_EPS).rsqrt()


def fin_errors(jobs, mean, rstd, cout):
    """Largest relative L2 error of scale / shift / mean / rstd over the jobs (device tensor: no host sync)."""
    errs = []
    for jt in jobs:
        sl = slice(jt['c_off'], jt['c_off'] + cout)
        gm = jt['gamma'][sl].double() if jt['gamma'] is not None else torch.ones_like(mean[0])
        bt = jt['beta'][sl].double() if jt['beta'] is not None else torch.zeros_like(mean[0])
        sc = gm * rstd
        sh = bt - mean * sc
        if jt['mult'] is not None:
            sc, sh = sc * jt['mult'][:, sl].double(), sh * jt['mult'][:, sl].double()
        for got, want in ((jt['scale'][:, sl], sc), (jt['shift'][:, sl], sh), (jt['mean'][:, sl], mean), (jt['rstd'][:, sl], rstd)):
            e = (got.double() - want).norm() / (want.norm() + 1e-30)
            errs.append(torch.nan_to_num(e, nan=1e30))
    return torch.stack(errs).max()


def fin_untouched(jobs, cout) -> bool:
    """Channels of a job's arrays outside [c_off, c_off + cout) belong to another producer: left alone (still NaN)."""
    ok = True
    for jt in jobs:
        for k in ('scale', 'shift', 'mean', 'rstd'):
            rest = torch.ones(jt['c_tot'], dtype=torch.bool, device=jt[k].device)
            rest[jt['c_off']:jt['c_off'] + cout] = False
            ok &= bool(torch.isnan(jt[k][:, rest]).all())
    return ok


def run_fin(recipe, expect_variant, dev, seed=5, arena=None) -> float:
    """The recorded forward call with its finalisation tail (random contents; the convolution itself is compared with the oracle by
    tests/test_gpu_layers.py): scale / shift / mean / rstd of every job against float64 statistics of the stored output."""
    L = recipe['layer']
    g = torch.Generator().manual_seed(seed)
    st, lay = LR.make_layer_from(L, dev, arena=arena)
    lay.pack()
    sr = recipe['src']
    N = sr['N']
    src, _ = LR.make_operand(sr, L['pad'], dev, g, arena=arena)
    odt = torch.float32 if recipe['out_f32'] else torch.bfloat16
    out = LR.dev_out(arena, (N,) + tuple(lay.out_dims) + (L['cout'],), odt, dev, 0.0, 'out', must_write=True)
    sums = LR.dev_out(arena, (8, N, L['cout'], 2), torch.float32, dev, 0.0, 'out_sums')
    res = rs = rb = None
    if recipe['res']:
        res = LR.dev_in(arena, torch.randn(N, *lay.out_dims, L['cout'], generator=g).to(torch.bfloat16), dev, 'res')
        rs, rb = LR.dev_in(arena, torch.rand(N, L['cout'], generator=g) + 0.5, dev, 'res_scale'), LR.dev_in(arena, torch.randn(N, L['cout'], generator=g), dev, 'res_shift')
    f, _, jobs = fin_build(recipe, N, L['cout'], dev, seed, arena)
    call = lambda: lay.forward(src, out, sums=sums, res=res, res_scale=rs, res_shift=rb, tanh=recipe['tanh'], fin=f)
    assert LR.dry_variants(call) == [expect_variant]
    call()
    torch.cuda.synchronize()
    mean, rstd = fin_reference(out, recipe['fin']['count'])
    err = float(fin_errors(jobs, mean, rstd, L['cout']))
    assert err <= 1e-4, 'finalisation tail rel %.2e' % err
    assert fin_untouched(jobs, L['cout'])
    if arena is not None:
        arena.verify()
    return err


def stress_fin(recipe, expect_variant, dev, launches=200, seed=6, arena=None) -> float:
    """The tail under load: `launches` launches alternating between two streams, each with fresh (zeroed) sums and ticket; every
    launch's finalised statistics within the bound of run_fin.  A last workgroup that reads a stripe before every contribution has
    landed (or a ticket that does not count every workgroup) finalises from partial sums."""
    L = recipe['layer']
    g = torch.Generator().manual_seed(seed)
    st, lay = LR.make_layer_from(L, dev, arena=arena)
    lay.pack()
    sr = recipe['src']
    N = sr['N']
    src, _ = LR.make_operand(sr, L['pad'], dev, g, arena=arena)
    odt = torch.float32 if recipe['out_f32'] else torch.bfloat16
    res = rs = rb = None
    if recipe['res']:
        res = LR.dev_in(arena, torch.randn(N, *lay.out_dims, L['cout'], generator=g).to(torch.bfloat16), dev, 'res')
        rs, rb = LR.dev_in(arena, torch.rand(N, L['cout'], generator=g) + 0.5, dev, 'res_scale'), LR.dev_in(arena, torch.randn(N, L['cout'], generator=g), dev, 'res_shift')
    lanes = []
    for i in range(2):
        out = LR.dev_out(arena, (N,) + tuple(lay.out_dims) + (L['cout'],), odt, dev, 0.0, 'out %d' % i, must_write=True)
        sums = LR.dev_out(arena, (8, N, L['cout'], 2), torch.float32, dev, 0.0, 'out_sums %d' % i)
        f, tk, jobs = fin_build(recipe, N, L['cout'], dev, seed + i, arena)
        lanes.append((out, sums, f, tk, jobs))
    call = lambda ln: lay.forward(src, ln[0], sums=ln[1], res=res, res_scale=rs, res_shift=rb, tanh=recipe['tanh'], fin=ln[2])
    assert LR.dry_variants(lambda: call(lanes[0])) == [expect_variant]
    call(lanes[0])
    torch.cuda.synchronize()
    mean, rstd = fin_reference(lanes[0][0], recipe['fin']['count'])       # the output itself is deterministic
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    worst = [torch.zeros((), dtype=torch.float64, device=dev) for _ in range(2)]
    for i in range(launches):
        ln = lanes[i & 1]
        with torch.cuda.stream(streams[i & 1]):
            ln[1].zero_(); ln[3].zero_()
            for jt in ln[4]:
                for k in ('scale', 'shift', 'mean', 'rstd'):
                    jt[k].fill_(float('nan'))
            call(ln)
            worst[i & 1] = torch.maximum(worst[i & 1], fin_errors(ln[4], mean, rstd, L['cout']))
    torch.cuda.synchronize()
    w = max(float(x) for x in worst)
    assert w <= 1e-4, 'finalisation tail under load: worst rel %.2e over %d launches' % (w, launches)
    if arena is not None:
        arena.verify()               # once, after the loop: a check per launch would serialise the two streams
    return w
