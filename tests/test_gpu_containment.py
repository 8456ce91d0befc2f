"""GPU: where do the kernels read and write?  Workspaces at exactly the size the library asks for, inside guards.

The parity modules run every kernel with far more workspace than any plan needs (160 MB for vg_conv3d, 384 MB for the weight gradients),
so nothing noticed a kernel that used more than its host-side formula grants.  Here every workspace is a slot of a guarded arena
(tests/guarded.py: 0xFF bytes everywhere, at least 1 MiB of guard in front of and behind every slot) of exactly the size under test; the
sizes come from the host-side boundary search of tests/containment_cases.py, which tests/test_containment_host.py checks on the CPU:

  - every gather K-split variant (conv<...>|ks>=2) of the representative lists at S = VG_SCRATCH_CTR_BYTES + cells * ks * one partial
    tile: parity at run_recipe's bounds, guards intact, inputs unchanged, counters back at zero; a second launch into the untouched
    workspace bit-identical (the header's "no state between launches"); at S - 16 the smaller split, without a workspace no split;
  - every conv_dma descriptor (wlayout != 0) of the lists with 1, 2 and 3 samples at exactly vg_conv3d_scratch_bytes, at the smallest
    workspace that keeps its plan where that is less, at counters + operand (K split dropped), and one byte below: VG_EINVAL, nothing
    written;
  - each weight-gradient family whose plan depends on the workspace at its boundary, one float below it (the next plan) and without;
  - vg_spectral_norm at exactly vg_spectral_norm_scratch_bytes and vg_adam_clip with norms[T + 2 * ceil(total / 4096)], all operands
    guarded;
  - whole steps: two train steps of nine engines, a test step and the inference forward on both libraries with the engine's Arena
    replaced by one that leaves a 64 KiB gap of 0xFF behind every allocation (zeros in the zero pool) and recycles nothing inside a
    step -- every gap intact after every step, the losses those of a second engine on the stock Arena;
  - the positive control: a plain torch store into a guard and into an input must be reported by name and offset.

What this cannot see: a read outside an operand whose value a select discards (the halo dummy of DESIGN.md section 4 was one)."""
import math

import pytest
import torch

import containment_cases as CC
import guarded
import layer_recipes as LR

pytestmark = pytest.mark.gpu

_KS = CC.ksplit_cases()
_DMA = CC.dma_cases()
_WG = CC.wgrad_cases()


def _dev():
    return torch.device('cuda:0')


def _report(name, **kw):
    print('%-110s %s' % (name, '  '.join('%s %s' % kv for kv in kw.items())))


# ----------------------------------------------------------------------------------------------------------------------
# positive control: no project kernel, cannot fault
# ----------------------------------------------------------------------------------------------------------------------
def test_guard_check_sees_a_torch_store_on_the_device():
    dev = _dev()
    ar = guarded.GuardedArena(16 << 20, dev)
    a = ar.put(torch.arange(4096, dtype=torch.float32), name='a')
    o = ar.out((5, 7, 3), torch.bfloat16, name='o')
    w = ar.view(1001, name='w', align=16)
    assert bool(torch.isnan(o.float()).all()) and bool((w == 0xFF).all())
    ar.verify()
    so, sw, sa = ar.slot_of(o), ar.slot_of(w), ar.slot_of(a)
    idx = torch.tensor([so.start - 3, so.start - 61456], device=dev)
    ar.buf[idx] = 0                                                  # a plain indexed store inside the arena: in front of `o`
    with pytest.raises(guarded.GuardError) as e:
        ar.check()
    assert "slot 'o'" in str(e.value) and 'front guard, 2 bytes changed, first at -61456, last at -3' in str(e.value)
    assert "slot 'w'" not in str(e.value) and "slot 'a'" not in str(e.value)
    ar.buf[idx] = 0xFF
    ar.check()
    ar.buf[torch.tensor([sw.end, sw.end + 99], device=dev)] = 7      # behind the odd-sized workspace
    with pytest.raises(guarded.GuardError) as e:
        ar.verify()
    assert "slot 'w'" in str(e.value) and 'back guard, 2 bytes changed, first at +0, last at +99' in str(e.value)
    ar.buf[torch.tensor([sw.end, sw.end + 99], device=dev)] = 0xFF
    ar.buf[torch.tensor([sa.start + 4 * 100], device=dev)] ^= 1      # one bit of an input
    ar.check()
    with pytest.raises(guarded.GuardError) as e:
        ar.unchanged(a)
    assert "input slot 'a'" in str(e.value) and 'first at byte 400, last at byte 400' in str(e.value)
    with pytest.raises(guarded.GuardError):
        ar.verify()


# ----------------------------------------------------------------------------------------------------------------------
# vg_conv3d at an exact workspace
# ----------------------------------------------------------------------------------------------------------------------
def _conv_workspace(arena, nbytes):
    """A guarded workspace of exactly nbytes: counters zeroed once (the caller's duty), the rest 0xFF."""
    ws = arena.view(nbytes, name='workspace (%d bytes)' % nbytes)
    ws[:min(CC.CTR, nbytes)].zero_()
    return ws


def _run_at(recipe, variant, nbytes, relaunch=False):
    """run_recipe (parity at its bounds, then guards and inputs) with vg_conv_desc::scratch = a guarded slot of exactly nbytes (None:
    NULL); afterwards the counter bytes are all zero and the guards still intact.  relaunch: a second launch into the workspace as the
    first left it must reproduce the result bit for bit."""
    dev = _dev()
    arena = guarded.GuardedArena(LR.recipe_bytes(recipe) + guarded.slot_cost(nbytes or 0), dev)
    ws = None if nbytes is None else _conv_workspace(arena, nbytes)

    def again(call, result, reset):
        first = result.clone()
        assert bool(torch.isfinite(first.float()).all())
        assert ws is None or not bool(ws[:CC.CTR].any()), 'arrival counters not back at zero after the first launch'
        reset()
        if not recipe.get('accumulate'):
            result.view(torch.uint8).fill_(0xFF)
        call()
        torch.cuda.synchronize()
        assert torch.equal(result, first), 'second launch into the untouched workspace differs: %d elements' % int((result != first).sum())

    with CC.Workspace(nbytes, ws) as w:
        err = LR.run_recipe(recipe, variant, dev, arena=arena, after_launch=again if relaunch else None)
    assert w.seen, 'no vg_conv3d descriptor asked for a workspace'
    if ws is not None:
        assert not bool(ws[:min(CC.CTR, nbytes)].any()), 'arrival counters not left at zero'
    arena.check()
    return err


@pytest.mark.parametrize('cid', sorted(_KS))
def test_ksplit_at_exactly_its_workspace(cid):
    c, b = _KS[cid], CC.ksplit_boundary(cid)
    assert b['S'] == b['expected']
    err = _run_at(c['recipe'], c['variant'], b['S'], relaunch=True)
    _report(cid, S=b['S'], **{k: '%.2e' % v for k, v in err.items()})


@pytest.mark.parametrize('cid', sorted(_KS))
def test_ksplit_16_bytes_short_takes_the_smaller_split(cid):
    c, b = _KS[cid], CC.ksplit_boundary(cid)
    assert CC.ks_of(b['below']) < CC.ks_of(c['variant'])
    _run_at(c['recipe'], b['below'], b['S'] - 16)
    _report(cid, below=b['below'])


@pytest.mark.parametrize('cid', sorted(_KS))
def test_ksplit_without_a_workspace_does_not_split(cid):
    c, b = _KS[cid], CC.ksplit_boundary(cid)
    assert CC.ks_of(b['none']) == 1
    _run_at(c['recipe'], b['none'], None)


@pytest.mark.parametrize('cid', sorted(_DMA))
def test_conv_dma_at_exactly_what_the_library_asks_for(cid):
    """vg_conv3d_scratch_bytes(d) bytes: the roomy plan; where a smaller workspace still keeps it (fewer K slices), that one too."""
    c, b = _DMA[cid], CC.dma_boundary(cid)
    assert b['at_need'] == b['roomy']
    _run_at(c['recipe'], b['roomy'], b['need'], relaunch=True)
    if b['S'] != b['need']:
        _run_at(c['recipe'], b['roomy'], b['S'])
    _report(cid, need=b['need'], S=b['S'], variant=b['roomy'])


@pytest.mark.parametrize('cid', sorted(_DMA))
def test_conv_dma_with_room_for_the_operand_only(cid):
    c, b = _DMA[cid], CC.dma_boundary(cid)
    assert '|ks0|' in b['at_floor']
    _run_at(c['recipe'], b['at_floor'], b['floor'])
    _report(cid, floor=b['floor'], variant=b['at_floor'])


@pytest.mark.parametrize('cid', sorted(_DMA))
def test_conv_dma_one_byte_short_is_refused_and_writes_nothing(cid):
    """Block-layout weights have no other kernel: VG_EINVAL, no launch -- the output slot still all 0xFF, the workspace body too."""
    from van_gan_amd._lib import VgError
    c, b = _DMA[cid], CC.dma_boundary(cid)
    r, dev = c['recipe'], _dev()
    assert r['kind'] == 'dgrad' and b['below_floor'] is None
    L, N = r['layer'], r['N']
    arena = guarded.GuardedArena(LR.recipe_bytes(r) + guarded.slot_cost(b['floor']), dev)
    ws = _conv_workspace(arena, b['floor'] - 1)
    st, lay = LR.make_layer_from(L, dev, arena=arena)
    lay.pack()
    g = torch.Generator().manual_seed(2)
    dy = arena.put(torch.randn(N, *lay.out_dims, L['cout'], generator=g).to(torch.float32 if r['dy_f32'] else torch.bfloat16), name='dy')
    dp = arena.out((N,) + tuple(lay.buf_dims) + (L['cin'],), torch.float32 if r['out_f32'] else torch.bfloat16, None, name='dx')
    with CC.Workspace(b['floor'] - 1, ws):
        with pytest.raises(VgError) as e:
            lay.dgrad(dy, N, dp, accumulate=False)
    assert '(-1)' in str(e.value), str(e.value)                     # VG_EINVAL
    torch.cuda.synchronize()
    assert bool((dp.view(torch.uint8) == 0xFF).all()) and bool((ws[CC.CTR:] == 0xFF).all()) and not bool(ws[:CC.CTR].any())
    arena.verify()


# ----------------------------------------------------------------------------------------------------------------------
# vg_conv3d_wgrad at an exact workspace
# ----------------------------------------------------------------------------------------------------------------------
def _wgrad_at(recipe, variant, nbytes):
    dev = _dev()
    arena = guarded.GuardedArena(LR.recipe_bytes(recipe) + guarded.slot_cost(nbytes), dev)
    sc = arena.view(nbytes, name='weight-gradient workspace (%d bytes)' % nbytes).view(torch.float32) if nbytes else torch.empty(0, device=dev)
    assert nbytes or sc.data_ptr() == 0
    with CC.WgradWorkspace(nbytes, sc):
        err = LR.run_recipe(recipe, variant, dev, arena=arena)       # weight and bias gradient against the oracle at 2e-3, then verify()
    arena.check()
    return err


@pytest.mark.parametrize('fam', sorted(_WG))
def test_weight_gradient_family_at_its_workspace_boundary(fam):
    c = _WG[fam]
    assert c['below'] != c['roomy'] and c['none'] != c['roomy']
    e0 = _wgrad_at(c['recipe'], c['roomy'], c['S'])
    e1 = _wgrad_at(c['recipe'], c['below'], c['S'] - CC.WGRAD_GRANULE)
    e2 = _wgrad_at(c['recipe'], c['none'], 0)
    _report('%s [%s %s]' % (c['roomy'], c['config'], c['layer']), S=c['S'], at_S='%.2e' % e0['w'], below='%s %.2e' % (c['below'], e1['w']),
            none='%s %.2e' % (c['none'], e2['w']))


# ----------------------------------------------------------------------------------------------------------------------
# other caller-sized workspaces of the training path
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2])
def test_spectral_norm_at_exactly_its_scratch(n):
    """tests/test_gpu_specnorm.py's kernel case (its float64 restatement, its 5e-5 bounds) with weights, vectors, state and a scratch of
    exactly vg_spectral_norm_scratch_bytes(total_blocks) bytes as guarded slots, at the 16 bytes the header promises for them."""
    import sn_restate as R
    from van_gan_amd import _lib, ops
    dev = _dev()
    ops.set_device(0)
    arena = guarded.GuardedArena(sum(guarded.slot_cost(4 * K * C_ + 4 * C_) + guarded.slot_cost(0) for K, C_ in R.SHAPES) + (64 << 20), dev)
    Ws, us = zip(*[R.he_normal(K, C_, 100 + i) for i, (K, C_) in enumerate(R.SHAPES)])
    dW = [arena.put(w, name='W%d' % i, align=16, mutable=True) for i, w in enumerate(Ws)]           # projected in place
    du = [arena.put(u, name='u%d' % i, align=16, mutable=True) for i, u in enumerate(us)]
    tab = ops.SpecNormTable(dW, du, dev)
    nb = int(_lib.lib.vg_spectral_norm_scratch_bytes(tab.total_blocks))
    assert nb > 0 and nb % 4 == 0
    tab.scratch = arena.view(nb, name='scratch', align=16).view(torch.float32)     # the caller-owned scratch run() passes, 0xFF on entry
    tab.run(n)
    torch.cuda.synchronize()
    state = tab.state                                   # the table's own state block and item table stay what SpecNormTable built
    for i, (W, u) in enumerate(zip(Ws, us)):
        Wr, ur, sig = W.double().numpy(), u.double().numpy(), []
        for _ in range(n):
            Wr, ur, s = R.project(Wr, ur)
            sig.append(s)
        es = max(abs(float(state[i, p]) - sig[p]) / sig[p] for p in range(n))
        eu, ew = LR.rel_l2(du[i], torch.from_numpy(ur)), LR.rel_l2(dW[i], torch.from_numpy(Wr))
        assert es <= 5e-5 and eu <= 5e-5 and ew <= 5e-5, (W.shape, es, eu, ew)
    arena.verify()


@pytest.mark.parametrize('net', ['gen', 'disc'])
def test_adam_with_norms_of_exactly_the_documented_length(net):
    """vg_adam_clip over a network's table with w, g, m, v, seg_off and norms[T + 2 * ceil(total / 4096)] as guarded slots, some tensors
    clipped: one step against the oracle's float64 Adam at tests/test_gpu_calls.py's bound (1e-6 absolute)."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, disc_param_specs, gen_param_specs
    dev = _dev()
    specs = {'gen': gen_param_specs, 'disc': disc_param_specs}[net]()
    st = ParamStore(specs, dev)
    n_norms = st.T + 2 * ((st.total + 4095) // 4096)
    assert st.norms.numel() == n_norms
    arena = guarded.GuardedArena(4 * guarded.slot_cost(4 * st.total) + 4 * guarded.slot_cost(8 * (st.T + 1) + 4 * n_norms), dev)
    g = torch.Generator().manual_seed(51)
    P = {n: torch.randn(sh, generator=g) * 0.05 for n, sh, _ in specs}
    G = {n: torch.randn(sh, generator=g) * 0.01 for n, sh, _ in specs}
    big = sorted(P, key=lambda n: -P[n].numel())
    for n in big[:3] + big[-3:]:
        G[n] = G[n] * (400.0 / float(G[n].norm()))
    st.load(P)
    for n in P:
        st.grad(n).copy_(G[n])
    w = arena.put(st.w, name='w', mutable=True)
    gr = arena.put(st.g, name='g')
    m, v = arena.out((st.total,), torch.float32, 0.0, name='m'), arena.out((st.total,), torch.float32, 0.0, name='v')
    seg = arena.put(st.seg_off, name='seg_off')
    norms = arena.out((n_norms,), torch.float32, None, name='norms')               # scratch: 0xFF on entry
    scale, lr_t = 0.75, 2e-4 * math.sqrt(1 - 0.9) / (1 - 0.5)
    ops.adam_clip(w, gr, m, v, seg, st.T, norms, lr_t, 0.5, 0.9, 1e-7, 100.0, grad_scale=scale)
    torch.cuda.synchronize()
    Pd, state = {n: t.double() for n, t in P.items()}, {}
    O.adam_step(Pd, {n: t.double() * scale for n, t in G.items()}, state)
    st.w = w
    got = st.export()
    e = max(float((got[n].double().cpu() - Pd[n]).abs().max()) for n in P)
    assert e < 1e-6, e
    arena.verify()


# ----------------------------------------------------------------------------------------------------------------------
# whole steps in a guarded arena
# ----------------------------------------------------------------------------------------------------------------------
GAP = 64 << 10


def _step_arena_class():
    from van_gan_amd import ops

    class GuardedStepArena(ops.Arena):
        """ops.Arena with every byte 0xFF, a gap of GAP bytes behind every allocation and no recycling inside a step: release() joins
        the side stream where the stock code would, and never lowers the offset, so every gap of a step can be checked after it.  Gaps of
        the zero pool stay zero (reset() clears the pool up to its high-water mark) and are checked for zero."""
        ZPOOL = 512 << 20
        made = []

        def __init__(self, nbytes, device):
            super().__init__(nbytes, device)
            self.buf.fill_(0xFF)
            self.gaps, self.zgaps = {}, {}
            type(self).made.append(self)

        def _carve(self, shape, dtype, zero):
            z0 = self.zoff
            t, big_zero = super()._carve(shape, dtype, zero)
            if self.zoff != z0:
                a, b = self.zoff, self.zoff + GAP
                if b > self.ZPOOL:
                    raise MemoryError('guarded zero pool exhausted')
                self.zgaps[a], self.zoff = b, b
            else:
                a, b = self.off, self.off + GAP
                if b > self.buf.numel():
                    raise MemoryError('guarded arena exhausted')
                self.gaps[a], self.off = b, b
                self.peak = max(self.peak, b)
            return t, big_zero

        def release(self, mark, defer=False):
            if defer and self.lazy_ok and ops.SIDE is not None and ops.PROF is None and ops.DRY is None:
                return
            ops.side_join()

        def assert_gaps_intact(self, what):
            torch.cuda.synchronize()
            bad = torch.zeros((), dtype=torch.int64, device=self.buf.device)
            for a, b in self.gaps.items():
                bad = bad + (self.buf[a:b] != 0xFF).sum()
            for a, b in self.zgaps.items():
                bad = bad + (self.zpool[a:b] != 0).sum()
            if int(bad):
                lines = []
                for pool, gaps, fill in ((self.buf, self.gaps, 0xFF), (self.zpool, self.zgaps, 0)):
                    for a, b in sorted(gaps.items()):
                        idx = torch.nonzero(pool[a:b] != fill).view(-1)
                        if idx.numel():
                            lines.append('%s gap at [%d, %d): %d bytes changed, first %d and last %d bytes behind the allocation in front of it'
                                         % ('arena' if fill else 'zero-pool', a, b, idx.numel(), int(idx[0]), int(idx[-1])))
                raise AssertionError('%s: gaps overwritten\n%s' % (what, '\n'.join(lines[:20])))
            return len(self.gaps) + len(self.zgaps)

    return GuardedStepArena


def test_step_arena_gap_check_sees_a_torch_store():
    """Positive control of the whole-step check: a plain torch store into a recorded gap of the arena and of the zero pool (no project
    kernel) must be reported, with its distance to the allocation in front of it."""
    dev = _dev()
    ar = _step_arena_class()(64 << 20, dev)
    a = ar.alloc((1000,), torch.float32)
    z = ar.alloc((16,), torch.float32, zero=True)
    ar.alloc((3, 5), torch.bfloat16)
    assert bool(torch.isnan(a).all()) and bool((z == 0).all())
    assert ar.assert_gaps_intact('fresh') == 3
    a_end = a.data_ptr() - ar.buf.data_ptr() + 4000
    ar.buf[torch.tensor([a_end + 7], device=dev)] = 0
    with pytest.raises(AssertionError) as e:
        ar.assert_gaps_intact('control')
    assert 'arena gap at [%d, %d): 1 bytes changed, first 7 and last 7 bytes' % (a_end, a_end + GAP) in str(e.value) and 'zero-pool' not in str(e.value)
    ar.buf[torch.tensor([a_end + 7], device=dev)] = 0xFF
    z_end = z.data_ptr() - ar.zpool.data_ptr() + 64
    ar.zpool[torch.tensor([z_end, z_end + GAP - 1], device=dev)] = 1
    with pytest.raises(AssertionError) as e:
        ar.assert_gaps_intact('control')
    assert 'zero-pool gap at [%d, %d): 2 bytes changed, first 0 and last %d bytes' % (z_end, z_end + GAP, GAP - 1) in str(e.value)
    ar.zpool[torch.tensor([z_end, z_end + GAP - 1], device=dev)] = 0
    assert ar.assert_gaps_intact('restored') == 3


def _engines(monkeypatch, dims, B, precision, **kw):
    """(engine in guarded arenas, two engines of the same seed and weights on the stock Arena, the guarded arenas, real_I, real_S).  The
    second stock engine measures, inside the test, how far two engines on the stock Arena are apart: the reference's own spread."""
    import van_gan_amd.vangan as V
    from van_gan_amd.synth import synth_volumes
    S = dims[0] * dims[1] * dims[2]
    stock = V.VanGan(dims, batch_size=B, device='cuda:0', seed=3, precision=precision, **kw)
    other = V.VanGan(dims, batch_size=B, device='cuda:0', seed=3, precision=precision, **kw)
    cls = _step_arena_class()
    monkeypatch.setattr(V, 'Arena', cls)
    nbytes = max(4 << 30, B * S * 8000 * 8 * (2 if precision == 'fp32' else 1)) + (2 << 30)       # nothing is recycled inside a step
    guard = V.VanGan(dims, batch_size=B, device='cuda:0', seed=3, precision=precision, arena_bytes=nbytes, **kw)
    monkeypatch.undo()
    assert len(cls.made) >= 1 and all(isinstance(a, cls) for a in (guard.arena, guard.arena_b) if a is not None)
    assert not isinstance(stock.arena, cls) and not isinstance(other.arena, cls)
    for e in (guard, other):
        e.load_weights(stock.export_weights())
    rI, rS = synth_volumes(B, *dims, seed=7)
    return guard, stock, other, cls.made, rI.cuda(), rS.cuda()


def _finite_params(eng):
    return all(bool(torch.isfinite(st.w).all()) for st in eng.stores.values())


def _grad_distance(a, b):
    """Per network (1 - cosine, relative L2) of the flat gradients of two engines: what tests/test_gpu_graph.py's _grads_agree measures."""
    from van_gan_amd.vangan import NETS
    ga, gb = a.export_grads(), b.export_grads()
    out = {}
    for n in NETS:
        fa = torch.cat([t.flatten() for t in ga[n].values()]).double()
        fb = torch.cat([t.flatten() for t in gb[n].values()]).double()
        out[n] = (1.0 - float((fa @ fb) / (fa.norm() * fb.norm() + 1e-300)), float((fa - fb).norm() / (fa.norm() + 1e-300)))
    return out


def _weight_distance(a, b):
    from van_gan_amd.vangan import NETS
    wa, wb = a.export_weights(), b.export_weights()
    return max(float((wa[n][k].double() - wb[n][k].double()).abs().max()) for n in NETS for k in wa[n])


_ENGINES = {
    '32^3 B1 fp32': ((32, 32, 32), 1, 'fp32', {}),
    '32^3 B1 bf16': ((32, 32, 32), 1, 'bf16', {}),
    '32x48x80 B1 bf16': ((32, 48, 80), 1, 'bf16', {}),                      # the ragged walk in which the halo bug lived
    '32^3 B3 bf16': ((32, 32, 32), 3, 'bf16', {}),
    'resnet': ((32, 32, 32), 1, 'bf16', dict(generator='resnet')),
    'attention gate': ((32, 32, 32), 1, 'bf16', dict(attention_gate=True)),
    'spectral norm': ((32, 32, 32), 1, 'bf16', dict(spectral_norm=True)),
    'wasserstein': ((32, 32, 32), 1, 'bf16', dict(wasserstein=True, lr=1e-4, beta_1=0.0, beta_2=0.9, clipnorm=0)),
    'L4 / mae cycle losses, bfce': ((32, 32, 32), 1, 'bf16', dict(cycle_loss_SIS='L4', cycle_loss_ISI='mae', gan_loss='bfce')),
}


# Engines whose second step runs on re-synchronised weights (see the test): two engines on the STOCK Arena are themselves as far apart
# as the bf16 bound after one Adam step there (measured, three pairs each: ResNet generator 0.43 / 0.97 / 1.05 of the bound, attention gate
# 0.49 / 0.54 / 0.90 and 0.25 / 0.52 / 0.98, Wasserstein 0.19 / 1.00 / 1.02; spectral norm 0.16 - 0.39, the loss types 0.06 - 0.30 and
# the default engines 0.02 - 0.24 stay as they are).
_RESYNC = ('resnet', 'attention gate', 'wasserstein')

# (1 - cosine, relative L2) two engines' flat gradients of one network may be apart.  fp32: tests/test_gpu_graph.py's _grads_agree (two
# stock engines measured 3e-7 - 3.7e-5 and 8e-4 - 8.6e-3).  bf16: no bound exists in the suite, and two engines on the stock Arena are
# far apart by themselves -- over 27 pairs of the nine engines 1 - cos up to 0.22 and rel up to 0.70 for the generators, in discrete levels
# (the ResNet generator's gen_IS: 7.5e-3 or 0.24): 16-bit roundings and arg-extrema of the min-max flip with the float atomics.  The bound
# is what tells that spread from a wrong gradient: a missing or mis-signed contribution of the size of the gradient gives rel >= 1.
_GRAD_BOUND = {'fp32': (1e-4, 1e-2), 'bf16': (0.5, 1.0)}


def _loss_tol(precision, x, equal_weights):
    if precision == 'fp32':
        return 2e-5 * abs(x) + 1e-7 if equal_weights else 1e-2 * abs(x) + 1e-6
    return 5e-2 * abs(x) + 1e-3


@pytest.mark.parametrize('name', list(_ENGINES))
def test_train_steps_stay_inside_their_allocations(name, monkeypatch):
    """Two train steps (the second on the cached allocation sequence) with every Arena allocation followed by a 64 KiB gap of 0xFF
    (zeros in the zero pool) and nothing recycled, beside two engines of the same seed on the stock Arena.  After each step every gap
    intact, the ten losses and all parameters finite, and the losses those of the first stock engine within tests/test_gpu_graph.py's
    bounds for two engines: fp32 2e-5 |x| + 1e-7 where the weights are equal, 1e-2 |x| + 1e-6 after an Adam step; bf16 5e-2 |x| + 1e-3.
    A step that goes non-finite only here would be a kernel consuming memory it never wrote.
    What the guarded backward sweep and optimizer produced is compared after the FIRST step, before anything is reloaded: the flat
    gradient of every network at _GRAD_BOUND (fp32: _grads_agree's cosine > 0.9999 and relative L2 < 1e-2; bf16: see there) -- or, where
    two engines on the stock Arena are further apart themselves, within three times their distance, measured here with the second stock
    engine -- and every weight
    after Adam within 2 lr of the stock engine's: a first Adam update moves a weight by at most lr whatever its gradient (m / sqrt(v) =
    +-1, clipping only shrinks it), so two engines whose gradients differ in sign somewhere are 2 lr apart there and no further (not for
    the spectrally normalised discriminators, whose kernels are also divided by sigma, nor the Wasserstein critic).
    The second step follows the first with nothing reloaded, at the bounds above -- except for the engines of _RESYNC, where the guarded
    and the second stock engine take the first stock engine's weights again before it and the bound is the equal-weights one: that
    sign-like first update turns the last bit of the float atomics into weight differences of lr (every pair measured ends exactly 2 lr
    apart), and two engines on the STOCK Arena then differ at the second step by as much as the bound (figures at _RESYNC; guarded
    engines measured 0.11 - 1.19 with the attention gate, 0.40 and 1.48 with the ResNet generator, 1.61 Wasserstein): the engines' own
    spread, not the arena's -- with equal weights the second step checks the cached allocation sequence in the guarded arena."""
    from van_gan_amd.vangan import RESULT_KEYS
    dims, B, precision, kw = _ENGINES[name]
    guard, stock, other, arenas, rI, rS = _engines(monkeypatch, dims, B, precision, **kw)
    assert len(RESULT_KEYS) == 10
    equal = True
    for step in range(2):
        rg = guard.train_step(rI, rS)
        ngaps = sum(a.assert_gaps_intact('%s step %d' % (name, step)) for a in arenas)
        rs, ro = stock.train_step(rI, rS), other.train_step(rI, rS)
        worst = 0.0
        for k in RESULT_KEYS:
            assert math.isfinite(rg[k]), (step, k, rg[k])
            tol = _loss_tol(precision, rs[k], equal)
            worst = max(worst, abs(rg[k] - rs[k]) / tol)
            assert abs(rg[k] - rs[k]) <= tol, (step, k, rg[k], rs[k], 'two stock engines: %r' % ro[k])
        assert _finite_params(guard)
        rep = dict(gaps=ngaps, worst_loss='%.2f of bound' % worst, peak_MB=sum(a.peak for a in arenas) >> 20)
        if step == 0:
            dg, ds = _grad_distance(guard, stock), _grad_distance(other, stock)
            for n in dg:
                b = _GRAD_BOUND[precision]
                assert dg[n][0] < max(b[0], 3 * ds[n][0]) and dg[n][1] < max(b[1], 3 * ds[n][1]), (n, 'guarded vs stock', dg[n], 'stock vs stock', ds[n])
            rep.update(grad_rel='%.1e (stock pair %.1e)' % (max(v[1] for v in dg.values()), max(v[1] for v in ds.values())))
            wd = _weight_distance(guard, stock)
            rep.update(weights='%.2f lr' % (wd / guard.lr))
            if not (kw.get('spectral_norm') or kw.get('wasserstein')):
                assert wd <= 2 * guard.lr * (1 + 1e-3) + 1e-6, (wd, guard.lr)
            if name in _RESYNC:
                for e in (guard, other):
                    e.load_weights(stock.export_weights())
            else:
                equal = False
        _report('%s step %d' % (name, step), **rep)
    assert ngaps > 500


def test_test_step_stays_inside_its_allocations(monkeypatch):
    from van_gan_amd.vangan import RESULT_KEYS
    guard, stock, _, arenas, rI, rS = _engines(monkeypatch, (32, 48, 80), 1, 'bf16')
    rg = guard.test_step(rI, rS)
    ngaps = sum(a.assert_gaps_intact('test_step') for a in arenas)
    rs = stock.test_step(rI, rS)
    for k in RESULT_KEYS:
        assert math.isfinite(rg[k]) and abs(rg[k] - rs[k]) <= 5e-2 * abs(rs[k]) + 1e-3, (k, rg[k], rs[k])
    assert ngaps > 100


@pytest.mark.parametrize('lib', ['bf16', 'fp16'])
def test_inference_forward_stays_inside_its_allocations(lib, monkeypatch):
    """ResUNet.forward(save=False) on two 32x48x80 windows, on both libraries: the block temporaries the stock Arena recycles are kept
    apart here.  Gaps intact, the volume finite (an allocation consumed before it was written would be NaN here), and the volume that of
    an engine on the stock Arena as closely as a SECOND engine on the stock Arena reproduces it: no bound for single voxels of two
    16-bit engines is known (the InstanceNorm statistics are float atomics, a flipped 16-bit rounding travels through nine levels), so
    the reference's own spread is measured beside it -- relative L2 and largest difference of the guarded volume within three times
    those of the two stock engines (measured, four stock pairs and two guarded ones per library: bf16 rel 1.4e-2 - 1.6e-2 and largest
    difference 0.097 - 0.123 against 1.4e-2 - 1.7e-2 and 0.106 - 0.127; fp16 2.2e-3 - 2.4e-3 and 0.016 - 0.019 against 2.2e-3 - 2.3e-3 and
    0.017 - 0.023; outputs in [-1, 1], rms 0.82)."""
    from van_gan_amd import ops
    guard, stock, other, arenas, rI, rS = _engines(monkeypatch, (32, 48, 80), 2, 'bf16')
    outs = []
    for eng in (guard, stock, other):
        if lib == 'bf16':
            outs.append(eng.generate('gen_IS', rI))
        else:
            net = eng.fp16_generator('gen_IS')
            out = torch.full(rI.shape, float('nan'), device=rI.device)
            with ops.Fp16():
                eng.arena.reset()
                net.forward(eng.arena, rI, out, save=False)
            outs.append(out)
        torch.cuda.synchronize()
    ngaps = guard.arena.assert_gaps_intact('inference forward, %s library' % lib)
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    dist = lambda a, b: (LR.rel_l2(a, b), float((a - b).abs().max()))
    dg, ds = dist(outs[0], outs[1]), dist(outs[2], outs[1])
    _report('inference forward, %s library' % lib, gaps=ngaps, guarded_vs_stock='rel %.3e max %.3e' % dg, stock_vs_stock='rel %.3e max %.3e' % ds)
    assert dg[0] <= 3 * ds[0] and dg[1] <= 3 * ds[1], ('guarded vs stock', dg, 'stock vs stock', ds)
    assert ngaps > 50
