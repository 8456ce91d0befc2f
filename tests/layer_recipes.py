"""Which kernel variants do the BASELINE configurations run, and a parity case at a TRUE LAYER SHAPE for each of them.

The schedules of van_gan_amd/nets.py (generator forward + backward, discriminator forward + both backward sweeps) are walked
on the CPU in `ops.DryRun` mode: every vg_conv3d / vg_conv3d_wgrad call runs its complete host-side dispatch without
launching and reports the kernel variant it selected (template arguments + run-time regime, include/vangan_hip.h:
vg_conv3d_variant), together with a shape-level recipe of the call.  For every variant the cheapest call that selects it
becomes its representative; tests/test_gpu_layers.py replays the representative on the GPU with random contents and
compares it with the oracle's convolution (autograd for the two gradients), tests/test_variant_coverage.py (CPU) proves the
representatives cover every variant of BASELINE configs 2, 3 and 4.  The same for the sliding-window inference forward
(INFER_CONFIGS; tests/test_gpu_infer_layers.py) and for patches whose level grids are no powers of two (RAGGED_CONFIGS /
RAGGED_INFER_CONFIGS; tests/test_gpu_ragged.py, tests/test_ragged_coverage.py), and for the train steps at the reference's own
per-GPU batch of three (BATCH3_CONFIGS; tests/test_gpu_batch3.py, tests/test_batch3_coverage.py).

Helper module (no tests in here)."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

# name -> (patch dims, per-replica batch).  The first three are BASELINE.json configs 2, 3 and 4 (per-GPU workload of the
# 8-GPU run); 32^3 (config 1) only donates cheaper representatives of variants it shares with them.
CONFIGS = {
    '128^3 B1': ((128, 128, 128), 1),
    '64^3 B2': ((64, 64, 64), 2),
    '128x128x64 B2': ((128, 128, 64), 2),
    '32^3 B1': ((32, 32, 32), 1),
}
NEEDED = ('128^3 B1', '64^3 B2', '128x128x64 B2')


def enumerate_config(dims, B, precision='bf16'):
    """-> [(kind, layer name, variant, recipe)] of one train step's conv launches (one generator: a forward application and the
    backward sweep over both applications; one discriminator with its two backward sweeps: the others repeat the same calls)."""
    return walk_config(dims, B, precision)[0]


def walk_config(dims, B, precision='bf16'):
    """-> (enumerate_config's list, [(entry point, regime)] of the same walk's non-convolution calls: ops.DryRun.calls)."""
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, PatchGAN, ResUNet, disc_param_specs, gen_param_specs
    dt = torch.bfloat16 if precision == 'bf16' else torch.float32
    S = dims[0] * dims[1] * dims[2]
    G = ResUNet(ParamStore(gen_param_specs(), 'cpu'), dims, dt)
    D = PatchGAN(ParamStore(disc_param_specs(), 'cpu'), dims, dt)
    ar = ops.Arena(int(B * S * 5200 * 2) + (512 << 20), 'cpu')          # never touched: dry runs do not write
    with ops.DryRun() as dry:
        # as in VanGan._losses_and_backward: the two applications of a generator are B-sample forward passes into paired 2B-sample
        # tensors and ONE 2B-sample backward sweep (the second forward repeats the first one's calls: not recorded twice)
        from van_gan_amd.nets import pair_ctx
        x2 = ar.alloc((2 * B,) + dims + (1,), torch.float32)
        y, yb = ar.alloc((B,) + dims + (1,), torch.float32), ar.alloc((B,) + dims + (1,), torch.float32)
        ar.pair_begin('g', 0)
        ctx = G.forward(ar, x2[:B], y)
        ar.pair_end()
        n0, c0 = len(dry.records), len(dry.calls)
        ar.pair_begin('g', 1)
        G.forward(ar, x2[B:], yb)
        ar.pair_end()
        del dry.records[n0:]; del dry.recipes[n0:]; del dry.calls[c0:]
        G.backward(ar, pair_ctx(ar, ctx, x2, (y, yb), G.lv[0]), x2)
        lg = ar.alloc((2 * B,) + tuple(n // 8 for n in dims) + (1,), torch.float32)
        noise = {k: torch.empty(shp, dtype=torch.bfloat16) for k, shp in D.noise_shapes(2 * B).items()}
        drop = {k: torch.empty(2 * B, c) for k, c in (('down0', 128), ('down1', 256), ('down2', 512))}
        dctx = D.forward(ar, x2, lg, noise, drop)
        # the step's discriminator backward: ONE sweep over [d critic loss (2B); d generator loss (B)] (PatchGAN.backward_both)
        lg3 = ar.alloc((3 * B,) + tuple(n // 8 for n in dims) + (1,), torch.float32)
        D.backward_both(ar, dctx, lg3, B, ar.alloc((B,) + dims + (1,), torch.float32))
    return [(k, n, v, r) for (k, n, v), r in zip(dry.records, dry.recipes)], list(dry.calls)


def enumerate_resnet(dims, N):
    """[(kind, layer, variant)] of one application (forward + backward) of the ResNet generator in dry-run mode."""
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, ResNetGenerator, resnet_param_specs
    G = ResNetGenerator(ParamStore(resnet_param_specs(), 'cpu'), dims, torch.bfloat16)
    ar = ops.Arena(int(N * dims[0] * dims[1] * dims[2] * 9000) + (512 << 20), 'cpu')
    with ops.DryRun() as dry:
        x, y = torch.empty((N,) + dims + (1,)), torch.empty((N,) + dims + (1,))
        drop = {k: torch.empty(N, c) for k, c in ResNetGenerator.DROP_CH.items()}
        G.backward(ar, G.forward(ar, x, y, drop), y)
    return list(dry.records)


def recipe_macs(r) -> float:
    L = r['layer']
    out = [(-(-n // L['stride'])) for n in L['in_dims']]
    N = r['src']['N'] if 'src' in r else r['N']
    return float(N) * math.prod(out) * L['cin'] * L['cout'] * L['k'] ** 3


@functools.lru_cache(maxsize=None)
def all_records(precision='bf16'):
    return {name: enumerate_config(dims, B, precision) for name, (dims, B) in CONFIGS.items()}


@functools.lru_cache(maxsize=None)
def representatives(precision='bf16') -> Dict[Tuple[str, str], dict]:
    """(kind, variant) -> {'recipe', 'config', 'layer', 'macs'}: the cheapest call that selects the variant."""
    best: Dict[Tuple[str, str], dict] = {}
    for cfg, recs in all_records(precision).items():
        for kind, name, variant, recipe in recs:
            key, m = (kind, variant), recipe_macs(recipe)
            if key not in best or m < best[key]['macs']:
                best[key] = dict(recipe=recipe, config=cfg, layer=name, macs=m)
    return best


def needed_variants(precision='bf16'):
    recs = all_records(precision)
    return sorted({(k, v) for cfg in NEEDED for (k, _, v, _) in recs[cfg]})


# ----------------------------------------------------------------------------------------------------------------------
# the sliding-window inference forward: ResUNet.forward(save=False) on window batches (VanGan.stitch_subvolumes)
# ----------------------------------------------------------------------------------------------------------------------
# name -> (window dims, windows per batch).  The first two are what the published inference line runs (128^3 windows, two per batch,
# and the one-window tail batch of an odd window count); the small ones only donate cheaper representatives, as '32^3 B1' does above.
INFER_CONFIGS = {
    'infer 128^3 N2': ((128, 128, 128), 2),
    'infer 128^3 N1': ((128, 128, 128), 1),
    'infer 64^3 N2': ((64, 64, 64), 2),
    'infer 32^3 N2': ((32, 32, 32), 2),
}
INFER_NEEDED = ('infer 128^3 N2', 'infer 128^3 N1')


def walk_inference(dims, N, dtype=torch.bfloat16):
    """-> ([(kind, layer name, variant, recipe)], [(entry point, regime)]) of ONE forward-only application of the ResUNet generator on
    N windows, as the sliding-window path runs it (block temporaries recycled).  dtype: the network's storage type (torch.float16 is
    the libvangan_hip_h.so engine; the dispatch is host logic shared by both builds)."""
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, ResUNet, gen_param_specs
    G = ResUNet(ParamStore(gen_param_specs(), 'cpu'), dims, dtype)
    ar = ops.Arena(int(N * dims[0] * dims[1] * dims[2] * 5200) + (512 << 20), 'cpu')     # never touched: dry runs do not write
    with ops.DryRun() as dry:
        x, y = ar.alloc((N,) + tuple(dims) + (1,), torch.float32), ar.alloc((N,) + tuple(dims) + (1,), torch.float32)
        G.forward(ar, x, y, save=False)
    return [(k, n, v, r) for (k, n, v), r in zip(dry.records, dry.recipes)], list(dry.calls)


@functools.lru_cache(maxsize=None)
def all_inference_walks():
    return {name: walk_inference(dims, N) for name, (dims, N) in INFER_CONFIGS.items()}


def inference_needed_variants():
    walks = all_inference_walks()
    return sorted({(k, v) for cfg in INFER_NEEDED for (k, _, v, _) in walks[cfg][0]})


def recipe_variant(recipe) -> str:
    """The variant a recorded FORWARD call selects, by a CPU dry run of the rebuilt call (no contents: empty tensors)."""
    got = dry_variants(empty_call(recipe))
    assert len(got) == 1
    return got[0]


def empty_call(recipe):
    """The call run_recipe rebuilds from `recipe`, on empty CPU tensors, as a function to issue inside ops.DryRun -- once per workspace
    size when a test searches the size at which the plan changes (tests/containment_cases.py)."""
    if recipe['kind'] != 'fwd':
        return _empty_grad_call(recipe)
    from van_gan_amd.ops import Src
    assert recipe['kind'] == 'fwd'
    L, sr = recipe['layer'], recipe['src']
    _, lay = make_layer_from(L, 'cpu')
    N, dims, c0, c1, sh = sr['N'], tuple(sr['dims']), sr['c0'], sr['c1'], sr['shift0']
    e = lambda *shp, dt=torch.bfloat16: torch.empty(*shp, dtype=dt)
    src = Src(e(N, *[n >> sh for n in dims], c0, dt=torch.float32 if sr['f32'] else torch.bfloat16), (N,) + dims, c0,
              e(N, *dims, c1) if c1 else None, c1, shift0=sh, f32=sr['f32'],
              scale=e(N, c0 + c1, dt=torch.float32) if sr['affine'] else None, shift=e(N, c0 + c1, dt=torch.float32) if sr['affine'] else None,
              act=sr['act'], noise=e(N, *[n + 2 * sr['noise_pad'] for n in dims], c0 + c1) if sr['noise'] else None, noise_pad=sr['noise_pad'])
    out = e(N, *lay.out_dims, L['cout'], dt=torch.float32 if recipe['out_f32'] else torch.bfloat16)
    pc = lambda: e(N, L['cout'], dt=torch.float32)
    sums, res = e(8, N, L['cout'], 2, dt=torch.float32) if recipe['sums'] else None, e(N, *lay.out_dims, L['cout']) if recipe['res'] else None
    rs, rb = (pc(), pc()) if recipe['res'] else (None, None)
    return lambda: lay.forward(src, out, sums=sums, res=res, res_scale=rs, res_shift=rb, tanh=recipe['tanh'])


SHRINK_ABOVE = 1e9          # MACs: cheaper calls are replayed as recorded (a shrunk grid has fewer tiles and fewer workgroups)


def shrink_recipe(recipe, variant):
    """A cheaper forward call of the same layer that selects the IDENTICAL variant string: one sample instead of several, axes halved
    (greedily, while the call costs more than SHRINK_ABOVE and the CPU dry run of the shrunk call still reports `variant`).  The recorded finalisation tail keeps its jobs; its
    voxel count follows the output grid."""
    def with_shape(r, N, dims):
        L = dict(r['layer'], in_dims=tuple(dims))
        out = dict(r, layer=L, src=dict(r['src'], N=N, dims=tuple(dims)))
        if r.get('fin'):
            s, k = L['stride'], L['k']
            od = [(n + 2 - k) // s + 1 if L['pad'] == 'reflect' else -(-n // s) for n in dims]
            out['fin'] = dict(r['fin'], count=float(math.prod(od)))
        return out

    best, moved = recipe, True
    while moved and recipe_macs(best) > SHRINK_ABOVE:
        moved = False
        N, dims = best['src']['N'], tuple(best['src']['dims'])
        tries = [(1, dims)] if N > 1 else []
        tries += [(N, dims[:a] + (dims[a] // 2,) + dims[a + 1:]) for a in range(3) if dims[a] % 4 == 0 and dims[a] >= 16]
        for n_, d_ in tries:
            cand = with_shape(best, n_, d_)
            try:
                same = recipe_variant(cand) == variant
            except Exception:                       # no tile plan for the shrunk grid: not a candidate
                same = False
            if same:
                best, moved = cand, True
                break
    return best


@functools.lru_cache(maxsize=None)
def inference_representatives() -> Dict[Tuple[str, str], dict]:
    """(kind, variant) -> {'recipe', 'config', 'layer', 'macs'} for every variant of the inference walks: the cheapest call over those
    walks and the training walks, shrunk further where the dispatch keeps the variant (shrink_recipe).  representatives() is not
    touched: it stays the case list of tests/test_gpu_layers.py."""
    walks = {cfg: recs for cfg, (recs, _) in all_inference_walks().items()}
    keys = {(k, v) for recs in walks.values() for (k, _, v, _) in recs}
    best: Dict[Tuple[str, str], dict] = {}
    for cfg, recs in list(walks.items()) + list(all_records().items()):
        for kind, name, variant, recipe in recs:
            key, m = (kind, variant), recipe_macs(recipe)
            if key in keys and (key not in best or m < best[key]['macs']):
                best[key] = dict(recipe=recipe, config=cfg, layer=name, macs=m)
    for key, b in best.items():
        r = shrink_recipe(b['recipe'], key[1])
        if r is not b['recipe']:
            b.update(recipe=r, macs=recipe_macs(r), shrunk=True)
    return best


def inference_only_variants():
    """The variants of the two NEEDED inference walks that no train step of BASELINE configs 1-4 selects."""
    reps = representatives()
    return sorted(kv for kv in inference_needed_variants() if kv not in reps)


# ----------------------------------------------------------------------------------------------------------------------
# ragged patches: legal patch sizes (axes multiples of 16, at least 32) whose level grids are no powers of two
# ----------------------------------------------------------------------------------------------------------------------
# 32x48x80 is the smallest legal patch with three different axes (level grids 16x24x40, 8x12x20, 4x6x10, bridge 2x3x5); 48x80x96 has no
# power-of-two axis (24x40x48, 12x20x24, 6x10x12, bridge 3x5x6).  Batch 2 changes the dispatch of the first.  Nothing above this line
# depends on these: CONFIGS / INFER_CONFIGS and the case lists derived from them stay what they are.
RAGGED_CONFIGS = {
    '32x48x80 B1': ((32, 48, 80), 1),
    '32x48x80 B2': ((32, 48, 80), 2),
    '48x80x96 B1': ((48, 80, 96), 1),
}
RAGGED_INFER_CONFIGS = {
    'infer 32x48x80 N2': ((32, 48, 80), 2),
    'infer 48x80x96 N2': ((48, 80, 96), 2),
    'infer 48x80x96 N1': ((48, 80, 96), 1),
}


@functools.lru_cache(maxsize=None)
def all_ragged_walks():
    """config -> (conv records, non-convolution calls): the train walks of RAGGED_CONFIGS, then the inference walks of RAGGED_INFER_CONFIGS."""
    walks = {name: walk_config(dims, B) for name, (dims, B) in RAGGED_CONFIGS.items()}
    walks.update({name: walk_inference(dims, N) for name, (dims, N) in RAGGED_INFER_CONFIGS.items()})
    return walks


def _cheapest(walks, keep=lambda kind, variant: True):
    best: Dict[Tuple[str, str], dict] = {}
    for cfg, (recs, _) in walks.items():
        for kind, name, variant, recipe in recs:
            key, m = (kind, variant), recipe_macs(recipe)
            if keep(kind, variant) and (key not in best or m < best[key]['macs']):
                best[key] = dict(recipe=recipe, config=cfg, layer=name, macs=m)
    return best


@functools.lru_cache(maxsize=None)
def ragged_representatives() -> Dict[Tuple[str, str], dict]:
    """(kind, variant) -> {'recipe', 'config', 'layer', 'macs'} for every variant of the ragged walks: the cheapest call OF A RAGGED WALK
    that selects it, replayed as recorded (never a power-of-two call that shares the string, never shrunk: the partial tiles of the
    recorded grid are what the case is for)."""
    return _cheapest(all_ragged_walks())


@functools.lru_cache(maxsize=None)
def ragged_inference_representatives() -> Dict[Tuple[str, str], dict]:
    """The same for the forward variants of the ragged INFERENCE walks alone, each from one of those walks (the fp16 library's cases)."""
    return _cheapest({cfg: w for cfg, w in all_ragged_walks().items() if cfg in RAGGED_INFER_CONFIGS})


def ragged_only_variants():
    """The (kind, variant) pairs of the ragged walks that neither representatives() nor inference_representatives() has a case for."""
    have = set(representatives()) | set(inference_representatives())
    return sorted(kv for kv in ragged_representatives() if kv not in have)


# ----------------------------------------------------------------------------------------------------------------------
# batch 3: the reference's own per-GPU training batch
# ----------------------------------------------------------------------------------------------------------------------
# The generator's kernels run at N = 3 and 6, the discriminator's at N = 6 and 9 (backward_both's 3B launch); every other walk of this
# module has a batch of 1 or 2.  The four power-of-two patches of CONFIGS and the smallest ragged one; the sliding-window inference does
# not depend on the training batch: no inference walks.  Nothing above this line depends on these.  (walk_config's dry-run arena is an
# untouched torch.empty of B * S * 10400 bytes: 65 GB of address space at 128^3 B3, none of it ever written.)
BATCH3_CONFIGS = {
    '32^3 B3': ((32, 32, 32), 3),
    '64^3 B3': ((64, 64, 64), 3),
    '128x128x64 B3': ((128, 128, 64), 3),
    '128^3 B3': ((128, 128, 128), 3),
    '32x48x80 B3': ((32, 48, 80), 3),
}
BATCH3_N = (3, 6, 9)


@functools.lru_cache(maxsize=None)
def all_batch3_walks():
    """config -> (conv records, non-convolution calls): the train walks of BATCH3_CONFIGS."""
    return {name: walk_config(dims, B) for name, (dims, B) in BATCH3_CONFIGS.items()}


def recipe_n(recipe) -> int:
    return recipe['src']['N'] if 'src' in recipe else recipe['N']


def macs_cap() -> float:
    """No case of a later module is heavier than the heaviest one of tests/test_gpu_layers.py (down2's data gradient at 128^3 B1)."""
    return max(r['macs'] for r in representatives().values())


def shrink_call(recipe, variant, cap):
    """shrink_recipe for all three kinds and for a batch that has to stay what it is: a cheaper call of the same layer with the SAME
    number of samples for which the CPU dry run of the rebuilt call (replay_variant) still reports `variant` -- one axis halved at a
    time, greedily, until the call costs no more than `cap` MACs.  Returns `recipe` itself if no such call exists."""
    def with_dims(r, dims):
        out = dict(r, layer=dict(r['layer'], in_dims=tuple(dims)))
        if 'src' in r:
            out['src'] = dict(r['src'], dims=tuple(dims))
        if r.get('fin'):
            out['fin'] = dict(r['fin'], count=float(math.prod(out_grid(out))))
        return out

    best, moved = recipe, True
    while moved and recipe_macs(best) > cap:
        moved = False
        dims = tuple(best['layer']['in_dims'])
        for a in sorted(range(3), key=lambda a: -dims[a]):
            if dims[a] % 4 or dims[a] < 16:
                continue
            cand = with_dims(best, dims[:a] + (dims[a] // 2,) + dims[a + 1:])
            try:
                same = replay_variant(cand) == variant
            except Exception:                       # no tile plan for the shrunk grid: not a candidate
                same = False
            if same:
                best, moved = cand, True
                break
    return best if recipe_macs(best) <= cap else recipe


@functools.lru_cache(maxsize=None)
def batch3_representatives() -> Dict[Tuple[str, str], dict]:
    """(kind, variant) -> {'recipe', 'config', 'layer', 'macs'} for every variant of the batch-3 walks: the cheapest call OF A BATCH-3 WALK
    that selects it, replayed as recorded -- N = 3, 6 or 9 -- unless it costs more than macs_cap(): then with axes halved while the dry
    run keeps the identical variant string (shrink_call; 'shrunk': True, 'recorded': the walk's own recipe).  The batch is never
    touched."""
    best = _cheapest(all_batch3_walks())
    cap = macs_cap()
    for key, b in best.items():
        if b['macs'] > cap:
            r = shrink_call(b['recipe'], key[1], cap)
            if r is not b['recipe']:
                b.update(recipe=r, macs=recipe_macs(r), shrunk=True, recorded=b['recipe'])
    return best


def batch3_only_variants():
    """The (kind, variant) pairs of the batch-3 walks that no older table has a case for: representatives(),
    inference_representatives(), ragged_representatives()."""
    have = set(representatives()) | set(inference_representatives()) | set(ragged_representatives())
    return sorted(kv for kv in batch3_representatives() if kv not in have)


def replay_variant(recipe) -> str:
    """recipe_variant for all three kinds: the variant the call that run_recipe rebuilds from `recipe` selects, by a CPU dry run on empty
    tensors (a data gradient may be issued in several launches of one variant: the set must have one element)."""
    if recipe['kind'] == 'fwd':
        return recipe_variant(recipe)
    got = dry_variants(empty_call(recipe))
    assert len(set(got)) == 1, got
    return got[0]


def _empty_grad_call(recipe):
    from van_gan_amd import ops
    kind, L = recipe['kind'], recipe['layer']
    _, lay = make_layer_from(L, 'cpu')
    e = lambda *shp, dt=torch.bfloat16: torch.empty(*shp, dtype=dt)
    if kind == 'wgrad':
        sr = recipe['src']
        N, dims, c0, c1, sh = sr['N'], tuple(sr['dims']), sr['c0'], sr['c1'], sr['shift0']
        src = ops.Src(e(N, *[n >> sh for n in dims], c0, dt=torch.float32 if sr['f32'] else torch.bfloat16), (N,) + dims, c0,
                      e(N, *dims, c1) if c1 else None, c1, shift0=sh, f32=sr['f32'],
                      scale=e(N, c0 + c1, dt=torch.float32) if sr['affine'] else None, shift=e(N, c0 + c1, dt=torch.float32) if sr['affine'] else None,
                      act=sr['act'], noise=e(N, *[n + 2 * sr['noise_pad'] for n in dims], c0 + c1) if sr['noise'] else None, noise_pad=sr['noise_pad'])
        dy = e(N, *lay.out_dims, L['cout'], dt=torch.float32 if recipe['dy_f32'] else torch.bfloat16)
        return lambda: lay.wgrad(src, dy)
    else:
        N, Cc = recipe['N'], L['cin']
        dy = e(N, *lay.out_dims, L['cout'], dt=torch.float32 if recipe['dy_f32'] else torch.bfloat16)
        dp = e(N, *lay.buf_dims, Cc, dt=torch.float32 if recipe['out_f32'] else torch.bfloat16)
        bs, bdesc = recipe.get('bstat'), None
        if bs:
            dims_in = tuple(lay.in_dims)
            c0, sh = (bs['c_x0'], 1) if bs['cat'] else (Cc, 0)
            f = lambda *shp: e(*shp, dt=torch.float32)
            bdesc = ops.actnorm_desc(dp, bs['pad'], e(N, *[n >> sh for n in dims_in], c0), (N,) + dims_in, Cc, e(N, *dims_in, Cc), scale=f(N, Cc),
                                     shift=f(N, Cc), act=bs['act'], norm=True, gamma=f(Cc), mean=f(N, Cc), rstd=f(N, Cc),
                                     red=f(ops.STRIPES * N * Cc * 2 + 4), accumulate=False, x1=e(N, *dims_in, Cc - c0) if bs['cat'] else None,
                                     c_x0=c0 if bs['cat'] else 0, x0_shift=sh, dgamma=f(Cc), dbeta=f(Cc))
        return lambda: lay.dgrad(dy, N, dp, accumulate=recipe['accumulate'], bstat=bdesc)


def out_grid(recipe) -> Tuple[int, int, int]:
    """The grid a recorded call's kernel tiles: the convolution's output grid (forward; weight gradient: its reduction runs over it), the
    layer's input grid for the data gradient it writes (without the margin of a 'reflect' layer: n + 2 is never a power of two)."""
    L = recipe['layer']
    if recipe['kind'] == 'dgrad':
        return tuple(L['in_dims'])
    s, k = L['stride'], L['k']
    return tuple((n + 2 - k) // s + 1 if L['pad'] == 'reflect' else -(-n // s) for n in L['in_dims'])


# ----------------------------------------------------------------------------------------------------------------------
# replaying a recipe on the GPU against the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------
def bf(x, storage=torch.bfloat16):
    """x rounded to the library's 16-bit storage format (bf16; torch.float16 for libvangan_hip_h.so), in x's own dtype."""
    return x.to(storage).to(x.dtype)


def _ref_dtype(macs):
    return torch.float64 if macs < 3e9 else torch.float32      # float32 CPU accumulation error (~1e-6) << one bf16 rounding


# ---- where the replays' device tensors come from: plain torch allocations, or slots of a guarded arena (tests/guarded.py) ----
def dev_in(arena, host, dev, name=None, mutable=False):
    """An input operand on the device: a copy of `host` (None stays None); with an arena, a sealed slot of it (mutable: an operand the
    call accumulates into, not sealed)."""
    if host is None:
        return None
    return host.to(dev) if arena is None else arena.put(host, name=name, mutable=mutable)


def dev_out(arena, shape, dtype, dev, fill, name=None, must_write=False):
    """An output on the device, every element `fill`.  must_write, with an arena: the call has to store every element, so the slot starts
    as 0xFF bytes (a NaN in every float format) instead, and one it skips fails parity whatever the reference holds there."""
    if arena is None:
        return torch.full(tuple(shape), fill, dtype=dtype, device=dev)
    return arena.out(shape, dtype, None if must_write else fill, name=name)


def recipe_bytes(recipe) -> int:
    """Upper bound of the guarded-arena bytes a replay of `recipe` takes (run_recipe, run_fin, the stress loops).  On the layer's
    reflect-padded input grid: the source or the data gradient (at most 4 bytes an element), the noise or the statistics' forward
    tensors and their dx (2 + 2) -- 8 bytes, budgeted 12; on its output grid: the output or dY (4) and the residual (2), three outputs
    in a stress loop (2 each) -- 6 bytes, budgeted 12; the weight and gradient tables; 64 slots of up to 1 MiB for everything small."""
    import guarded
    L = recipe['layer']
    N = recipe_n(recipe)
    s, k = L['stride'], L['k']
    vin = math.prod(n + 2 for n in L['in_dims'])
    vout = math.prod((n + 2 - k) // s + 1 if L['pad'] == 'reflect' else -(-n // s) for n in L['in_dims'])
    big = [4 * N * vin * L['cin']] * 3 + [4 * N * vout * L['cout']] * 3 + [4 * k ** 3 * L['cin'] * L['cout'] + 4 * L['cout']] * 2
    return sum(guarded.slot_cost(b) for b in big) + 64 * guarded.slot_cost(1 << 20)


def guarded_for(recipe, dev):
    """A guarded arena big enough for one replay of `recipe`."""
    import guarded
    return guarded.GuardedArena(recipe_bytes(recipe), dev)


def make_layer_from(ctor, dev, seed=0, dtype=torch.bfloat16, arena=None):
    """arena: the parameter and gradient tables of the layer's store are slots of it (the weights sealed once they are set).  The packed
    operands stay what ConvLayer allocates: the pack kernels' outputs, read-only for every launch of these replays."""
    from van_gan_amd.nets import ParamStore
    from van_gan_amd.ops import ConvLayer
    k, cin, cout = ctor['k'], ctor['cin'], ctor['cout']
    specs = [('c.w', (k, k, k, cin, cout), 'x')] + ([('c.b', (cout,), 'x')] if ctor['bias'] else [])
    st = ParamStore(specs, dev)
    if arena is not None:               # before ConvLayer takes its views
        st.w = arena.out((st.total,), torch.float32, 0.0, name='weights')
        st.g = arena.out((st.total,), torch.float32, 0.0, name='weight gradients')
    g = torch.Generator().manual_seed(seed)
    st.param('c.w').copy_(torch.randn(k, k, k, cin, cout, generator=g) / math.sqrt(k ** 3 * cin))
    if ctor['bias']:
        st.param('c.b').copy_(torch.randn(cout, generator=g) * 0.1)
    if arena is not None:
        arena.seal(st.w)
    lay = ConvLayer(st, 'c', k, cin, cout, ctor['stride'], ctor['pad'], ctor['bias'], ctor['in_dims'],
                    need_dgrad=ctor['need_dgrad'], dtype=dtype)
    if ctor.get('c_up'):
        lay.enable_up(ctor['c_up'])
    return st, lay


def make_operand(sr, pad, dev, g, storage=torch.bfloat16, arena=None):
    """Random contents for a Src recipe -> (Src on dev, host tensors).  storage: the 16-bit type of the stored tensors.  arena: every
    device tensor of the Src is a sealed slot of it."""
    from van_gan_amd.ops import Src
    N, dims, c0, c1, sh = sr['N'], tuple(sr['dims']), sr['c0'], sr['c1'], sr['shift0']
    C_ = c0 + c1
    low = tuple(n >> sh for n in dims)
    x0 = torch.randn(N, *low, c0, generator=g)
    x0 = x0 if sr['f32'] else x0.to(storage)
    x1 = torch.randn(N, *dims, c1, generator=g).to(storage) if c1 else None
    scale = (torch.rand(N, C_, generator=g) + 0.5) if sr['affine'] else None
    shift = (torch.randn(N, C_, generator=g) * 0.3) if sr['affine'] else None
    noise = None
    if sr['noise']:
        npd = sr['noise_pad']
        noise = (torch.randn(N, *[n + 2 * npd for n in dims], C_, generator=g) * 0.1).to(storage)
    d = lambda t, name: dev_in(arena, t, dev, name)
    src = Src(d(x0, 'src0'), (N,) + dims, c0, d(x1, 'src1'), c1, shift0=sh, f32=sr['f32'], scale=d(scale, 'in_scale'), shift=d(shift, 'in_shift'),
              act=sr['act'], noise=d(noise, 'noise'), noise_pad=sr['noise_pad'])
    return src, dict(x0=x0, x1=x1, scale=scale, shift=shift, noise=noise)


def ref_operand(sr, host, pad, dt, storage=torch.bfloat16):
    """The convolution's input as the kernels stage it: act(IN-affine(virtual upsample + concat)) [-> reflection pad]
    + noise, rounded to bf16 (to `storage`).  NCDHW, on the padded grid for 'reflect'."""
    from oracle import vangan_oracle as O
    from van_gan_amd import ops
    x = host['x0'].to(dt)
    if sr['shift0']:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)       # UpSampling3D(2), nearest
    if host['x1'] is not None:
        x = torch.cat([x, host['x1'].to(dt)], dim=-1)                                      # concatenate([x_up, skip])
    N, C_ = x.shape[0], x.shape[-1]
    if host['scale'] is not None:
        x = x * host['scale'].to(dt).view(N, 1, 1, 1, C_) + host['shift'].to(dt).view(N, 1, 1, 1, C_)
    if sr['act'] == ops.ACT_RELU:
        x = F.relu(x)
    elif sr['act'] == ops.ACT_LRELU:
        x = F.leaky_relu(x, 0.2)
    a = O.to_ncdhw(x)
    if pad == 'reflect':
        a = O.reflect_pad1(a)
    if host['noise'] is not None:
        a = a + O.to_ncdhw(host['noise'].to(dt))
    return bf(a, storage)


def _f64_pair(got, ref):
    """Both in float64 on one device: where they already share one (a device-side reference of 600 M elements at 128^3, batch 3) the
    comparison stays there -- the same float64 arithmetic without two 5 GB copies to the host -- otherwise on the host."""
    if got.device == ref.device:
        return got.double(), ref.double()
    return got.double().cpu(), ref.double().cpu()


def close_bf16(got, ref, name='', rel=1.2e-2, floor=2e-3):
    got, ref = _f64_pair(got, ref)
    tol = rel * ref.abs() + floor * ref.abs().max() + 1e-30
    bad = (got - ref).abs() > tol
    assert not bad.any(), '%s: %d/%d outside tolerance, max err %.3e (max ref %.3e)' % (
        name, int(bad.sum()), bad.numel(), float((got - ref).abs().max()), float(ref.abs().max()))


def rel_l2(got, ref):
    got, ref = _f64_pair(got, ref)
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def dry_variants(fn):
    """Variant strings `fn()` would launch (fn issues ConvLayer calls)."""
    from van_gan_amd import ops
    with ops.DryRun() as dry:
        fn()
    return [v for (_, _, v) in dry.records]


# Bounds of a forward replay per storage type: close_bf16's (rel, floor) on a 16-bit output, rel-L2 of the statistics, rel-L2 of an f32
# output.  bf16: those of tests/test_gpu_ops.py.  fp16: kernel and reference read identical 16-bit-rounded operands, so what differs is
# the fp32 accumulation order and the ONE rounding of the stored output; fp16 carries 11 significand bits where bf16 carries 8, so every
# bound that comes from that rounding scales by 2^-3 (tests/test_variant_coverage.py checks on the CPU that a float32 convolution + .half()
# stays inside it against float64).  The f32-output bound has no 16-bit rounding in it and stays.
FWD_TOL = {torch.bfloat16: dict(rel=1.2e-2, floor=2e-3, sums=2e-2, f32=1e-4),
           torch.float16: dict(rel=1.5e-3, floor=2.5e-4, sums=2.5e-3, f32=1e-4)}


def run_recipe(recipe, expect_variant, dev, seed=1, precision='bf16', storage=torch.bfloat16, arena=None, after_launch=None):
    """Replay one recorded call on `dev` with random contents and compare with the oracle.  Tolerances as in
    tests/test_gpu_ops.py: identical bf16-rounded operands into the reference, so only fp32 accumulation order and the one
    rounding of the stored output differ.
    storage=torch.float16 (forward calls only, made inside ops.Fp16()): 16-bit tensors are IEEE half, the reference rounds with
    .half() where it rounds to bf16 otherwise, bounds FWD_TOL[torch.float16]; a single-channel fp32 residual (res_c1, stem.cb) is
    replayed as recorded.  Returns the measured errors of the replay.
    arena (tests/guarded.py): every device operand is a sealed slot of it and every output a slot that starts as 0xFF bytes (accumulators
    as zeros); after the parity assertions, which are the same either way, arena.verify(): every guard intact, every input unchanged.
    after_launch(call, result, reset): called once the launch has run and before anything is compared -- `result` the tensor the call
    writes, reset() puts what the call accumulates into back to its state before the launch, call() launches again (the parity
    assertions then see the last launch; tests/test_gpu_containment.py relaunches into a workspace it has not touched)."""
    from oracle import vangan_oracle as O
    L = recipe['layer']
    kind, pad, stride = recipe['kind'], L['pad'], L['stride']
    dt = _ref_dtype(recipe_macs(recipe))
    g = torch.Generator().manual_seed(seed)
    half = storage != torch.bfloat16
    assert storage in FWD_TOL and (not half or kind == 'fwd')
    st, lay = make_layer_from(L, dev, dtype=storage, arena=arena)
    lay.pack()
    w_ref = bf(st.param('c.w').cpu().to(dt), storage)
    b_ref = st.param('c.b').cpu().to(dt) if L['bias'] else None
    conv_pad = 'valid' if pad == 'reflect' else 'same'
    if kind in ('fwd', 'wgrad'):
        sr = recipe['src']
        N = sr['N']
        src, host = make_operand(sr, pad, dev, g, storage, arena)
        ap = ref_operand(sr, host, pad, dt, storage)
    if kind == 'fwd':
        tol = FWD_TOL[storage]
        odt = torch.float32 if recipe['out_f32'] else storage
        out = dev_out(arena, (N,) + tuple(lay.out_dims) + (L['cout'],), odt, dev, 0.0, 'out', must_write=True)
        sums = dev_out(arena, (8, N, L['cout'], 2), torch.float32, dev, 0.0, 'out_sums') if recipe['sums'] else None
        res = rs = rb = None
        c1 = half and bool(recipe.get('res_c1'))
        if recipe['res']:
            res = torch.randn(N, *lay.out_dims, 1, generator=g) if c1 else torch.randn(N, *lay.out_dims, L['cout'], generator=g).to(storage)
            rs, rb = torch.rand(N, L['cout'], generator=g) + 0.5, torch.randn(N, L['cout'], generator=g)
        res_d, rs_d, rb_d = dev_in(arena, res, dev, 'res'), dev_in(arena, rs, dev, 'res_scale'), dev_in(arena, rb, dev, 'res_shift')
        call = lambda: lay.forward(src, out, sums=sums, res=res_d, res_scale=rs_d, res_shift=rb_d,
                                   tanh=recipe['tanh'], **(dict(res_c1=True) if c1 else {}))
        assert dry_variants(call) == [expect_variant]
        call()
        torch.cuda.synchronize()
        if after_launch is not None:
            after_launch(call, out, lambda: None if sums is None else sums.zero_())
        y = O.to_ndhwc(O.conv3d(ap, w_ref, b_ref, stride, conv_pad))
        if res is not None:
            y = y + res.to(dt) * rs.to(dt).view(N, 1, 1, 1, -1) + rb.to(dt).view(N, 1, 1, 1, -1)
        if recipe['tanh']:
            y = torch.tanh(y)
        err = {}
        if recipe['out_f32']:
            err['f32'] = rel_l2(out, y)
            assert err['f32'] < tol['f32'], 'forward (f32 output) rel %.2e' % err['f32']
        else:
            err['out'] = float((out.double().cpu() - y.double()).abs().max() / y.double().abs().max())
            close_bf16(out, y, 'forward', rel=tol['rel'], floor=tol['floor'])
        if sums is not None:
            yq = bf(y, storage) if not recipe['out_f32'] else y
            ref_sums = torch.stack([yq.sum(dim=(1, 2, 3)), (yq ** 2).sum(dim=(1, 2, 3))], dim=-1)
            err['sums'] = rel_l2(sums.sum(0), ref_sums)
            assert err['sums'] < tol['sums'], 'IN statistics rel %.2e' % err['sums']
        if arena is not None:
            arena.verify()
        return err
    odims = lay.out_dims
    dy = torch.randn(recipe['src']['N'] if kind == 'wgrad' else recipe['N'], *odims, L['cout'], generator=g)
    dys = dy if recipe['dy_f32'] else dy.to(torch.bfloat16)
    dy_ref = O.to_ncdhw(bf(dys.to(dt)))                 # the kernels round dY to bf16 when they stage it
    dy_d = dev_in(arena, dys, dev, 'dy')
    if kind == 'wgrad':
        call = lambda: lay.wgrad(src, dy_d)
        assert dry_variants(call) == [expect_variant]
        st.g.zero_()
        call()
        torch.cuda.synchronize()
        if after_launch is not None:
            after_launch(call, st.g, lambda: st.g.zero_())
        w = w_ref.clone().requires_grad_(True)
        (O.conv3d(ap, w, None, stride, conv_pad) * dy_ref).sum().backward()
        err = dict(w=rel_l2(st.grad('c.w'), w.grad))
        assert err['w'] < 2e-3, 'weight gradient rel %.2e' % err['w']
        if L['bias']:
            err['b'] = rel_l2(st.grad('c.b'), dy_ref.sum(dim=(0, 2, 3, 4)))
            assert err['b'] < 2e-3, 'bias gradient rel %.2e' % err['b']
        if arena is not None:
            arena.verify()
        return err
    # data gradient: on the reflect-PADDED grid for 'reflect' convs (the fold is a separate kernel), plain grid for 'same'
    N = recipe['N']
    odt = torch.float32 if recipe['out_f32'] else torch.bfloat16
    prior = None
    if recipe['accumulate']:
        prior = torch.randn(N, *lay.buf_dims, L['cin'], generator=g).to(odt)
        dp = prior.to(dev).clone() if arena is None else arena.put(prior, name='dx (accumulated into)', mutable=True)
    else:
        dp = dev_out(arena, (N,) + tuple(lay.buf_dims) + (L['cin'],), odt, dev, 7.0, 'dx', must_write=True)   # must be overwritten everywhere
    bs = recipe.get('bstat')
    bdesc = None
    if bs:
        # the IN backward that consumes this data gradient: its statistics ride on the launch (ConvLayer.dgrad(bstat=...))
        from van_gan_amd import ops
        Cc, dims_in = L['cin'], tuple(lay.in_dims)
        c0 = bs['c_x0'] if bs['cat'] else Cc
        sh = 1 if bs['cat'] else 0
        bx0 = torch.randn(N, *[n >> sh for n in dims_in], c0, generator=g).to(torch.bfloat16)
        bx1 = torch.randn(N, *dims_in, Cc - c0, generator=g).to(torch.bfloat16) if bs['cat'] else None
        bsc, bsf = torch.rand(N, Cc, generator=g) + 0.5, torch.randn(N, Cc, generator=g) * 0.3
        bmu, brs = torch.randn(N, Cc, generator=g) * 0.2, torch.rand(N, Cc, generator=g) + 0.5
        red = dev_out(arena, (ops.STRIPES * N * Cc * 2 + 4,), torch.float32, dev, 0.0, 'red')
        dgam, dbet = dev_out(arena, (Cc,), torch.float32, dev, 0.0, 'dgamma'), dev_out(arena, (Cc,), torch.float32, dev, 0.0, 'dbeta')
        dxo = dev_out(arena, (N,) + dims_in + (Cc,), torch.bfloat16, dev, 0.0, 'IN-backward dx', must_write=True)
        tod = lambda t, name: dev_in(arena, t, dev, 'IN-backward ' + name)
        bdesc = ops.actnorm_desc(dp, bs['pad'], tod(bx0, 'x0'), (N,) + dims_in, Cc, dxo, scale=tod(bsc, 'scale'), shift=tod(bsf, 'shift'), act=bs['act'], norm=True,
                                 gamma=tod(torch.ones(Cc), 'gamma'), mean=tod(bmu, 'mean'), rstd=tod(brs, 'rstd'), red=red, accumulate=False, x1=tod(bx1, 'x1'),
                                 c_x0=c0 if bs['cat'] else 0, x0_shift=sh, dgamma=dgam, dbeta=dbet)
    done = []
    call = lambda: done.append(lay.dgrad(dy_d, N, dp, accumulate=recipe['accumulate'], bstat=bdesc))
    got_variants = dry_variants(call)
    assert expect_variant in got_variants and len(set(got_variants)) == 1, (got_variants, expect_variant)
    call()
    torch.cuda.synchronize()
    if after_launch is not None:
        after_launch(call, dp, lambda: (None if prior is None else dp.copy_(prior), None if not bs else red.zero_()))
    if bs:
        assert done[-1] is True
        # reference statistics from the data gradient the kernel stored: transpose of the reflection pad, dn = g * act'(pre)
        gp = O.to_ncdhw(dp.double().cpu())
        a0 = torch.zeros(N, L['cin'], *lay.in_dims, dtype=torch.float64, requires_grad=True)
        ((O.reflect_pad1(a0) if bs['pad'] else a0) * gp).sum().backward()
        gf = O.to_ndhwc(a0.grad)
        xf = bx0.double()
        if bs['cat']:
            xf = torch.cat([xf.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3), bx1.double()], dim=-1)
        v = lambda t: t.double().view(N, 1, 1, 1, -1)
        pre = xf * v(bsc) + v(bsf)
        slope = 0.0 if bs['act'] == ops.ACT_RELU else (0.2 if bs['act'] == ops.ACT_LRELU else 1.0)
        dn = gf * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))
        xh = (xf - v(bmu)) * v(brs)
        ref_red = torch.stack([dn.sum(dim=(1, 2, 3)), (dn * xh).sum(dim=(1, 2, 3))], dim=-1)
        got_red = red[:ops.STRIPES * N * L['cin'] * 2].view(ops.STRIPES, N, L['cin'], 2).sum(0)       # striped: the apply pass adds them up
        assert rel_l2(got_red, ref_red) < 2e-3, 'fused IN-backward statistics rel %.2e' % rel_l2(got_red, ref_red)
        ops.actnorm_run(bdesc, stats_done=True)                                                     # apply: dx and the gamma / beta gradients
        torch.cuda.synchronize()
        assert rel_l2(dbet, ref_red[..., 0].sum(0)) < 2e-3 and rel_l2(dgam, ref_red[..., 1].sum(0)) < 2e-3
        ref_dx = v(brs) * (dn - ref_red[..., 0].view(N, 1, 1, 1, -1) / dn[0, ..., 0].numel() - xh * ref_red[..., 1].view(N, 1, 1, 1, -1) / dn[0, ..., 0].numel())
        assert rel_l2(dxo, ref_dx) < 1e-2, 'IN backward after fused statistics rel %.2e' % rel_l2(dxo, ref_dx)
    xin = torch.zeros(N, L['cin'], *lay.buf_dims, dtype=dt, requires_grad=True)
    (O.conv3d(xin, w_ref, None, stride, conv_pad) * dy_ref).sum().backward()
    ref = O.to_ndhwc(xin.grad)
    if prior is not None:
        ref = ref + prior.to(dt)
    close_bf16(dp, ref, 'data gradient', rel=2.5e-2, floor=6e-3)
    if arena is not None:
        arena.verify()
    return dict(dx=float((dp.double().cpu() - ref.double()).abs().max() / ref.double().abs().max()))


def stress_recipe(recipe, expect_variant, dev, launches=200, seed=3, arena=None):
    """K-split exchange under load: the recorded call `launches` times back to back, alternating between two streams (each with its
    own output buffer; the library's per-stream scratch -- partial tiles + arrival counters -- is reused by every launch of a
    stream), every output compared BITWISE with the first launch's.  The slices' partial tiles are added in slice order, so any
    difference is a partial tile read before it was complete, or a counter that did not return to zero.
    arena (tests/guarded.py): operands and the three outputs are slots of it; guards and inputs are verified ONCE, after the loop (a
    check per launch would put a host sync between the launches the loop is there to overlap)."""
    L = recipe['layer']
    kind = recipe['kind']
    g = torch.Generator().manual_seed(seed)
    st, lay = make_layer_from(L, dev, arena=arena)
    lay.pack()
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    if kind == 'fwd':
        sr = recipe['src']
        src, _ = make_operand(sr, L['pad'], dev, g, arena=arena)
        odt = torch.float32 if recipe['out_f32'] else torch.bfloat16
        outs = [dev_out(arena, (sr['N'],) + tuple(lay.out_dims) + (L['cout'],), odt, dev, 0.0, 'out %d' % i, must_write=True) for i in range(3)]
        call = lambda o: lay.forward(src, o, tanh=recipe['tanh'])
    else:
        assert kind == 'dgrad' and not recipe['accumulate'] and not recipe.get('bstat')
        N = recipe['N']
        dy = torch.randn(N, *lay.out_dims, L['cout'], generator=g)
        dys = dev_in(arena, dy if recipe['dy_f32'] else dy.to(torch.bfloat16), dev, 'dy')
        odt = torch.float32 if recipe['out_f32'] else torch.bfloat16
        outs = [dev_out(arena, (N,) + tuple(lay.buf_dims) + (L['cin'],), odt, dev, 0.0, 'dx %d' % i, must_write=True) for i in range(3)]
        call = lambda o: lay.dgrad(dys, N, o, accumulate=False)
    got = dry_variants(lambda: call(outs[2]))
    assert got == [expect_variant], (got, expect_variant)
    call(outs[2])
    torch.cuda.synchronize()
    ref = outs[2].clone()
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    bad = 0
    for i in range(launches):
        with torch.cuda.stream(streams[i & 1]):
            outs[i & 1].fill_(7.0)
            call(outs[i & 1])
            bad = bad + (outs[i & 1] != ref).sum()             # device-side count: no host sync between the launches
    torch.cuda.synchronize()
    bad = int(bad)
    assert bad == 0, '%d elements differ from the first launch over %d launches on two streams' % (bad, launches)
    if arena is not None:
        arena.verify()
