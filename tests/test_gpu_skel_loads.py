"""The clDice skeleton kernels request their global operands on CLAMPED addresses, all of them before the first wait (the LDS tile in
two phases, the per-voxel operands of the column walk in front of the tile's barrier), and select the fill value afterwards.  What can
go wrong with that is a clamp: one that leaves the sample's own volume (the neighbouring sample's voxels instead of the fill value), a
predicate that no longer matches its element, a store or an atomic that lost its bounds check.  So: volumes smaller than one tile,
ragged tiles with two samples adjacent in memory, exactly one tile (every halo face outside), full interior tiles at the workload's 15
iterations; continuous data, and binary data full of ties for the ragged shape.

Bounds: the erosion chain is a minimum (exact) -> bit equality with the CPU restatement below; the skeletons of the different launch
schedules run the same arithmetic in the same order -> bit equality; against the float64 oracle the bounds are those of
test_gpu_ops.py (final skeleton rel_l2 < 1e-6, gradient rel_l2 < 1e-3, filed-codes path within 2e-5 * max(|g|, 1))."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import vangan_oracle as O  # noqa: E402

CASES = {
    'smaller_than_a_tile': (1, 5, 3, 9, 3, False),
    'ragged_two_samples': (2, 11, 13, 37, 6, False),
    'ragged_two_samples_ties': (2, 11, 13, 37, 6, True),
    'ragged_three_samples': (3, 11, 13, 37, 6, False),      # a clamp that leaves the middle sample reads a neighbour on either side
    'exactly_one_tile': (1, 8, 8, 32, 3, False),
    'interior_tiles': (1, 16, 16, 64, 15, False),
}
_FOOTPRINT = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if abs(a) + abs(b) + abs(c) <= 2]     # 19 voxels


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def erode_cpu(x):
    """x: [B, D, H, W] float32.  Minimum over the 19-voxel footprint (3 x 3 x 3 minus its corners), +inf outside the volume."""
    _, D, H, W = x.shape
    pad = F.pad(x, (1, 1, 1, 1, 1, 1), value=float('inf'))
    out = torch.full_like(x, float('inf'))
    for (a, b, c) in _FOOTPRINT:
        out = torch.minimum(out, pad[:, 1 + a:1 + a + D, 1 + b:1 + b + H, 1 + c:1 + c + W])
    return out


def _forward(p, dims, it, aux=None, fill=(0.0, 0.0)):
    from van_gan_amd import ops
    vol = dims + (1,)
    imgs = torch.full((it + 2,) + vol, fill[0], device=p.device)
    skels = torch.full((it + 1,) + vol, fill[1], device=p.device)
    ops.soft_skel_fwd(p, dims, it, imgs, skels, aux)
    torch.cuda.synchronize()
    return imgs, skels


@functools.lru_cache(maxsize=None)
def run(name):
    """Everything one case needs from the GPU and from the oracle, computed once and read by all tests."""
    from van_gan_amd import ops
    from van_gan_amd._lib import lib
    B, D, H, W, it, binary = CASES[name]
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(41)
    p = torch.rand(B, D, H, W, 1, generator=g)
    if binary:
        p = (F.avg_pool3d(p.permute(0, 4, 1, 2, 3), 3, 1, 1) > 0.5).float().permute(0, 2, 3, 4, 1).contiguous()
    gskel = torch.randn(B, D, H, W, 1, generator=g)
    dims, vol = (B, D, H, W), (B, D, H, W, 1)
    pd = p.to(dev)
    r = {'p': p, 'it': it}
    fwd = {}
    try:
        for key, knob, val in (('default', None, 0), ('per_step', b'SKEL_CHAIN', 0), ('multi4', b'SKEL_MULTI', 4), ('multi2', b'SKEL_MULTI', 2),
                               ('multi1', b'SKEL_MULTI', 1)):
            if knob:
                lib.vg_set_tuning(knob, val, 0)
            imgs, skels = _forward(pd, dims, it, fill=(-5.0, 3.0))              # every element has to be written
            if knob:
                lib.vg_set_tuning(knob, 0, 1)
            fwd[key] = (imgs.cpu(), skels.cpu())
    finally:
        lib.vg_set_tuning(b'SKEL_CHAIN', 0, 1)
        lib.vg_set_tuning(b'SKEL_MULTI', 0, 1)
    r['fwd'] = fwd
    # backward: the scan path (no aux) and the filed-codes path, both accumulating into a gradient pre-filled with 0.25
    imgs, skels = _forward(pd, dims, it)
    aux = torch.zeros(ops.skel_aux_bytes(dims, it), dtype=torch.uint8, device=dev)
    imgs_a, skels_a = _forward(pd, dims, it, aux)
    r['fwd_aux'] = (imgs_a.cpu(), skels_a.cpu())
    gs = gskel.to(dev)
    gp = torch.full(vol, 0.25, device=dev)
    work = torch.zeros((3,) + vol, device=dev)
    ops.soft_skel_bwd(imgs, skels, gs, dims, it, work, gp)
    gp_a = torch.full(vol, 0.25, device=dev)
    work_a = torch.full((4,) + vol, float('nan'), device=dev)
    ops.soft_skel_bwd(imgs_a, skels_a, gs, dims, it, work_a, gp_a, aux)
    torch.cuda.synchronize()
    r['grad_scan'], r['grad_codes'], r['work'] = gp.cpu() - 0.25, gp_a.cpu() - 0.25, work.cpu()
    # float64 oracle: final skeleton and the gradient of <gskel, soft_skel(p)>
    pr = p.double().requires_grad_(True)
    sk = O.soft_skel(pr[..., 0], it)
    (sk * gskel.double()[..., 0]).sum().backward()
    r['skel_ref'], r['grad_ref'] = sk.detach(), pr.grad
    return r


@pytest.mark.parametrize('name', list(CASES))
def test_erosion_chain_is_bitwise_the_cpu_minimum(name):
    r = run(name)
    imgs = r['fwd']['default'][0][..., 0]
    assert torch.equal(imgs[0], r['p'][..., 0])
    for j in range(r['it'] + 1):
        assert torch.equal(imgs[j + 1], erode_cpu(imgs[j])), (name, 'img_%d' % (j + 1))
    for key in ('per_step', 'multi4', 'multi2', 'multi1'):
        assert torch.equal(r['fwd'][key][0], r['fwd']['default'][0]), (name, key)
    assert torch.equal(r['fwd_aux'][0], r['fwd']['default'][0]), (name, 'aux')


@pytest.mark.parametrize('name', list(CASES))
def test_skeletons_are_bitwise_the_same_for_every_launch_schedule(name):
    r = run(name)
    ref = r['fwd']['default'][1]
    for key in ('per_step', 'multi4', 'multi2', 'multi1'):
        assert torch.equal(r['fwd'][key][1], ref), (name, key)
    assert torch.equal(r['fwd_aux'][1], ref), (name, 'aux')
    err = rel_l2(ref[r['it']][..., 0], r['skel_ref'])
    print(name, 'final skeleton rel_l2 vs float64 oracle: %.3e' % err)
    assert err < 1e-6, (name, err)


@pytest.mark.parametrize('name', list(CASES))
def test_scan_backward_matches_the_oracle_and_the_filed_codes(name):
    r = run(name)
    g, ga, ref = r['grad_scan'], r['grad_codes'], r['grad_ref']
    assert bool(torch.isfinite(g).all())
    err = rel_l2(g, ref)
    diff, top = float((g - ga).abs().max()), float(ga.abs().max())
    print(name, 'gradient rel_l2 vs float64 autograd: %.3e   max |scan - codes| %.3e (max |g| %.3e)' % (err, diff, top))
    assert err < 1e-3, (name, err)
    assert diff <= 2e-5 * max(top, 1.0), (name, diff, top)


@pytest.mark.parametrize('name', list(CASES))
def test_scan_backward_leaves_its_consumed_buffer_zero(name):
    """erode_bwd_kernel zeroes every element of d img_{j+1} that it consumed (the buffer is the next step's accumulator, and nothing else
    clears it).  The two buffers swap roles once per step, so after the last step the consumed one is work[1] for an even number of
    iterations and work[2] for an odd one -- it must hold zeros only; the other one holds d img_0."""
    r = run(name)
    consumed, kept = r['work'][1 + r['it'] % 2], r['work'][1 + (r['it'] + 1) % 2]
    assert bool((consumed == 0).all()), (name, int((consumed != 0).sum()))
    assert torch.equal(kept + 0.25 - 0.25, r['grad_scan']), name


@pytest.mark.parametrize('dims', [(2, 5, 3, 9), (1, 1, 1, 7), (2, 8, 8, 32), (3, 5, 3, 9)])
def test_ssim_window_loads_stay_inside_their_sample(dims):
    """ssim_fwd_kernel / ssim_bwd_kernel request their 27-voxel windows the same way (clamped, all before the first wait).  Two samples
    adjacent in memory, volumes thinner than the window; value and gradient against the float64 oracle with the bounds of
    test_losses_vs_oracle (1e-3 relative)."""
    from van_gan_amd import ops
    dev = torch.device('cuda:0')
    B, D, H, W = dims
    g = torch.Generator().manual_seed(43)
    p = torch.rand(B, D, H, W, 1, generator=g); tt = torch.rand(B, D, H, W, 1, generator=g)
    pr = p.double().requires_grad_(True)
    ls = O.ssim_loss_3d(tt.double(), pr).sum()
    ls.backward()
    acc = torch.zeros(1, device=dev)
    part = torch.zeros(3, B, D, H, W, 1, device=dev)
    gp = torch.full((B, D, H, W, 1), 0.25, device=dev)                  # accumulated into
    gp2 = torch.full((B, D, H, W, 1), float('nan'), device=dev)         # overwritten
    ops.ssim_fwd(tt.to(dev), p.to(dev), dims, acc, part)
    ops.ssim_bwd(tt.to(dev), p.to(dev), part, dims, 1.0, gp, accumulate=True)
    ops.ssim_bwd(tt.to(dev), p.to(dev), part, dims, 1.0, gp2)
    torch.cuda.synchronize()
    assert abs(float(acc[0]) - float(ls.detach())) < 1e-3 * abs(float(ls.detach()))
    assert rel_l2(gp - 0.25, pr.grad) < 1e-3
    assert rel_l2(gp2, pr.grad) < 1e-3
