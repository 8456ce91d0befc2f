"""CPU: the spectral-normalisation feature's host side -- the entry points are declared and exported by both libraries (which still
import no allocating / synchronising HIP call), the SN parameter specs, the reference-shaped keyword, the float64 restatement the GPU
tests compare against (checked against numpy's SVD), and the SN discriminator's schedule walked in dry-run mode: five forward
convolutions, no InstanceNorm statistics / finalisation, activation-only backward."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sn_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_and_exported():
    from van_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    for name in ('vg_spectral_norm', 'vg_spectral_norm_scratch_bytes', 'vg_spectral_norm_blocks'):
        assert re.search(r'^(?:int|int64_t)\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name) and name in _lib.EXPORTS
    banned = re.compile(r'\b(hipMalloc\w*|hipFree\w*|hipHostMalloc|hipMallocAsync|hipDeviceSynchronize|hipStreamSynchronize|hipMemcpy)\b')
    for lib in (build.LIB, build.LIB_H):
        out = subprocess.run(['nm', '-D', '--undefined-only', lib], stdout=subprocess.PIPE, check=True).stdout.decode()
        assert 'hipLaunchKernel' in out or '__hipPushCallConfiguration' in out
        assert not banned.search(out), banned.findall(out)
    import ctypes as C
    assert _lib.lib.vg_abi_sizeof(4) == C.sizeof(_lib.SnItem) == 40


def test_shape_and_argument_validation_without_gpu():
    from van_gan_amd._lib import lib
    assert [lib.vg_spectral_norm_blocks(K, C_) for K, C_ in R.SHAPES] == [1, 8, 32, 128]
    assert lib.vg_spectral_norm_blocks(64, 96) == -1 and lib.vg_spectral_norm_blocks(3, 64) == -1 and lib.vg_spectral_norm_blocks(0, 64) == -1
    assert lib.vg_spectral_norm_scratch_bytes(169) == 169 * 516 * 4 and lib.vg_spectral_norm_scratch_bytes(0) == -1
    # rejected before anything is launched: null table / scratch, too many projections, scratch too small, misaligned scratch
    assert lib.vg_spectral_norm(None, 4, 169, 2, 1 << 20, 1 << 30, None) == -1
    assert lib.vg_spectral_norm(1 << 20, 4, 169, 2, None, 1 << 30, None) == -1
    assert lib.vg_spectral_norm(1 << 20, 4, 169, 5, 1 << 20, 1 << 30, None) == -1
    assert lib.vg_spectral_norm(1 << 20, 4, 169, 2, 1 << 20, 169 * 516 * 4 - 1, None) == -1
    assert lib.vg_spectral_norm(1 << 20, 4, 169, 2, (1 << 20) + 4, 1 << 30, None) == -1


def test_param_specs():
    from van_gan_amd.nets import ParamStore, disc_param_specs, init_reference
    from oracle import vangan_oracle as O
    assert [(n, tuple(s)) for n, s, _ in disc_param_specs()] == [(n, tuple(s)) for n, s, _ in O.disc_param_specs()]
    assert disc_param_specs(spectral_norm=False) == disc_param_specs() and disc_param_specs(64) == disc_param_specs(64, False)
    sp = disc_param_specs(spectral_norm=True)
    assert not [n for n, _, _ in sp if '.in.' in n]
    assert [(n, s) for n, s, i in sp if i == 'sn_u'] == [('conv0.sn_u', (1, 64)), ('down0.sn_u', (1, 128)), ('down1.sn_u', (1, 256)),
                                                        ('down2.sn_u', (1, 512))]
    st = ParamStore(sp, 'cpu')
    assert st.total == 11029953 - 1920 and st.state.numel() == 960 and st.T == 7 and int(st.seg_off[-1]) == st.total
    assert st.w.numel() == st.g.numel() == st.m.numel() == st.v.numel() == st.total          # sn_u: no gradient, no Adam slots
    init_reference(st, 5)
    P = st.export()
    u = P['down2.sn_u']
    assert u.shape == (1, 512) and float(u.abs().max()) <= 0.04 + 1e-7 and 0.012 < float(u.std()) < 0.02       # TruncatedNormal(0.02), +-2 sigma
    assert set(st.export(st.g)) == {n for n, _, i in sp if i != 'sn_u'}
    st2 = ParamStore(sp, 'cpu'); st2.load(P)
    assert torch.equal(st.w, st2.w) and torch.equal(st.state, st2.state)
    with pytest.raises(KeyError):
        st2.load({k: v for k, v in P.items() if not k.endswith('sn_u')})
    # the wasserstein head combines with it; the default store has no state
    assert ParamStore(disc_param_specs(64, True), 'cpu').total == st.total + 65 and ParamStore(disc_param_specs(), 'cpu').state.numel() == 0


def test_reference_keyword_maps_to_engine():
    from van_gan_amd import compat
    a = argparse.Namespace(N_DEVICES=1, INPUT_IMG_SIZE=(1, 64, 64, 64, 1), CHANNELS=1, GLOBAL_BATCH_SIZE=1, DIMENSIONS=3,
                           SUBVOL_PATCH_SIZE=(32, 32, 32), train_steps=5, BATCH_SIZE=1, output_dir=None)
    kw = compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', use_SN=True)
    assert kw['spectral_norm'] is True
    assert 'spectral_norm' not in compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet')
    kw = compat.engine_kwargs_from_args(a, gen_i2s='resUnet', gen_s2i='resUnet', wasserstein=True, use_SN=True)
    assert kw['spectral_norm'] and kw['wasserstein'] and kw['clipnorm'] == 0.0
    seen = {}

    class Eng:
        layer_noise, lr, current_epoch, checkpoint_loaded = 0.1, 2e-4, 0, False

        def __init__(self, **k):
            seen.update(k)
            self.spectral_norm = k.get('spectral_norm', False)
            self.gen_IS = self.gen_SI = self.disc_I = self.disc_S = object()
    g = compat.VanGan(a, None, gen_i2s='resUnet', gen_s2i='resUnet', use_SN=True, engine_factory=Eng)
    assert seen['spectral_norm'] is True and g.use_SN
    names = [l.name for l in g.disc_S.layers]
    assert 'instance_normalization' not in names and names.count('spectral_normalization') == 1
    noise = [l for l in g.disc_S.layers if isinstance(l, compat.GaussianNoiseShim)]
    assert len(noise) == 5                      # GanMonitor.updateDiscriminatorNoise still finds every GaussianNoise layer
    noise[0].stddev = 0.05
    assert g.eng.layer_noise == 0.05


def test_restatement_converges_to_the_top_singular_value():
    """The power iteration's estimate errs by ~(s2 / s1)^(2 n) after n projections.  An i.i.d. he_normal [4096, 128] matrix has
    s2 / s1 ~ 0.99 (Marchenko-Pastur edge): 200 projections leave ~1e-5 there, whatever the formulae.  The restatement is therefore
    checked on a seeded matrix with a spectral gap -- he_normal noise plus a rank-one term, s2 / s1 ~ 0.7 -- where 200 projections
    of a CORRECT power iteration are far below the 1e-6 asked for, and a wrong one is not."""
    W, u = R.he_normal(4096, 128, 1)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(4096, 1, generator=g), torch.randn(1, 128, generator=g)
    W = W + 2.0 * (a / a.norm()) @ (b / b.norm())
    W, u = W.double().numpy(), u.double().numpy()
    sv = np.linalg.svd(W, compute_uv=False)
    top = float(sv[0])
    assert sv[1] / sv[0] < 0.8
    prod = 1.0
    for _ in range(200):
        W, u, s = R.project(W, u)
        est = s * prod
        prod *= s
    assert abs(est - top) <= 1e-6 * top, (est, top)
    assert abs(float(np.linalg.svd(W, compute_uv=False)[0]) - 1.0) <= 1e-6
    assert abs(float((u * u).sum()) - 1.0) < 1e-12
    # the first two projections at the four true shapes: the ranges the feature was specified with
    for i, (K, C_) in enumerate(R.SHAPES):
        W, u = R.he_normal(K, C_, 10 + i)
        W1, u1, s1 = R.project(W.numpy(), u.numpy())
        _, _, s2 = R.project(W1, u1)
        assert 1.4 < s1 < 2.3 and 1.0 < s2 < 1.25, (K, C_, s1, s2)
    Z, uz, sz = R.project(np.zeros((64, 64)), u[:, :64] if u.shape[1] >= 64 else u)
    assert sz == 0.0 and not Z.any()


def _walk(dims, B, dtype):
    from van_gan_amd import ops
    from van_gan_amd.nets import ParamStore, PatchGAN, disc_param_specs
    S = dims[0] * dims[1] * dims[2]
    D = PatchGAN(ParamStore(disc_param_specs(spectral_norm=True), 'cpu'), dims, dtype, spectral_norm=True)
    ar = ops.Arena(int(B * S * 5200 * 2) + (512 << 20), 'cpu')
    ld = tuple(n // 8 for n in dims)
    with ops.DryRun() as dry:
        x2 = ar.alloc((2 * B,) + dims + (1,), torch.float32)
        lg = ar.alloc((2 * B,) + ld + (1,), torch.float32)
        noise = {k: torch.empty(shp, dtype=torch.bfloat16) for k, shp in D.noise_shapes(2 * B).items()}
        drop = {k: torch.empty(2 * B, c) for k, c in (('down0', 128), ('down1', 256), ('down2', 512))}
        ctx = D.forward(ar, x2, lg, noise, drop)
        nf = len(dry.records)
        D.backward_both(ar, ctx, ar.alloc((3 * B,) + ld + (1,), torch.float32), B, ar.alloc((B,) + dims + (1,), torch.float32))
    return dry, nf


@pytest.mark.parametrize('dims', [(32, 32, 32), (128, 128, 128)])
def test_dry_run_walk_of_the_sn_discriminator(dims):
    for dtype in (torch.bfloat16, torch.float32):
        dry, nf = _walk(dims, 1, dtype)
        fwd = [r for r in dry.records[:nf]]
        assert [(k, n) for k, n, _ in fwd] == [('fwd', n) for n in ('conv0', 'down0', 'down1', 'down2', 'out')]
        names = [n for n, _ in dry.calls]
        assert 'vg_in_finalize' not in names and not [n for n in names if 'stats' in n]
        anb = [dict(r) for n, r in dry.calls if n == 'vg_actnorm_bwd' and dict(r)['C'] > 1]      # (C == 1: the fold of conv0's input gradient)
        assert [r['C'] for r in anb] == [512, 256, 128, 64]
        assert all(r['norm'] == 0 and r['act'] == 2 and r['has_mult'] == (r['C'] > 64) and not r['has_dgamma'] for r in anb)
        assert all(r['alias_n0'] == 2 and r['alias_shift'] == 1 for r in anb)
        kinds = [k for k, _, _ in dry.records[nf:]]
        assert kinds.count('wgrad') == 5 and kinds.count('dgrad') == 5
        # the variants the GPU tests of tests/test_gpu_specnorm.py run at 32^3 (and the flagship's at 128^3), for the record
        print(dims, dtype, sorted({(k, v.split('|')[0]) for k, _, v in dry.records}))
    with pytest.raises(ValueError):
        from van_gan_amd.nets import ParamStore, PatchGAN, disc_param_specs
        PatchGAN(ParamStore(disc_param_specs(), 'cpu'), dims, torch.bfloat16, spectral_norm=True)
