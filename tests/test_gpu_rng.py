"""The device RNG (vg_randn_bf16, vg_dropout_mask: randn_bf16_kernel and dropout_mask_kernel, Philox-4x32-10 into Box-Muller) against
its numpy restatement (tests/rng_restate.py, checked by itself in tests/test_rng_host.py): masks bit for bit, noise element by element, the moments and the
independence of the grid-stride case, the variants that read counter and sigma from device memory, and the engine's counter accounting.
Sizes are the smallest that reach each path: below one quad, the n % 4 tails, more quads than the largest grid has threads (the
grid-stride loop), and offsets whose low word carries into the high word inside the launch."""
import functools

import numpy as np
import pytest
import torch

import rng_restate as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64
VG_EINVAL = -1

# Largest (|got - ref| - 2^-8 |ref|) / std over all noise cases of this module, measured on an MI355X against the float64 restatement:
# 9.55e-7, in the grid-stride case at an element next to zero (got -0.000006 at std 0.1), where the absolute error of __sinf / __cosf
# shows; everywhere else the one bf16 rounding covers the whole difference.  That is what __logf, __cosf, __sinf and the fp32
# arithmetic around them cost; A is twice the measurement.  The condition, independent of the measurement: A <= 2^-6 (a wrong word
# pairing or exchanged sin / cos is an O(1) error).
A_MEASURED = 9.55e-7
A = 2 * A_MEASURED
assert A <= R.A_CAP

HI = 0x9E3779B9 << 32            # seeds with a non-zero high word: key word 1 is live


def _noise(n, std, seed, offset, launch=None):
    """bf16 noise of a launch into a guard-padded buffer -> (float64 numpy [n], guard cells intact?)."""
    from van_gan_amd import ops
    buf = torch.full((n + GUARD,), 9.0, dtype=torch.bfloat16, device=DEV)
    (launch or (lambda out: ops.randn_bf16(out, std, seed, offset)))(buf[:n])
    torch.cuda.synchronize()
    return buf[:n].double().cpu().numpy(), bool((buf[n:] == 9.0).all())


@functools.lru_cache(maxsize=None)
def _big_noise():
    """The grid-stride case, once for the tests that read it: std 0.1 (the engine's default sigma), more than four times 8192 x 256
    elements, counters across 2^32, n % 4 = 3."""
    c = R.BIG_NOISE
    got, guard_ok = _noise(c['n'], 0.1, c['seed'], c['offset'])
    ref = R.randn(c['n'], 0.1, c['seed'], c['offset'])
    got.setflags(write=False); ref.setflags(write=False)
    return got, ref, guard_ok


def _check_noise(got, ref, std, what):
    ex = R.noise_excess(got, ref, std)
    i = int(ex.argmax())
    print('   %-44s max (|got - ref| - 2^-8 |ref|) / std = %.3e  (at %d: got %.6f ref %.6f)' % (what, ex[i], i, got[i], ref[i]))
    assert ex[i] <= A, (what, i, got[i], ref[i])


SMALL_NOISE = [(n, std, HI + 17 * n, off) for n in (1, 2, 3, 5, 1027) for std, off in ((1.0, 2 ** 32 - 1), (0.1, 3 * 2 ** 40 + n))]


@pytest.mark.parametrize('n,std,seed,offset', SMALL_NOISE)
def test_noise_matches_restatement(n, std, seed, offset):
    got, guard_ok = _noise(n, std, seed, offset)
    assert guard_ok, 'wrote past n'
    _check_noise(got, R.randn(n, std, seed, offset), std, 'n %d std %g offset %#x' % (n, std, offset))


def test_noise_grid_stride_carry_and_tail():
    got, ref, guard_ok = _big_noise()
    assert guard_ok, 'wrote past n'
    assert R.BIG_NOISE['n'] % 4 == 3 and (R.BIG_NOISE['n'] + 3) // 4 > R.GRID_THREADS
    assert R.BIG_NOISE['offset'] < 2 ** 32 < R.BIG_NOISE['offset'] + R.GRID_THREADS
    _check_noise(got, ref, 0.1, 'grid stride, n %d' % got.size)


def test_noise_moments_and_independence():
    """The bounds of tests/test_rng_host.py on the device's own output, divided by std.  What rounding to bf16 adds: the error is
    symmetric about zero, so the odd moments and the correlations gain no systematic term, and their spread grows by a relative 2^-17
    at the most, far inside 5 se.  The variance gains E (z delta)^2 with delta uniform within half a bf16 unit: a relative 2^-18 / 3 in the
    mean over a binade (2^-16 / 3, 5e-6, at the worst; 5 sqrt(2) se is 2.4e-3), and the fourth moment six times that relative to 3.
    max|z| may round up by one part in 2^8 and carries the elementwise allowance A."""
    got, _, _ = _big_noise()
    z = got / 0.1
    n = z.size
    q_var = 2.0 ** -18 / 3
    widen = {'var - 1': q_var, 'E z^4 - 3': 3 * 6 * q_var}
    st = R.noise_statistics(z)
    assert len(st) == 12
    for name, (v, se) in st.items():
        print('   %-22s %+.3e  = %+.2f se' % (name, v, v / se))
    for name, (v, se) in st.items():
        assert abs(v) <= 5 * se + widen.get(name, 0.0), (name, v, se)
    assert np.abs(z).max() <= R.MAX_ABS * (1 + 2.0 ** -8) + A
    assert n == R.BIG_NOISE['n']


def _mask(n, rate, seed, offset, launch=None):
    from van_gan_amd import ops
    buf = torch.full((n + GUARD,), -3.0, dtype=torch.float32, device=DEV)
    (launch or (lambda out: ops.dropout_mask(out, rate, seed, offset)))(buf[:n])
    torch.cuda.synchronize()
    return buf[:n].cpu(), bool((buf[n:] == -3.0).all())


def _check_mask(got, guard_ok, n, rate, seed, offset):
    assert guard_ok, 'wrote past n'
    keep = torch.from_numpy(R.dropout_keep(n, rate, seed, offset))
    assert torch.equal(got != 0, keep), 'kept / dropped differ in %d of %d' % (int(((got != 0) != keep).sum()), n)
    kept = np.float32(1) / (np.float32(1) - np.float32(rate))
    vals = got[keep].numpy()
    assert np.all(np.abs(vals.astype(np.float64) - float(kept)) <= float(np.spacing(kept))), np.unique(vals)      # 1 ulp: the device's division
    assert np.all(got[~keep].numpy() == 0)


SMALL_MASK = [(n, rate, HI + 1000 * n + j, off) for n in (1, 3, 255, 257)
              for j, (rate, off) in enumerate(((0.0, 0), (0.2, 2 ** 32 - 2), (0.5, 5 * 2 ** 33 + 1)))]


@pytest.mark.parametrize('n,rate,seed,offset', SMALL_MASK)
def test_mask_matches_restatement(n, rate, seed, offset):
    got, guard_ok = _mask(n, rate, seed, offset)
    _check_mask(got, guard_ok, n, rate, seed, offset)
    if rate == 0.0:
        assert bool((got == 1).all())


def test_mask_grid_stride_and_carry():
    c = R.BIG_MASK
    assert c['n'] > R.GRID_THREADS and c['offset'] < 2 ** 32 < c['offset'] + c['n'] and c['seed'] >> 32
    got, guard_ok = _mask(c['n'], c['rate'], c['seed'], c['offset'])
    _check_mask(got, guard_ok, c['n'], c['rate'], c['seed'], c['offset'])
    v, se = R.keep_statistic((got != 0).numpy(), c['rate'])
    print('   keep share - 0.8 = %+.3e = %+.2f se' % (v, v / se))
    assert abs(v) <= 5 * se


def test_dev_variants_read_counter_and_sigma_from_device_memory():
    """vg_randn_bf16_dev / vg_dropout_mask_dev (the launches of a captured train step): offset = *offset_dev + offset_add is formed on
    the device, here across the carry of the low word, and a relaunch after the device words were rewritten follows them."""
    from van_gan_amd import ops
    seed, n, add = HI + 5, 1027, 9
    off = torch.zeros(1, dtype=torch.int64, device=DEV)          # the 8-byte counter base
    std = torch.zeros(1, dtype=torch.float32, device=DEV)        # the 4-byte sigma
    for base, sigma in ((2 ** 32 - 5, 0.1), (7 * 2 ** 32 - 3, 0.25)):
        off.fill_(base); std.fill_(sigma)
        got, g_ok = _noise(n, None, None, None, lambda out: ops.randn_bf16_dev(out, std.data_ptr(), seed, off.data_ptr(), add))
        want, w_ok = _noise(n, sigma, seed, base + add)
        assert g_ok and w_ok
        assert np.array_equal(got, want), (base, int((got != want).sum()))
        _check_noise(got, R.randn(n, sigma, seed, base + add), sigma, '_dev, base %#x' % base)
        got, g_ok = _mask(n, None, None, None, lambda out: ops.dropout_mask_dev(out, 0.2, seed, off.data_ptr(), add))
        want, w_ok = _mask(n, 0.2, seed, base + add)
        assert g_ok and w_ok and torch.equal(got, want), base
        _check_mask(got, g_ok, n, 0.2, seed, base + add)


def test_bad_arguments_launch_nothing():
    from van_gan_amd import ops
    from van_gan_amd._lib import VgError, lib
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    std = torch.ones(1, dtype=torch.float32, device=DEV)
    z = torch.full((64,), 9.0, dtype=torch.bfloat16, device=DEV)
    m = torch.full((64,), -3.0, dtype=torch.float32, device=DEV)
    s = ops.stream()
    assert lib.vg_randn_bf16_dev(z.data_ptr(), 64, None, 1, off.data_ptr(), 0, s) == VG_EINVAL
    assert lib.vg_randn_bf16_dev(z.data_ptr(), 64, std.data_ptr(), 1, None, 0, s) == VG_EINVAL
    assert lib.vg_randn_bf16_dev(None, 64, std.data_ptr(), 1, off.data_ptr(), 0, s) == VG_EINVAL
    assert lib.vg_dropout_mask_dev(m.data_ptr(), 64, 0.2, 1, None, 0, s) == VG_EINVAL
    for rate in (1.0, 1.5, -0.1):
        assert lib.vg_dropout_mask_dev(m.data_ptr(), 64, rate, 1, off.data_ptr(), 0, s) == VG_EINVAL, rate
        assert lib.vg_dropout_mask(m.data_ptr(), 64, rate, 1, 0, s) == VG_EINVAL, rate
    with pytest.raises(VgError):
        ops.dropout_mask(m, 1.0, 1, 0)
    torch.cuda.synchronize()
    assert bool((z == 9.0).all()) and bool((m == -3.0).all())


def test_engine_counter_accounting():
    """VanGan._make_noise: the five noise views and the masks of an application are exactly what direct launches give with the engine's
    keys at the counter recorded before the call; the counter advances by ceil(flat / 4) + the masks' elements; the next application's
    range begins where this one ended, so no two draws of one key share a counter."""
    from van_gan_amd import VanGan, ops
    eng = VanGan((32, 32, 32), batch_size=1, device=DEV, seed=3, layer_noise=0.1, dropout_rate=0.2, precision='fp32', wasserstein=True,
                 lr=1e-4, beta_1=0.0, beta_2=0.9, clipnorm=0.0)
    eng.rng_offset = 2 ** 32 - 100000                      # a checkpointed counter: the first application crosses the carry
    eng.arena.reset()
    N = 2
    spans = []
    for disc in (eng.disc_S, eng.disc_I):
        off0 = eng.rng_offset
        noise, drop = eng._make_noise(disc, N, eng.arena)
        shapes = disc.noise_shapes(N)
        assert list(noise) == ['conv0', 'down0', 'down1', 'down2', 'out'] and {k: tuple(v.shape) for k, v in noise.items()} == shapes
        sizes = [int(np.prod(s)) for s in shapes.values()]
        flat_n = sum((s + 7) // 8 * 8 for s in sizes)
        flat = torch.empty(flat_n, dtype=torch.bfloat16, device=DEV)
        ops.randn_bf16(flat, eng.layer_noise, eng.noise_key, off0)
        o = 0
        for (k, v), s in zip(noise.items(), sizes):
            assert torch.equal(v.reshape(-1), flat[o:o + s]), k
            o += (s + 7) // 8 * 8
        off1 = off0 + (flat_n + 3) // 4
        chans = (('down0', 128), ('down1', 256), ('down2', 512))
        dflat = torch.empty(N * sum(c for _, c in chans), dtype=torch.float32, device=DEV)
        ops.dropout_mask(dflat, eng.dropout_rate, eng.drop_key, off1)
        o = 0
        for k, c in chans:
            assert tuple(drop[k].shape) == (N, c) and torch.equal(drop[k].reshape(-1), dflat[o:o + N * c]), k
            o += N * c
        off2 = off1 + dflat.numel()
        head = torch.empty(N * disc.n_patch, dtype=torch.float32, device=DEV)
        ops.dropout_mask(head, eng.dropout_rate, eng.drop_key + 77, off2)
        assert disc.n_patch == 64 and tuple(drop['head'].shape) == (N, 64) and torch.equal(drop['head'].reshape(-1), head)
        assert set(drop) == {'down0', 'down1', 'down2', 'head'}
        assert eng.rng_offset == off2 + head.numel() == off0 + (flat_n + 3) // 4 + dflat.numel() + head.numel()
        spans.append((off0, eng.rng_offset))
        # the restatement, on what is cheap to restate: the masks, and the head of the noise buffer
        assert torch.equal(dflat.cpu() != 0, torch.from_numpy(R.dropout_keep(dflat.numel(), eng.dropout_rate, eng.drop_key, off1)))
        _check_noise(flat[:4096].double().cpu().numpy(), R.randn(4096, eng.layer_noise, eng.noise_key, off0), eng.layer_noise, 'engine')
    assert spans[0][0] < 2 ** 32 < spans[0][1] and spans[1][0] == spans[0][1]
