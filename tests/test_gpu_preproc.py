"""GPU: the raw-volume preprocessing kernels (csrc/vg_preproc.hip) and van_gan_amd/preprocess.py built on them, against float64 numpy
(tests/preproc_restate.py).  The radix select is compared with np.sort by value equality, no tolerance; moments, z-scores and the end-to-end
result against bounds derived from the fp32 roundings involved (see the tests); the last stage bit for bit against the device-order
restatement fed with the device's own z-scores."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import preproc_restate as P  # noqa: E402
import gpu_helpers  # noqa: E402
from gpu_helpers import _dev, _Recorder  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------ selection
SIZES = [1, 63, 64, 65, 1000003]
KINDS = ['equal', 'two', 'uint8', 'mixed']


def _select_data(kind, n):
    rng = np.random.default_rng(n + len(kind))
    if kind == 'equal':
        return np.full(n, -2.75, F32)
    if kind == 'two':
        return np.where(rng.random(n) < 0.3, F32(-1.5), F32(4.0)).astype(F32)
    if kind == 'uint8':
        return np.minimum(rng.poisson(9.0, n), 255).astype(np.uint8).astype(F32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3e38, -3e38, 1.0, -1.0], F32)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(F32)
    idx = rng.random(n) < 0.4
    a[idx] = special[rng.integers(0, len(special), int(idx.sum()))]
    assert np.isfinite(a).all()
    return a


def _straddle(srt):
    """k such that sorted[k] and sorted[k+1] straddle the end of a run of ties (the boundary nearest the middle), or the middle."""
    n = srt.size
    if n < 2:
        return 0
    edges = np.flatnonzero(srt[1:] != srt[:-1])
    return int(edges[np.abs(edges - n // 2).argmin()]) if edges.size else (n - 2) // 2


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_order_stats_is_exact(kind, n):
    from van_gan_amd.preprocess import order_stats
    a = _select_data(kind, n)
    srt = np.sort(a)
    x = _dev(a)
    k = _straddle(srt)
    mid = n // 3
    rank_sets = [(0,), (n - 1,), (0, n - 1, mid, mid), (k, min(k + 1, n - 1)), (max(k - 1, 0), k, min(k + 1, n - 1), min(k + 2, n - 1))]
    before = x.clone()
    for ranks in rank_sets:
        got = order_stats(x, ranks).cpu().numpy()
        want = srt[list(ranks)]
        assert got.dtype == F32 and got.shape == (len(ranks),)
        assert (got == want).all(), (kind, n, ranks, got, want)
    assert torch.equal(x, before)
    x2 = _dev(np.concatenate([np.zeros(1, F32), a]))[1:]               # a pointer that is 4- but not 16-byte aligned: the scalar kernel
    assert x2.data_ptr() % 16 == 4
    ranks = (k, min(k + 1, n - 1), 0, n - 1)
    assert (order_stats(x2, ranks).cpu().numpy() == srt[list(ranks)]).all()


def test_order_stats_ranks_part_in_every_digit_pass():
    """Neighbouring sorted values that differ in sign, in the exponent only, in high mantissa bits only, in a middle mantissa byte and in
    the last bit: whatever the digit width, some pair of ranks parts ways in the first, a middle and the last digit pass."""
    from van_gan_amd.preprocess import order_stats
    v = [F32(-1.0), F32(0.5), F32(1.0), np.array([0x3F800100], np.uint32).view(F32)[0]]
    v.append(np.nextafter(v[-1], F32(2.0)))
    v += [F32(1.5), np.nextafter(F32(1.5), F32(2.0)), F32(2.0), F32(1024.0)]
    v = np.array(v, F32)
    assert (np.diff(v) > 0).all()
    counts = np.array([700, 1, 333, 64, 65, 2, 1000, 63, 5])
    a = np.repeat(v, counts)
    np.random.default_rng(0).shuffle(a)
    srt = np.sort(a)
    x = _dev(a)
    ends = np.cumsum(counts)[:-1] - 1                                       # k with sorted[k] != sorted[k + 1]
    assert (srt[ends] != srt[ends + 1]).all() and len(ends) == 8
    for i in range(0, len(ends), 2):
        ranks = [int(ends[i]), int(ends[i]) + 1, int(ends[i + 1]), int(ends[i + 1]) + 1]
        got = order_stats(x, ranks).cpu().numpy()
        assert (got == srt[ranks]).all() and got[0] != got[1] and got[2] != got[3], (ranks, got, srt[ranks])
        assert got.tobytes() == srt[ranks].tobytes()                        # no zeros here: the bit patterns agree as well


def test_percentiles_are_scipys():
    import scipy.stats
    from van_gan_amd.preprocess import percentiles
    a = _select_data('uint8', 23919) / F32(7) - F32(1)
    pers = [0, 0.05, 50, 99.95, 100]
    got = percentiles(_dev(a), pers)
    want = np.array([scipy.stats.scoreatpercentile(a, p) for p in pers], np.float64)
    assert got.dtype == np.float64 and np.array_equal(got, want), (got, want)
    assert percentiles(_dev(a), 50).shape == (1,)


# ------------------------------------------------------------------------------------------------ slice moments and z-score
SHAPES = [(37, 29, 23), (5, 3, 140), (64, 64, 1), (3, 2, 300), (3, 2, 301)]      # 301: odd, one z per lane, two column chunks of 256
DTYPES = ['uint8', 'uint16', 'float32', 'uint16-large-mean']


@functools.lru_cache(maxsize=None)
def _volume(shape, dtype):
    rng = np.random.default_rng(sum(shape) + len(dtype))
    Z = shape[2]
    if dtype == 'uint8':
        v = np.minimum(rng.poisson(20.0, shape) * (1 + np.arange(Z) % 3), 255).astype(np.uint8)
    elif dtype == 'uint16':
        v = rng.integers(0, 65536, shape).astype(np.uint16)
    elif dtype == 'uint16-large-mean':
        v = np.rint(rng.normal(30000.0, 50.0, shape)).astype(np.uint16)
    else:
        v = (rng.normal(3.0, 2.0, shape) * (1.0 + 0.25 * (np.arange(Z) % 5))).astype(F32)
    if Z > 1:
        v[..., Z // 2] = 7                                                   # one exactly constant slice (an integer: float64 numpy is exact too)
    v.setflags(write=False)
    return v


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_slice_moments_and_zscore(shape, dtype):
    from van_gan_amd.preprocess import slice_moments, zscore_slices
    v = _volume(shape, dtype)
    Z = shape[2]
    ms64 = P.slice_moments(v)
    ms = slice_moments(v).cpu().numpy()
    assert ms.dtype == F32 and ms.shape == (Z, 2)
    err = np.abs(ms.astype(np.float64) - ms64)
    rel = (err / np.maximum(np.abs(ms64), 1e-300)).max()
    print('%s %s: moments max rel err %.3g (bound %.3g)' % (shape, dtype, rel, 2.0 ** -23))
    assert (err <= 2.0 ** -23 * np.abs(ms64)).all()
    if Z > 1:
        assert ms[Z // 2, 1] == 0.0 and ms[Z // 2, 0] == 7.0 and ms64[Z // 2, 1] == 0.0
    assert np.array_equal(slice_moments(v).cpu().numpy(), ms)               # bitwise reproducible
    z, count = zscore_slices(v, return_count=True)
    z = z.cpu().numpy()
    assert z.dtype == F32 and z.shape == shape and int(count) == 0
    z64, bound = P.zscore_slices(v), P.zscore_bound(v)
    ez = np.abs(z.astype(np.float64) - z64)
    print('%s %s: z-score max err / bound %.3f' % (shape, dtype, (ez / bound).max()))
    assert (ez <= bound).all()
    if Z > 1:
        assert (z[..., Z // 2] == 0.0).all()
    assert np.abs(z).max() > 0.5


def test_zscore_of_an_unaligned_volume_and_a_tail():
    """An element count that is no multiple of 4 (the scalar tail) and a base pointer that is not 16-byte aligned (the scalar kernels)."""
    from van_gan_amd.preprocess import RawVolume, slice_moments, zscore_slices
    v = _volume((37, 29, 23), 'float32')
    assert v.size % 4 == 3
    ref_ms, ref_z = slice_moments(v), zscore_slices(v)
    buf = _dev(np.concatenate([np.zeros(1, F32), v.ravel()]))[1:]
    assert buf.data_ptr() % 16 == 4
    rv = RawVolume(buf, 2, v.shape)
    assert torch.equal(slice_moments(rv), ref_ms)
    assert torch.equal(zscore_slices(rv), ref_z)


# ------------------------------------------------------------------------------------------------ end to end
def _sparse():
    rng = np.random.default_rng(21)
    v = np.where(rng.random((24, 20, 12)) < 0.03, 200, 0).astype(np.uint8)
    return v


E2E = {'uint8': lambda: _volume((37, 29, 23), 'uint8'), 'uint16': lambda: _volume((37, 29, 23), 'uint16'),
       'float32-constant-slice': lambda: _volume((16, 19, 7), 'float32'), 'sparse-uint8': _sparse}


@pytest.mark.parametrize('name', list(E2E))
def test_prepare_imaging_matches_the_restatement(name):
    from van_gan_amd.preprocess import prepare_imaging, preprocess_rsom_images, zscore_slices
    v = E2E[name]()
    ref = P.prepare(v)
    out_t = prepare_imaging(v)
    assert out_t.is_cuda and out_t.dtype == torch.float32 and out_t.shape == v.shape + (1,)
    out = out_t.cpu().numpy()[..., 0]
    lp, up = ref['lp'], ref['up']
    assert up > lp
    delta = P.zscore_bound(v).max()
    bound = 8.0 * (delta + 2.0 ** -24 * max(abs(lp), abs(up))) / (up - lp) + 2.0 ** -21
    err = np.abs(out.astype(np.float64) - ref['out']).max()
    print('%s: end-to-end max err %.3g, bound %.3g (lp %.6g, up %.6g)' % (name, err, bound, lp, up))
    assert err <= bound
    assert out.min() == -1.0 and out.max() == 1.0
    # the last stage bit for bit, from the device's own z-scores
    z32 = zscore_slices(v).cpu().numpy()
    lp32, up32, out32 = P.device_order(z32)
    assert out.tobytes() == out32.tobytes()
    clipped = preprocess_rsom_images(v).cpu().numpy()
    assert clipped.min() == lp32 and clipped.max() == up32                  # the limits block, seen through the clip-only stage
    assert np.array_equal(clipped, np.clip(z32, lp32, up32))
    # [X,Y,Z,1], a device tensor and a host tensor give the same bits (uint16 has no torch arithmetic: numpy only)
    assert torch.equal(prepare_imaging(v[..., None]), out_t)
    if v.dtype != np.uint16:
        assert torch.equal(prepare_imaging(torch.from_numpy(v.copy())), out_t) and torch.equal(prepare_imaging(_dev(v)), out_t)


def test_limits_block_is_the_restatements(monkeypatch):
    """The 2-float block vg_clip_rescale writes equals the device-order restatement's (lp, up) bitwise (read where prepare_imaging reads it)."""
    from van_gan_amd import preprocess
    seen = []
    real = preprocess._state_block

    def keep(dev):
        seen.append(real(dev))
        return seen[-1]
    monkeypatch.setattr(preprocess, '_state_block', keep)
    for name in E2E:
        v = E2E[name]()
        del seen[:]
        preprocess.prepare_imaging(v, check=False)
        host = seen[0].cpu()
        lp32, up32, _ = P.device_order(preprocess.zscore_slices(v).cpu().numpy())
        assert int(host[0]) == 0
        assert host[2:].numpy().view(F32).tobytes() == np.array([lp32, up32], F32).tobytes(), name


# ------------------------------------------------------------------------------------------------ check
def test_check_raises_on_nan_and_on_a_constant_volume():
    from van_gan_amd.preprocess import MINMAX_ERROR, prepare_imaging
    v = _volume((16, 19, 7), 'float32').copy()
    v[3, 4, 5] = np.nan
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_imaging(v)
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_imaging(v, preprocess=None)
    const = np.full((16, 19, 7), 9, np.uint8)
    with pytest.raises(ValueError) as e:
        prepare_imaging(const)
    assert str(e.value) == MINMAX_ERROR
    with pytest.raises(ValueError) as e:
        prepare_imaging(const, preprocess=None)
    assert str(e.value) == MINMAX_ERROR
    for bad in (v, const):
        for pre in ('rsom', None):
            out = prepare_imaging(bad, preprocess=pre, check=False)
            assert isinstance(out, torch.Tensor) and out.shape == (16, 19, 7, 1)
    torch.cuda.synchronize()


def test_unchecked_call_makes_the_same_calls_whatever_the_data(monkeypatch):
    from van_gan_amd import preprocess
    a = _volume((37, 29, 23), 'uint8')
    b = np.where(np.random.default_rng(5).random(a.shape) < 0.5, 3, 250).astype(np.uint8)
    calls = []
    for pre in ('rsom', None):
        for v in (a, b):
            rec = _Recorder(preprocess.lib)
            monkeypatch.setattr(preprocess, 'lib', rec)
            preprocess.prepare_imaging(v, preprocess=pre, check=False)
            monkeypatch.undo()
            calls.append(rec.names)
    assert calls[0] == calls[1] and calls[2] == calls[3]
    assert [n for n in calls[0] if not n.endswith('_scratch_bytes')] == ['vg_slice_moments', 'vg_zscore_slices', 'vg_order_stats', 'vg_clip_rescale']
    assert 'vg_minmax' in calls[2] and 'vg_order_stats' not in calls[2]


# ------------------------------------------------------------------------------------------------ plumbing
_engine = functools.lru_cache(maxsize=None)(gpu_helpers._engine)           # one engine per test module, as before


def test_segment_volume_is_prepare_then_stitch(monkeypatch):
    """48x40x36 uint8, 32^3 windows, stride (8, 8, 4).  segment_volume('gen_IS', raw, ...) is stitch_subvolumes('gen_IS',
    prepare_imaging(raw), ...): the tensor it hands to the stitch equals prepare_imaging(raw) bit for bit, the keywords arrive unchanged,
    and what it returns is the very tensor the stitch returned.  Two separate runs of the stitch cannot be compared bitwise: they differ
    in their last bits (float atomics in the overlap-add and in the generator's InstanceNorm sums; printed below,
    measured 7e-4 on the 0..255 scale), so the comparison is made on one run."""
    from van_gan_amd.preprocess import prepare_imaging
    eng = _engine()
    raw = np.minimum(np.random.default_rng(8).poisson(30.0, (48, 40, 36)), 255).astype(np.uint8)
    stitch, seen = eng.stitch_subvolumes, []

    def recording(gen, img, subvol_size=None, **kw):
        out = stitch(gen, img, subvol_size, **kw)
        seen.append((gen, img, subvol_size, kw, out))
        return out
    monkeypatch.setattr(eng, 'stitch_subvolumes', recording)
    got = eng.segment_volume('gen_IS', raw, stride=(8, 8, 4))
    assert len(seen) == 1
    gen, img, subvol_size, kw, out = seen[0]
    assert gen == 'gen_IS' and subvol_size is None and kw == dict(stride=(8, 8, 4)) and got is out
    assert img.shape == (48, 40, 36, 1) and torch.equal(img, prepare_imaging(raw))
    assert got.shape == (48, 40, 36, 1) and bool(torch.isfinite(got).all())
    assert float(got.max()) == 255.0 and float(got.min()) == 0.0
    again = stitch('gen_IS', prepare_imaging(raw), stride=(8, 8, 4))
    diff = float((again - got).abs().max())
    print('segment_volume against a second stitch of prepare_imaging(raw): max difference %.3g on the 0..255 scale' % diff)
    assert diff <= 0.05                                                     # the bound of the stitch's own parity tests: the same computation
    eng.segment_volume('gen_IS', raw, (32, 32, 32), preprocess=None, check=False, stride=(16, 16, 16), complete=False)
    gen, img, subvol_size, kw, _ = seen[1]
    assert subvol_size == (32, 32, 32) and kw == dict(stride=(16, 16, 16), complete=False)
    assert torch.equal(img, prepare_imaging(raw, preprocess=None))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32'])
def test_no_preprocess_is_the_plain_minmax(dtype):
    from van_gan_amd.preprocess import prepare_imaging
    v = _volume((37, 29, 23), dtype)
    x = v.astype(F32)
    want = F32(2) * ((x - x.min()) / (x.max() - x.min())) - F32(1)
    got = prepare_imaging(v, preprocess=None).cpu().numpy()[..., 0]
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print('%s preprocess=None: max err %.3g' % (dtype, err))
    assert err <= 2.0 ** -22 and got.min() == -1.0 and got.max() == 1.0
