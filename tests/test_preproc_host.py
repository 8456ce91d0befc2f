"""CPU: the host side of the raw-volume preprocessing -- the float64 restatement the GPU tests compare against (tests/preproc_restate.py)
pinned to scipy.stats.scoreatpercentile and to the plain numpy loop, the new entries' declaration / prototype / export in both libraries,
their argument checks (which launch nothing), the rank / fraction computation of percentiles and the input validation of prepare_imaging,
which runs before any device access."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.stats
import torch

import preproc_restate as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERS = [0, 0.05, 50, 99.95, 100]


def _tied(n, seed):
    """float32 values with many ties (a few hundred distinct values, both signs, both zeros)."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(-120, 120, n) / np.float32(8)).astype(np.float32)
    a[rng.random(n) < 0.05] = np.float32(-0.0)
    return a


@pytest.mark.parametrize('n', [1, 2, 23919])
@pytest.mark.parametrize('per', PERS)
def test_restated_percentile_is_scipy_bit_for_bit(n, per):
    a = _tied(n, n)
    want = np.float64(scipy.stats.scoreatpercentile(a, per))
    got = P.percentile(a, per)
    assert isinstance(got, np.float64) and got.tobytes() == want.tobytes(), (got, want)
    got3 = P.percentile(a.reshape(-1, 1, 1) if n < 3 else a[:n - n % 3].reshape(3, -1, 1), per)       # any shape: the flattened values
    assert got3 == np.float64(scipy.stats.scoreatpercentile(a if n < 3 else a[:n - n % 3], per))


def test_restated_zscore_is_the_numpy_loop():
    rng = np.random.default_rng(3)
    x = rng.normal(3.0, 2.0, (9, 7, 5)).astype(np.float32)
    x[..., 2] = 4.0                                                         # a constant slice: the s == 0 branch
    want = x.astype(np.float64)
    for z in range(x.shape[2]):                                             # z_score_norm applied slice by slice, in float64
        sl = want[..., z].copy()
        sd = np.std(sl)
        want[..., z] = (sl - np.mean(sl)) / sd if sd > 0. else sl - np.mean(sl)
    got = P.zscore_slices(x)
    assert np.array_equal(got, want) and (got[..., 2] == 0).all()
    assert np.array_equal(P.zscore_slices(x[..., None]), want)
    ms = P.slice_moments(x)
    assert ms.shape == (5, 2) and ms[2, 1] == 0 and ms[2, 0] == 4.0
    assert np.allclose(ms[:, 0], [x[..., z].astype(np.float64).mean() for z in range(5)], rtol=1e-15)
    r = P.prepare(x)
    assert r['out'].min() == -1.0 and r['out'].max() == 1.0 and r['lp'] < r['up']
    assert r['clipped'].min() == r['lp'] and r['clipped'].max() == r['up']


ENTRIES = (('vg_slice_moments', 8), ('vg_zscore_slices', 8), ('vg_order_stats', 8), ('vg_clip_rescale', 9),
           ('vg_slice_moments_scratch_bytes', 2), ('vg_order_stats_scratch_bytes', 2))


def test_entry_points_declared_prototyped_and_exported():
    from van_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    for name, nargs in ENTRIES:
        assert re.search(r'^(?:int|int64_t)\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name)
    assert 'vg_preproc.hip' in build.SOURCES
    import van_gan_amd
    for name in ('slice_moments', 'zscore_slices', 'order_stats', 'percentiles', 'preprocess_rsom_images', 'prepare_imaging'):
        assert callable(getattr(van_gan_amd, name))
    assert callable(van_gan_amd.VanGan.segment_volume)


PTR = 1 << 20                              # never dereferenced: every call below is rejected on its arguments


def _libs():
    from van_gan_amd._lib import lib, lib_fp16
    return [lib, lib_fp16()]


def _order_stats(L, n=1000, ranks=(0, 999), R=None, x=PTR, out=PTR, scratch=PTR, short=0):
    nbytes = L.vg_order_stats_scratch_bytes(1000, 2)
    assert nbytes > 0
    rk = (C.c_int64 * max(len(ranks), 1))(*ranks)
    return L.vg_order_stats(x, n, rk, len(ranks) if R is None else R, out, scratch, nbytes - short, None)


@pytest.mark.parametrize('bad', [dict(n=0, ranks=(0,)), dict(n=2 ** 31, ranks=(0,)), dict(ranks=(0, 1, 2, 3, 4)), dict(ranks=(0, 1000)),
                                 dict(short=1), dict(ranks=(-1,)), dict(ranks=()), dict(x=None), dict(out=None), dict(scratch=None)],
                         ids=['n=0', 'n=2^31', 'R=5', 'rank=n', 'scratch-1', 'rank<0', 'R=0', 'x=NULL', 'out=NULL', 'scratch=NULL'])
def test_order_stats_rejects_bad_arguments_without_a_gpu(bad):
    for L in _libs():
        assert _order_stats(L, **bad) == -1, bad
        assert L.vg_order_stats_scratch_bytes(0, 1) == -1 and L.vg_order_stats_scratch_bytes(2 ** 31, 1) == -1
        assert L.vg_order_stats_scratch_bytes(10, 5) == -1 and L.vg_order_stats_scratch_bytes(2 ** 31 - 1, 4) > 0


def _moments(L, dtype=0, nxy=64, Z=23, vol=PTR, ms=PTR, scratch=PTR, short=0):
    return L.vg_slice_moments(vol, dtype, nxy, Z, ms, scratch, L.vg_slice_moments_scratch_bytes(64, 23) - short, None)


def _zscore(L, dtype=0, nxy=64, Z=23, vol=PTR, ms=PTR, out=PTR, ctr=PTR):
    return L.vg_zscore_slices(vol, dtype, nxy, Z, ms, out, ctr, None)


@pytest.mark.parametrize('bad', [dict(dtype=3), dict(dtype=-1), dict(nxy=0), dict(Z=0), dict(vol=None), dict(ms=None)],
                         ids=['dtype=3', 'dtype=-1', 'nxy=0', 'Z=0', 'vol=NULL', 'mean_std=NULL'])
def test_moments_and_zscore_reject_bad_arguments_without_a_gpu(bad):
    for L in _libs():
        assert _moments(L, **bad) == -1 and _zscore(L, **bad) == -1, bad


def test_scratch_one_byte_short_is_rejected():
    for L in _libs():
        assert L.vg_slice_moments_scratch_bytes(64, 23) == 64 * 23 * 16 and L.vg_slice_moments_scratch_bytes(10 ** 6, 140) == 1024 * 140 * 16
        assert _moments(L, short=1) == -1 and _moments(L, scratch=None) == -1 and _moments(L, scratch=PTR + 8) == -1
        assert _zscore(L, out=None) == -1 and _zscore(L, ctr=None) == -1
        assert _zscore(L, dtype=1, vol=PTR + 1) == -1 and _moments(L, dtype=2, vol=PTR + 2) == -1          # misaligned for the dtype


def test_clip_rescale_rejects_bad_arguments_without_a_gpu():
    for L in _libs():
        f = lambda **o: L.vg_clip_rescale(*[o.get(k, d) for k, d in (('z', PTR), ('n', 100), ('stats', PTR), ('f_lo', 0.25), ('f_hi', 0.5), ('rescale', 1),
                                                                     ('limits', PTR), ('out', PTR), ('stream', None))])
        for bad in (dict(z=None), dict(stats=None), dict(limits=None), dict(out=None), dict(n=0), dict(f_lo=-0.1), dict(f_hi=1.5),
                    dict(f_lo=float('nan')), dict(rescale=2), dict(z=PTR + 2)):
            assert f(**bad) == -1, bad


def test_percentile_rank_and_fraction():
    from van_gan_amd.preprocess import percentile_rank
    assert percentile_rank(1, 0.05) == (0, 0, 0.0) and percentile_rank(1, 100) == (0, 0, 0.0) and percentile_rank(1, 50) == (0, 0, 0.0)
    assert percentile_rank(5, 50) == (2, 3, 0.0) and percentile_rank(5, 100) == (4, 4, 0.0) and percentile_rank(5, 0) == (0, 1, 0.0)
    assert percentile_rank(9, 25) == (2, 3, 0.0)                           # an integral index: fraction 0, a[lower] alone counts
    lo, hi, f = percentile_rank(23919, 0.05)
    assert (lo, hi) == (11, 12) and f == 0.05 / 100.0 * 23918 - 11
    lo, hi, f = percentile_rank(23919, 99.95)
    assert (lo, hi) == (23906, 23907) and 0.0 < f < 1.0
    for n in (1, 2, 7, 23919, 2 ** 31 - 1):
        for per in PERS + [12.5, 33.3]:
            assert percentile_rank(n, per) == P.rank_fraction(n, per)
            lo, hi, f = percentile_rank(n, per)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= f < 1.0
    for bad in (-0.1, 100.5, float('nan')):
        with pytest.raises(ValueError):
            percentile_rank(10, bad)
    with pytest.raises(ValueError):
        percentile_rank(0, 50)
    # the interpolation the device forms from (rank, fraction) is scipy's value
    a = _tied(23919, 5)
    srt = np.sort(a)
    for per in PERS:
        lo, hi, f = percentile_rank(a.size, per)
        v = np.float64(srt[lo]) * (1.0 - f) + np.float64(srt[hi]) * f
        assert v == np.float64(scipy.stats.scoreatpercentile(a, per))


def test_prepare_imaging_validates_before_touching_the_device(monkeypatch):
    from van_gan_amd import preprocess

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(preprocess, '_resolve_device', no_device)
    for bad in (np.zeros((4, 4, 4, 1, 1), np.uint8), np.zeros((4, 4, 4), np.float64), torch.zeros(4, 4, 4, 1, 1), torch.zeros(4, 4, 4, dtype=torch.float64),
                np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4, 2), np.float32), np.zeros((4, 4, 4), np.int16), torch.zeros(4, 4, 4, dtype=torch.int16),
                np.zeros((4, 0, 4), np.uint8), [[[1.0]]]):
        with pytest.raises(ValueError):
            preprocess.prepare_imaging(bad)
        with pytest.raises(ValueError):
            preprocess.zscore_slices(bad)
    vol = np.zeros((4, 4, 4), np.uint8)
    for kw in (dict(preprocess='zscore'), dict(lower_thresh=-1.0), dict(upper_thresh=100.5), dict(lower_thresh=float('nan'))):
        with pytest.raises(ValueError):
            preprocess.prepare_imaging(vol, **kw)
    with pytest.raises(ValueError):
        preprocess.order_stats(torch.zeros(8), [0])                         # a host tensor
    assert preprocess.MINMAX_ERROR == 'Cannot perform min-max normalization when max and min are equal.'
