"""CPU: the host side of the imaging filters -- the numpy restatement the GPU tests compare against (tests/filters_restate.py) pinned to
scipy.ndimage.median_filter and to the literal numpy recipe of threshold_outliers, the new entries' declaration / prototype / export in
both libraries, their argument checks (which launch nothing), and the validation of median_filter / threshold_outliers / prepare_imaging,
which runs before any device access."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch

import filters_restate as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 7, 4), (17, 9, 33), (5, 5, 130), (3, 66, 2)]


def _volume(kind, shape):
    rng = np.random.default_rng(sum((i + 2) * s for i, s in enumerate(shape)))
    if kind == 'uint8':                                                     # four distinct values: heavy ties
        return rng.choice(np.array([0, 3, 200, 255], np.uint8), shape).astype(F32)
    if kind == 'uint16':
        return rng.integers(0, 65536, shape).astype(np.uint16).astype(F32)
    return rng.standard_normal(shape).astype(F32)


@pytest.mark.parametrize('size', [(3, 3, 3), (3, 3, 1)])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', ['uint8', 'uint16', 'float32'])
def test_restated_median_is_scipy(kind, shape, size):
    x = _volume(kind, shape)
    want = scipy.ndimage.median_filter(x, size=size)
    got = FR.median(x, size)
    assert got.dtype == F32 and got.shape == x.shape and np.array_equal(got, want)


def test_restated_median_int_size_and_known_answers():
    x = _volume('float32', (6, 5, 7))
    assert np.array_equal(FR.median(x, 3), FR.median(x, (3, 3, 3)))
    assert np.array_equal(FR.median(x, 1), x)
    hot = np.zeros((5, 5, 5), F32)
    hot[2, 2, 2] = 9.0
    assert not FR.median(hot, 3).any()


@pytest.mark.parametrize('kind', ['uint16', 'uint8', 'float32'])
def test_restated_outlier_limits_are_the_numpy_recipe(kind):
    x = FR.limit_volumes()[kind].astype(F32)
    thr = 6
    mean, std = x.mean(), x.std()                                           # numpy's own float32 moments
    assert mean.dtype == F32 and std.dtype == F32
    z = np.abs((x - mean) / std)
    upper, lower = np.max(x[z <= thr]), np.min(x[z <= thr])
    lo, hi, kept = FR.outlier_limits(x, mean, std, thr)
    assert (lo, hi, kept) == (lower, upper, int((z <= thr).sum()))
    assert lower > x.min() or upper < x.max()                               # the threshold does clip something
    want = np.clip(x, a_min=lower, a_max=upper)
    assert np.array_equal(np.clip(x, lo, hi), want)
    # the precondition of the GPU limits test holds on these volumes: the limits do not move with an ulp of either moment
    nine = FR.limits_at_neighbours(x, thr)
    assert all(r == nine[0] for r in nine)
    assert np.array_equal(FR.threshold_outliers(x, thr), np.clip(x, nine[0][0], nine[0][1]))


def test_restated_outlier_limits_edge_cases():
    c = np.full((3, 4, 5), 7.0, F32)
    assert FR.outlier_limits(c, F32(7.0), F32(0.0), 6) == (F32(np.inf), F32(-np.inf), 0)
    x = np.arange(60, dtype=F32).reshape(3, 4, 5).copy()
    x[1, 2, 3] = np.nan
    m, s = F32(np.nanmean(x)), F32(np.nanstd(x))
    lo, hi, kept = FR.outlier_limits(x, m, s, 6)
    assert (lo, hi, kept) == (F32(0), F32(59), 59)


ENTRIES = (('vg_median3', 11), ('vg_volume_moments_scratch_bytes', 1), ('vg_volume_moments', 7), ('vg_outlier_limits', 8))


def test_entry_points_declared_prototyped_and_exported():
    from van_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    assert 'Imaging filters' in hdr
    for name, nargs in ENTRIES:
        assert re.search(r'^(?:int|int64_t)\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name)
    assert 'vg_filters.hip' in build.SOURCES
    import van_gan_amd
    for name in ('median_filter', 'volume_moments', 'outlier_limits', 'threshold_outliers', 'prepare_imaging'):
        assert callable(getattr(van_gan_amd, name))


PTR = 1 << 20                              # never dereferenced: every call below is rejected on its arguments


def _libs():
    from van_gan_amd._lib import lib, lib_fp16
    return [lib, lib_fp16()]


def _median(L, **o):
    a = dict(vol=PTR, dtype=2, X=4, Y=5, Z=6, sx=3, sy=3, sz=3, out=PTR * 2, ctr=PTR * 3)
    a.update(o)
    return L.vg_median3(a['vol'], a['dtype'], a['X'], a['Y'], a['Z'], a['sx'], a['sy'], a['sz'], a['out'], a['ctr'], None)


@pytest.mark.parametrize('bad', [dict(vol=None), dict(out=None), dict(ctr=None), dict(dtype=3), dict(dtype=-1), dict(X=0), dict(Y=0), dict(Z=0),
                                 dict(Z=(1 << 20) + 1), dict(X=1 << 20, Y=1 << 20), dict(sx=2), dict(sy=5), dict(sz=0), dict(sx=-3),
                                 dict(out=PTR), dict(out=PTR + 4 * 119), dict(vol=PTR * 2 + 4 * 119), dict(vol=PTR + 2), dict(out=PTR * 2 + 2),
                                 dict(dtype=1, vol=PTR + 1)],
                         ids=['vol=NULL', 'out=NULL', 'ctr=NULL', 'dtype=3', 'dtype=-1', 'X=0', 'Y=0', 'Z=0', 'Z>2^20', 'XY=2^40', 'sx=2', 'sy=5',
                              'sz=0', 'sx=-3', 'out=vol', 'out-in-vol', 'vol-in-out', 'vol-misaligned', 'out-misaligned', 'u16-misaligned'])
def test_median3_rejects_bad_arguments_without_a_gpu(bad):
    for L in _libs():
        assert _median(L, **bad) == -1, bad


def test_moments_and_limits_reject_bad_arguments_without_a_gpu():
    for L in _libs():
        nbytes = L.vg_volume_moments_scratch_bytes(1000)
        assert nbytes > 0 and nbytes % 16 == 0
        assert L.vg_volume_moments_scratch_bytes(0) == -1 and L.vg_volume_moments_scratch_bytes(1 << 60) == -1
        mo = lambda **o: L.vg_volume_moments(*[o.get(k, d) for k, d in (('vol', PTR), ('dtype', 1), ('n', 1000), ('ms', PTR * 2), ('scratch', PTR * 3),
                                                                          ('nbytes', nbytes), ('stream', None))])
        for bad in (dict(vol=None), dict(ms=None), dict(scratch=None), dict(dtype=3), dict(n=0), dict(n=1 << 60), dict(nbytes=nbytes - 1),
                    dict(scratch=PTR * 3 + 8), dict(vol=PTR + 1), dict(ms=PTR * 2 + 2)):
            assert mo(**bad) == -1, bad
        ol = lambda **o: L.vg_outlier_limits(*[o.get(k, d) for k, d in (('vol', PTR), ('dtype', 2), ('n', 1000), ('ms', PTR * 2), ('thr', 6.0),
                                                                          ('stats', PTR * 3), ('counts', PTR * 4), ('stream', None))])
        for bad in (dict(vol=None), dict(ms=None), dict(stats=None), dict(counts=None), dict(dtype=-1), dict(n=0), dict(thr=0.0), dict(thr=-1.0),
                    dict(thr=float('nan')), dict(thr=float('inf')), dict(vol=PTR + 2), dict(stats=PTR * 3 + 1)):
            assert ol(**bad) == -1, bad


def test_arguments_are_validated_before_the_device_is_touched(monkeypatch):
    from van_gan_amd import preprocess

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(preprocess, '_resolve_device', no_device)
    vol = np.zeros((4, 4, 4), np.uint8)
    for pre in ('zscore', ('median', 'zscore'), ('median', 'median'), ('rsom', 'outliers', 'rsom'), (), ('median', None), 3, ['outliers', 'Median']):
        with pytest.raises(ValueError):
            preprocess.prepare_imaging(vol, preprocess=pre)
    for size in (2, 5, (3, 3), (3, 3, 2), 0, 3.0, 'x', (3, 3, 3, 3)):
        with pytest.raises(ValueError):
            preprocess.prepare_imaging(vol, preprocess='median', median_size=size)
        with pytest.raises(ValueError):
            preprocess.median_filter(vol, size=size)
    for thr in (0, -1, float('nan'), float('inf'), 'x', 1e-60):
        with pytest.raises(ValueError):
            preprocess.prepare_imaging(vol, preprocess='outliers', outlier_threshold=thr)
        with pytest.raises(ValueError):
            preprocess.threshold_outliers(vol, threshold=thr)
        with pytest.raises(ValueError):
            preprocess.outlier_limits(vol, threshold=thr)
    # the keywords are checked whatever the stages, and a float64 volume is refused by every entry
    with pytest.raises(ValueError):
        preprocess.prepare_imaging(vol, preprocess='rsom', median_size=2)
    for bad in (np.zeros((4, 4, 4), np.float64), torch.zeros(4, 4, 4, dtype=torch.float64)):
        for fn in (preprocess.median_filter, preprocess.volume_moments, preprocess.outlier_limits, preprocess.threshold_outliers):
            with pytest.raises(ValueError):
                fn(bad)
        for pre in ('median', 'outliers', ('median', 'rsom')):
            with pytest.raises(ValueError):
                preprocess.prepare_imaging(bad, preprocess=pre)
    # a valid call gets as far as the device, and no further
    for pre in ('median', 'outliers', ('median', 'rsom'), ['outliers', 'median'], 'rsom', None):
        with pytest.raises(AssertionError, match='the device was touched'):
            preprocess.prepare_imaging(vol, preprocess=pre, median_size=(3, 3, 1), outlier_threshold=2.5)
    assert preprocess.OUTLIERS_ERROR == 'threshold_outliers: no voxel lies within the threshold'
