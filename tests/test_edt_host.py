"""CPU: what the GPU suite of the mask measurements rests on (tests/test_gpu_edt.py compares the kernels with tests/edt_restate.py, so
the restatement itself is pinned to scipy here): the integer squared distance transform by equality, its square root bit for bit, the
weighted form within a few fp64 roundings, hole filling by equality; and the host side of van_gan_amd.postprocess: the argument checks,
which come before any device access, and the scratch arithmetic and refusals of the library entries, which launch nothing."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import edt_restate as R

CASES = [((9, 17, 70), 0.9), ((16, 9, 65), 0.999), ((1, 1, 1), 0.5), ((5, 1, 3), 0.7), ((3, 130, 67), 0.97), ((2, 2, 300), 0.99), ((12, 11, 10), 0.5)]


def _with_background(shape, p):
    m = R.bernoulli(shape, p)
    if m.all():
        m.ravel()[0] = 0                                             # scipy's result has no meaning without a background voxel
    return m


@pytest.mark.parametrize('shape,p', CASES)
def test_the_restatement_is_scipys_transform(shape, p):
    m = _with_background(shape, p)
    want = ndi.distance_transform_edt(m)
    got = R.edt_sq(m)
    assert got.dtype == np.int64 and np.array_equal(got, np.rint(want ** 2).astype(np.int64))
    assert np.array_equal(np.sqrt(got.astype(np.float64)), want)                    # bit for bit
    assert np.array_equal(R.edt(m), want.astype(np.float32))
    assert not got[m == 0].any() and (got[m != 0] >= 1).all()


def test_the_crafted_masks_against_scipy():
    for m in (R.one_background_corner((6, 7, 70)), R.background_plane((9, 17, 70)), R.tubes((16, 20, 24)), np.zeros((3, 4, 5), np.uint8)):
        assert np.array_equal(R.edt_sq(m), np.rint(ndi.distance_transform_edt(m) ** 2).astype(np.int64))
    far = R.edt_sq(R.one_background_corner((6, 7, 70)))
    assert far[5, 6, 69] == 25 + 36 + 69 * 69
    plane = R.background_plane((9, 17, 70))
    assert plane[:4].all() and plane[5:].all() and not plane[4].all()


def test_a_volume_without_background_is_the_sentinel():
    """The documented difference: scipy returns finite numbers without meaning there; the restatement (and the device) the sentinel."""
    ones = np.ones((3, 4, 5), np.uint8)
    assert (R.edt_sq(ones) == R.INF).all() and np.isposinf(R.edt(ones)).all() and np.isposinf(R.edt_weighted(ones, (2.0, 0.5, 1.25))).all()
    assert np.isfinite(ndi.distance_transform_edt(ones)).all()


@pytest.mark.parametrize('shape,p', CASES)
def test_the_weighted_restatement_is_scipys(shape, p):
    sampling = (2.0, 0.5, 1.25)
    m = _with_background(shape, p)
    want = ndi.distance_transform_edt(m, sampling=sampling)
    got = R.edt_weighted(m, sampling)
    assert got.dtype == np.float64 and np.all(np.abs(got - want) <= 4 * 2.0 ** -52 * np.abs(want))
    unit = R.edt_weighted(m, (1.0, 1.0, 1.0))
    assert np.array_equal(unit, np.sqrt(R.edt_sq(m).astype(np.float64)))            # weight 1: the integer form


def test_fill_holes_is_scipys():
    cases = dict(R.hole_cases())
    for shape, p in (((9, 17, 70), 0.5), ((12, 11, 10), 0.7), ((5, 1, 3), 0.5), ((1, 1, 1), 0.0), ((16, 9, 65), 0.85)):
        cases['bernoulli %s %s' % (shape, p)] = R.bernoulli(shape, p)
    for name, m in cases.items():
        want = ndi.binary_fill_holes(m).astype(np.uint8)
        assert np.array_equal(R.fill_holes(m), want), name
    filled = {name: int(R.fill_holes(m).sum() - m.sum()) for name, m in R.hole_cases().items()}
    assert filled['a closed box with a one-voxel cavity'] == 1
    assert filled['a cavity joined to the outside through an edge'] == 1 and filled['a cavity joined to the outside through a corner'] == 1
    assert filled['a cavity that touches a face'] == 0 and filled['a tube open at both ends'] == 0
    assert filled['a tube closed at both ends'] == 3 * 3 * 64
    assert filled['nested shells'] == 7 * 7 * 66 - 5 * 5 * 64 + 3 * 3 * 62 - 60       # both rings of background between the shells


def test_argument_checks_come_before_the_device():
    from van_gan_amd import postprocess as P
    mask = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for fn in (P.distance_transform_edt, P.fill_holes, P.vessel_radius):
        with pytest.raises(ValueError, match='on the device'):
            fn(mask)
        with pytest.raises(ValueError, match='on the device'):
            fn(mask.numpy())
        with pytest.raises(ValueError, match=r'\[X,Y,Z\]'):
            fn(mask[0])
        with pytest.raises(ValueError, match='must be'):
            fn(mask.to(torch.float32))
        with pytest.raises(ValueError, match='contiguous'):
            fn(mask.transpose(0, 2))
    for bad in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, float('nan'), 1.0), (1.0, float('inf'), 1.0), 'abc', 0.0, True,
                (1.0, None, 1.0)):
        with pytest.raises(ValueError, match='sampling'):
            P.distance_transform_edt(mask, bad)
        with pytest.raises(ValueError, match='sampling'):
            P.vessel_radius(mask, bad)
    with pytest.raises(ValueError, match='squared'):
        P.distance_transform_edt(mask, (1.0, 1.0, 1.0), squared=True)
    assert P._sampling(None) is None and P._sampling(2) == (2.0, 2.0, 2.0) and P._sampling(np.array([2.0, 0.5, 1.25])) == (2.0, 0.5, 1.25)
    # X^2 + Y^2 + Z^2 < 2^31, checked on a tensor without storage before its device is looked at
    long = torch.empty(46341, 1, 1, dtype=torch.uint8, device='meta')
    for fn in (P.distance_transform_edt, P.vessel_radius):
        with pytest.raises(ValueError, match=r'X\^2 \+ Y\^2 \+ Z\^2'):
            fn(long)
    with pytest.raises(ValueError, match='on the device'):
        P.distance_transform_edt(torch.empty(46340, 1, 1, dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError, match=r'2\^31'):
        P.distance_transform_edt(torch.empty(2 ** 11, 2 ** 10, 2 ** 10, dtype=torch.uint8, device='meta'))
    pred = torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match='on the device'):
        P.vessel_mask(pred, fill_holes=True)


def test_the_entries_refuse_on_the_host():
    import ctypes
    from van_gan_amd import _lib, build
    from van_gan_amd._lib import lib, lib_fp16
    for name, nargs in (('vg_edt_scratch_bytes', 4), ('vg_edt', 10), ('vg_fill_holes_mark', 6), ('vg_fill_holes_apply', 6)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(lib, name) and hasattr(lib_fp16(), name)
    assert 'vg_edt.hip' in build.SOURCES
    for shape in ((1, 1, 1), (9, 17, 70), (512, 512, 140), (46340, 1, 1), (1, 1, 46340), (26754, 26754, 3)):
        n = shape[0] * shape[1] * shape[2]
        assert lib.vg_edt_scratch_bytes(*shape, 0) == 2 * ((4 * n + 15) // 16 * 16) == lib_fp16().vg_edt_scratch_bytes(*shape, 0)
        assert lib.vg_edt_scratch_bytes(*shape, 1) == 2 * ((8 * n + 15) // 16 * 16)
    for shape in ((0, 1, 1), (1, -1, 1), (46341, 1, 1), (1, 1, 46341), (26755, 26755, 3), (2048, 1024, 1024), (32768, 32768, 2)):
        assert lib.vg_edt_scratch_bytes(*shape, 0) < 0 and lib.vg_edt_scratch_bytes(*shape, 1) < 0
    assert lib.vg_edt_scratch_bytes(4, 4, 4, 2) < 0
    fake = 1 << 20                                                 # non-NULL, aligned, never dereferenced: every call below is refused on the host
    big = 1 << 40
    s3 = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    assert lib.vg_edt(None, 4, 4, 4, None, None, 1, None, 0, None) == -1
    assert lib.vg_edt(fake, 46341, 1, 1, None, fake, 1, fake, big, None) == -1           # the overflow precondition
    assert lib.vg_edt(fake, 4, 4, 4, None, fake, 2, fake, big, None) == -1               # no such output
    assert lib.vg_edt(fake, 4, 4, 4, s3, fake, 0, fake, big, None) == -1                 # squared distances with a sampling
    assert lib.vg_edt(fake, 4, 4, 4, None, fake, 1, fake, 511, None) == -1               # scratch one byte short
    assert lib.vg_edt(fake, 4, 4, 4, s3, fake, 1, fake, 1023, None) == -1
    assert lib.vg_edt(fake, 4, 4, 4, None, fake + 2, 1, fake, big, None) == -1 and lib.vg_edt(fake, 4, 4, 4, None, fake, 1, fake + 8, big, None) == -1
    for bad in ((1.0, 0.0, 1.0), (-1.0, 1.0, 1.0), (1.0, 1.0, float('nan')), (float('inf'), 1.0, 1.0)):
        assert lib.vg_edt(fake, 4, 4, 4, (ctypes.c_double * 3)(*bad), fake, 1, fake, big, None) == -1
    assert lib.vg_fill_holes_mark(None, 4, 4, 4, None, None) == -1 and lib.vg_fill_holes_mark(fake, 4, 0, 4, fake, None) == -1
    assert lib.vg_fill_holes_mark(fake, 2048, 1024, 1024, fake, None) == -1 and lib.vg_fill_holes_mark(fake + 2, 4, 4, 4, fake, None) == -1
    assert lib.vg_fill_holes_apply(None, None, None, 8, None, None) == -1 and lib.vg_fill_holes_apply(fake, fake, fake, 0, fake, None) == -1
    assert lib.vg_fill_holes_apply(fake, fake, fake, 2 ** 31, fake, None) == -1 and lib.vg_fill_holes_apply(fake, fake + 2, fake, 8, fake, None) == -1
