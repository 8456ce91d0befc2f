"""GPU: the imaging filters (csrc/vg_filters.hip; van_gan_amd.preprocess.median_filter, volume_moments, outlier_limits,
threshold_outliers) against the numpy restatement (tests/filters_restate.py, pinned to scipy / numpy by tests/test_filters_host.py), and
their place in prepare_imaging / segment_volume.

The median is a selection and the outlier limits are data values, so both are compared by equality.  The moments are held to 2^-23
relative to the float64 restatement, the bound of test_slice_moments_and_zscore for the same accumulation (fp64 sums, one rounding to
fp32 is 2^-24; the other half covers the fp64 accumulation error of at most n 2^-53 relative to sums that do not cancel, n < 2^29).
The median kernel's tile is 8 (y) x 32 (z) outputs marched over 32 planes of x: the shapes below cross every one of those edges."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filters_restate as FR  # noqa: E402
import gpu_helpers  # noqa: E402
from gpu_helpers import DEV, _dev, _raw, _Recorder  # noqa: E402

F32 = np.float32
DTYPES = ['uint8', 'uint16', 'float32']
SIZES = [(3, 3, 3), (3, 3, 1)]
MEDIAN_SHAPES = [(1, 1, 1), (2, 2, 2), (1, 7, 4), (3, 66, 2),
                 (35, 11, 37),             # no axis a multiple of the tile (32 planes, 8 rows, 32 columns), each crosses one tile edge
                 (5, 5, 65),               # two z tiles and one column: several workgroups along the contiguous axis
                 (40, 37, 70)]


@functools.lru_cache(maxsize=None)
def _volume(shape, dtype):
    rng = np.random.default_rng(sum((i + 3) * s for i, s in enumerate(shape)) + len(dtype))
    if dtype == 'uint8':                                                    # few distinct values: heavy ties
        v = rng.choice(np.array([0, 3, 200, 255], np.uint8), shape)
    elif dtype == 'uint16':
        v = rng.integers(0, 65536, shape).astype(np.uint16)
    else:
        v = rng.standard_normal(shape).astype(F32)
        v[rng.random(shape) < 0.05] = F32(-0.0)
        v[rng.random(shape) < 0.05] = F32(0.0)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _median_ref(shape, dtype, size):
    want = FR.median(_volume(shape, dtype).astype(F32), size)
    want.setflags(write=False)
    return want


# ------------------------------------------------------------------------------------------------ median
@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', MEDIAN_SHAPES)
def test_median_is_the_restatement(shape, dtype, size):
    from van_gan_amd.preprocess import median_filter
    v = _volume(shape, dtype)
    got_t, count = median_filter(v, size, return_count=True)
    assert got_t.is_cuda and got_t.dtype == torch.float32 and got_t.shape == shape
    got = got_t.cpu().numpy()
    assert np.array_equal(got, _median_ref(shape, dtype, size))
    assert int(count) == 0
    assert torch.equal(median_filter(v, size), got_t)                       # equal bits on a second call
    if v.dtype != np.uint16:
        xd = _dev(v)
        assert torch.equal(median_filter(xd, size), got_t) and np.array_equal(xd.cpu().numpy(), v)     # a device tensor; the input is unchanged


def test_median_int_size_trailing_axis_and_the_other_windows():
    from van_gan_amd.preprocess import median_filter
    v = _volume((35, 11, 37), 'float32')
    ref = median_filter(v, (3, 3, 3))
    assert torch.equal(median_filter(v, 3), ref) and torch.equal(median_filter(v[..., None], 3), ref)
    assert median_filter(v, 1).cpu().numpy().tobytes() == v.tobytes()       # a window of one voxel copies
    for size in [(1, 1, 3), (1, 3, 1), (3, 1, 1), (1, 3, 3), (3, 1, 3)]:
        assert np.array_equal(median_filter(v, size).cpu().numpy(), FR.median(v, size)), size


def test_median_of_an_unaligned_volume():
    from van_gan_amd.preprocess import RawVolume, median_filter
    v = _volume((35, 11, 37), 'float32')
    buf = _dev(np.concatenate([np.zeros(1, F32), v.ravel()]))[1:]
    assert buf.data_ptr() % 16 == 4
    assert np.array_equal(median_filter(RawVolume(buf, 2, v.shape), 3).cpu().numpy(), _median_ref((35, 11, 37), 'float32', (3, 3, 3)))


@pytest.mark.parametrize('size', SIZES)
def test_median_known_answers(size):
    from van_gan_amd.preprocess import median_filter
    hot = np.zeros((9, 10, 40), F32)
    hot[4, 5, 33] = 1e6
    hot[0, 0, 0] = -5.0                                                     # a corner is read at most 8 of 27 (4 of 9) times
    assert not median_filter(hot, size).cpu().numpy().any()
    x, y, z = np.meshgrid(np.arange(36), np.arange(10), np.arange(34), indexing='ij')
    ramp = (x + 100 * y + 10000 * z).astype(F32)                            # integers below 2^24: exact; the centre is the median of a symmetric window
    got = median_filter(ramp, size).cpu().numpy()
    assert np.array_equal(got[1:-1, 1:-1, 1:-1], ramp[1:-1, 1:-1, 1:-1])
    two = np.where(x + y >= 20, F32(7.5), F32(-2.0)).astype(F32)            # a planar interface: every window holds a majority of its centre's side
    got = median_filter(two, size).cpu().numpy()
    assert np.array_equal(got[1:-1, 1:-1, 1:-1], two[1:-1, 1:-1, 1:-1])


def test_median_counts_a_nan_and_check_raises():
    from van_gan_amd.preprocess import median_filter, prepare_imaging
    v = _volume((35, 11, 37), 'float32').copy()
    v[33, 9, 35] = np.nan
    for size in SIZES:
        out, count = median_filter(v, size, return_count=True)
        assert int(count) == 1
        far = np.ones(v.shape, bool)
        far[32:35, 8:11, 34:37] = False                                     # windows without the NaN are unaffected
        assert np.array_equal(out.cpu().numpy()[far], _median_ref((35, 11, 37), 'float32', size)[far])
    v[0, 0, 0] = np.inf
    assert int(median_filter(v, 3, return_count=True)[1]) == 2
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_imaging(v, preprocess='median')
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_imaging(v, preprocess=('median', 'rsom'))
    out = prepare_imaging(v, preprocess='median', check=False)
    assert out.shape == v.shape + (1,)
    torch.cuda.synchronize()


def test_median_raw_entry_rejects_aliasing():
    from van_gan_amd._lib import lib
    x = _dev(_volume((5, 5, 65), 'float32'))
    keep = x.clone()
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.vg_median3(x.data_ptr(), 2, 5, 5, 65, 3, 3, 3, x.data_ptr(), ctr.data_ptr(), None) == -1
    assert lib.vg_median3(x.data_ptr(), 2, 5, 5, 32, 3, 3, 1, x.data_ptr() + 4 * 400, ctr.data_ptr(), None) == -1      # out begins inside vol
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and int(ctr) == 0                           # nothing was launched


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 7), (37, 29, 23), (40, 37, 70)])
def test_volume_moments(shape, dtype):
    from van_gan_amd.preprocess import volume_moments
    v = _volume(shape, dtype)
    m64, s64, _, _ = FR.moments64(v)
    ms_t = volume_moments(v)
    assert ms_t.is_cuda and ms_t.dtype == torch.float32 and ms_t.shape == (2,)
    ms = ms_t.cpu().numpy().astype(np.float64)
    err = np.abs(ms - [m64, s64])
    print('%s %s: moments rel err %.3g, %.3g (bound %.3g)' % (shape, dtype, err[0] / max(abs(m64), 1e-300), err[1] / max(s64, 1e-300), 2.0 ** -23))
    assert err[0] <= 2.0 ** -23 * abs(m64) and err[1] <= 2.0 ** -23 * s64
    assert torch.equal(volume_moments(v), ms_t)                             # bitwise reproducible


def test_moments_of_a_constant_an_unaligned_volume_and_a_tail():
    from van_gan_amd.preprocess import RawVolume, volume_moments
    for c, dt in ((9, np.uint8), (30000, np.uint16), (-731.25, F32)):
        ms = volume_moments(np.full((13, 7, 5), c, dt)).cpu().numpy()
        assert ms[0] == F32(c) and ms[1] == 0.0
    v = _volume((37, 29, 23), 'float32')
    assert v.size % 4 == 3
    buf = _dev(np.concatenate([np.zeros(1, F32), v.ravel()]))[1:]
    assert buf.data_ptr() % 16 == 4
    a, b = volume_moments(RawVolume(buf, 2, v.shape)).cpu().numpy().astype(np.float64), volume_moments(v).cpu().numpy().astype(np.float64)
    m64, s64, _, _ = FR.moments64(v)
    for got in (a, b):                                                     # another order of summation: each within the bound
        assert abs(got[0] - m64) <= 2.0 ** -23 * abs(m64) and abs(got[1] - s64) <= 2.0 ** -23 * s64


# ------------------------------------------------------------------------------------------------ outlier limits
def _agreed_limits(x32, thr):
    """The precondition of the limits test, a condition on the inputs: the restated limits at the rounded float64 moments and at their
    eight neighbours one ulp away all agree -- then the device, whose moments lie within an ulp, must find exactly these."""
    nine = FR.limits_at_neighbours(x32, thr)
    assert all(r == nine[0] for r in nine), 'the volume does not satisfy the precondition: change the seed, not the rule'
    return nine[0]


@pytest.mark.parametrize('thr', [6, 2.5])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8', 'float32'])
def test_outlier_limits_are_the_restatements(dtype, thr):
    from van_gan_amd.preprocess import outlier_limits
    raw = FR.limit_volumes()[dtype]
    lo, hi, kept = _agreed_limits(raw.astype(F32), thr)
    limits, counts = outlier_limits(raw, thr)
    assert limits.is_cuda and limits.dtype == torch.float32 and limits.shape == (2,) and counts.dtype == torch.int32 and counts.shape == (2,)
    got = limits.cpu().numpy()
    print('%s thr %s: limits %r, kept %d of %d' % (dtype, thr, got.tolist(), int(counts[0]), raw.size))
    assert (got[0], got[1], int(counts[0]), int(counts[1])) == (lo, hi, kept, 0)
    assert kept < raw.size
    limits2, counts2 = outlier_limits(raw, thr)
    assert torch.equal(limits2, limits) and torch.equal(counts2, counts)


def test_outlier_limits_edge_cases():
    from van_gan_amd.preprocess import OUTLIERS_ERROR, RawVolume, outlier_limits, prepare_imaging, threshold_outliers
    const = np.full((16, 19, 7), 9, np.uint8)
    limits, counts = outlier_limits(const)
    assert limits.cpu().numpy().tolist() == [np.inf, -np.inf] and counts.cpu().numpy().tolist() == [0, 0]
    with pytest.raises(ValueError) as e:
        prepare_imaging(const, preprocess='outliers')
    assert str(e.value) == OUTLIERS_ERROR
    assert prepare_imaging(const, preprocess='outliers', check=False).shape == (16, 19, 7, 1)
    # one NaN: counted, never kept -- and it makes the moments NaN, so nothing is kept at all
    x = FR.limit_volumes()['float32'].copy()
    x[5, 6, 7] = np.nan
    limits, counts = outlier_limits(x)
    assert counts.cpu().numpy().tolist() == [0, 1] and limits.cpu().numpy().tolist() == [np.inf, -np.inf]
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_imaging(x, preprocess='outliers')
    assert threshold_outliers(x).shape == x.shape
    # a size that is no multiple of the workgroup's span (1024 elements with 16-byte loads) nor of 4, and a pointer that allows no 16-byte loads
    raw = FR.limit_volumes(seed=11, shape=(37, 29, 23))['float32']
    assert raw.size % 1024 != 0 and raw.size % 4 == 3
    want = _agreed_limits(raw, 6)
    for vol in (raw, RawVolume(_dev(np.concatenate([np.zeros(1, F32), raw.ravel()]))[1:], 2, raw.shape)):
        limits, counts = outlier_limits(vol)
        got = limits.cpu().numpy()
        assert (got[0], got[1], int(counts[0]), int(counts[1])) == want + (0,)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ threshold_outliers / prepare_imaging
@pytest.mark.parametrize('dtype', ['uint16', 'uint8', 'float32'])
def test_threshold_outliers_and_prepare_imaging_are_the_restatement_bitwise(dtype, monkeypatch):
    from van_gan_amd import preprocess
    raw = FR.limit_volumes()[dtype]
    x32 = raw.astype(F32)
    lo, hi, kept = _agreed_limits(x32, 6)
    want = FR.threshold_outliers(x32, 6)
    got = preprocess.threshold_outliers(raw)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == raw.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert want.min() == lo and want.max() == hi
    if dtype == 'float32':
        xd = _dev(raw)
        assert torch.equal(preprocess.threshold_outliers(xd), got) and np.array_equal(xd.cpu().numpy(), raw)       # the caller's tensor is not clipped
    seen, real = [], preprocess._state_block

    def keep(*a):
        seen.append(real(*a))
        return seen[-1]
    monkeypatch.setattr(preprocess, '_state_block', keep)
    out = preprocess.prepare_imaging(raw, preprocess='outliers')
    assert out.shape == raw.shape + (1,)
    assert out.cpu().numpy()[..., 0].tobytes() == FR.rescale(want, lo, hi).tobytes()
    assert float(out.min()) == -1.0 and float(out.max()) == 1.0
    host = seen[0].cpu().numpy()
    assert host[2:4].view(F32).tobytes() == np.array([lo, hi], F32).tobytes()      # the limits block check=True reads back
    assert int(host[0]) == 0 and int(host[4]) == kept and int(host[5]) == 0
    monkeypatch.undo()
    assert torch.equal(preprocess.prepare_imaging(raw, preprocess='outliers', check=False), out)
    assert torch.equal(preprocess.prepare_imaging(raw, preprocess=('outliers',), outlier_threshold=6.0), out)


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize('tgt', [None, (24, 20, 32)])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_stages_compose_left_to_right(dtype, tgt):
    from van_gan_amd.preprocess import median_filter, prepare_imaging, preprocess_rsom_images, threshold_outliers
    raw = _raw(dtype)
    for size in (3, (3, 3, 1)):
        got = prepare_imaging(raw, preprocess=('median', 'rsom'), median_size=size, target_size=tgt)
        assert torch.equal(got, prepare_imaging(median_filter(raw, size), preprocess='rsom', target_size=tgt))
    got = prepare_imaging(raw, preprocess=('outliers', 'median'), outlier_threshold=3, target_size=tgt)
    assert torch.equal(got, prepare_imaging(median_filter(threshold_outliers(raw, 3)), preprocess=None, target_size=tgt))
    assert got.shape == (tgt or raw.shape) + (1,) and float(got.min()) == -1.0 and float(got.max()) == 1.0
    got = prepare_imaging(raw, preprocess=['median', 'outliers'], outlier_threshold=3, target_size=tgt)
    assert torch.equal(got, prepare_imaging(median_filter(raw), preprocess='outliers', outlier_threshold=3, target_size=tgt))
    got = prepare_imaging(raw, preprocess=('rsom', 'median'), target_size=tgt)
    assert torch.equal(got, prepare_imaging(median_filter(preprocess_rsom_images(raw)), preprocess=None, target_size=tgt))


_engine = functools.lru_cache(maxsize=None)(gpu_helpers._engine)           # one engine per test module, as before


def test_segment_volume_passes_the_stages_through(monkeypatch):
    """segment_volume(gen, raw, size, preprocess=..., median_size=...) hands stitch_subvolumes exactly the tensor prepare_imaging returns
    for the same keywords, and returns what the stitch returns (one run of the stitch: two runs differ in their last bits, see
    tests/test_gpu_preproc.py)."""
    from van_gan_amd.preprocess import prepare_imaging
    eng = _engine()
    raw = _raw('uint8', (48, 40, 36))
    stitch, seen = eng.stitch_subvolumes, []

    def recording(gen, img, subvol_size=None, **kw):
        out = stitch(gen, img, subvol_size, **kw)
        seen.append((gen, img, subvol_size, kw, out))
        return out
    monkeypatch.setattr(eng, 'stitch_subvolumes', recording)
    got = eng.segment_volume('gen_IS', raw, (32, 32, 32), preprocess=('median', 'rsom'), median_size=(3, 3, 1), stride=(8, 8, 4))
    assert len(seen) == 1
    gen, img, subvol_size, kw, out = seen[0]
    assert gen == 'gen_IS' and subvol_size == (32, 32, 32) and kw == dict(stride=(8, 8, 4)) and got is out
    want = prepare_imaging(raw, preprocess=('median', 'rsom'), median_size=(3, 3, 1))
    assert img.shape == (48, 40, 36, 1) and torch.equal(img, want)
    assert not torch.equal(img, prepare_imaging(raw, preprocess=('median', 'rsom')))                 # the size did arrive
    assert got.shape == (48, 40, 36, 1) and bool(torch.isfinite(got).all())
    eng.segment_volume('gen_IS', raw, (32, 32, 32), preprocess='outliers', outlier_threshold=2.5, check=False, stride=(16, 16, 16), complete=False)
    assert torch.equal(seen[1][1], prepare_imaging(raw, preprocess='outliers', outlier_threshold=2.5))


# ------------------------------------------------------------------------------------------------ fusion and unchanged launches
def _calls(monkeypatch, raw, **kw):
    from van_gan_amd import preprocess
    rec = _Recorder(preprocess.lib)
    monkeypatch.setattr(preprocess, 'lib', rec)
    try:
        preprocess.prepare_imaging(raw, **kw)
    finally:
        monkeypatch.undo()
    return rec.names


RSOM_CALLS = ['vg_slice_moments_scratch_bytes', 'vg_slice_moments', 'vg_zscore_slices', 'vg_order_stats_scratch_bytes', 'vg_order_stats', 'vg_clip_rescale']
NONE_CALLS = ['vg_zscore_slices', 'vg_minmax', 'vg_clip_rescale']
RESIZE_Z = ['vg_resample_axis']
OUTLIER_HEAD = ['vg_volume_moments_scratch_bytes', 'vg_volume_moments', 'vg_outlier_limits']


def test_fusion_and_the_launches_of_every_recipe(monkeypatch):
    u8, f32 = _raw('uint8'), _raw('uint16').astype(F32)
    # what the parent commit's prepare_imaging calls, read off its code: the same here
    assert _calls(monkeypatch, u8, preprocess='rsom') == RSOM_CALLS
    assert _calls(monkeypatch, u8) == RSOM_CALLS
    assert _calls(monkeypatch, u8, preprocess=None) == NONE_CALLS
    assert _calls(monkeypatch, u8, preprocess='rsom', target_size=(24, 20, 32)) == RSOM_CALLS + RESIZE_Z + ['vg_minmax', 'vg_clip_rescale']
    assert _calls(monkeypatch, u8, preprocess=None, target_size=(24, 20, 32)) == ['vg_zscore_slices'] + RESIZE_Z + ['vg_minmax', 'vg_clip_rescale']
    # 'outliers' last and no resize: its clip carries the rescale -- one vg_clip_rescale, no vg_minmax (an integer stack is converted first)
    assert _calls(monkeypatch, f32, preprocess='outliers') == OUTLIER_HEAD + ['vg_clip_rescale']
    assert _calls(monkeypatch, u8, preprocess='outliers') == OUTLIER_HEAD + ['vg_zscore_slices', 'vg_clip_rescale']
    assert _calls(monkeypatch, f32, preprocess='outliers', target_size=(24, 20, 32)) == OUTLIER_HEAD + ['vg_clip_rescale'] + RESIZE_Z + ['vg_minmax', 'vg_clip_rescale']
    # 'median' has no limits of its own: a min / max pass and one vg_clip_rescale
    assert _calls(monkeypatch, u8, preprocess='median') == ['vg_median3', 'vg_minmax', 'vg_clip_rescale']
    assert _calls(monkeypatch, u8, preprocess=('median', 'rsom')) == ['vg_median3'] + RSOM_CALLS
    assert _calls(monkeypatch, u8, preprocess=('outliers', 'median')) == OUTLIER_HEAD + ['vg_zscore_slices', 'vg_clip_rescale', 'vg_median3', 'vg_minmax', 'vg_clip_rescale']
    assert _calls(monkeypatch, u8, preprocess=('median', 'outliers')) == ['vg_median3'] + OUTLIER_HEAD + ['vg_clip_rescale']


def test_unchecked_calls_do_not_depend_on_the_data(monkeypatch):
    a = _raw('uint8')
    b = np.full(a.shape, 9, np.uint8)                                       # constant: no voxel is kept, the limits coincide
    c = _raw('uint8').astype(F32)
    c[1, 2, 3] = np.nan
    for pre in ('median', 'outliers', ('median', 'rsom'), ('outliers', 'median', 'rsom')):
        ref = _calls(monkeypatch, a.astype(F32), preprocess=pre, check=False)
        assert _calls(monkeypatch, b.astype(F32), preprocess=pre, check=False) == ref
        assert _calls(monkeypatch, c, preprocess=pre, check=False) == ref
        assert _calls(monkeypatch, a.astype(F32), preprocess=pre, check=True) == ref
    torch.cuda.synchronize()
