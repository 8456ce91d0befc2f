"""GPU: the label-volume preprocessing (csrc/vg_labelprep.hip; van_gan_amd.preprocess.value_mode / prepare_segmentation;
DataPipeline.from_raw) against the float32 numpy restatement (tests/labelprep_restate.py).  Every comparison is exact: values and counts
by equality, volumes bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import labelprep_restate as R  # noqa: E402
from gpu_helpers import DEV, _dev, _Recorder  # noqa: E402

F32 = np.float32


def _bits(words):
    return np.array(words, np.uint32).view(F32)


def _result4(x, mm=None):
    """The four result words of vg_value_mode on the host."""
    from van_gan_amd import preprocess
    result = torch.empty(4, dtype=torch.int32, device=x.device)
    preprocess._value_mode_into(x, None if mm is None else mm.data_ptr(), result)
    return result.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ value_mode
SIZES = [1, 2, 63, 64, 65, 1000003]


def _slots():
    from van_gan_amd.preprocess import MODE_LDS_SLOTS
    return MODE_LDS_SLOTS


def _tie(n, rng):
    """Two values n // 2 times each; an odd n adds one value that occurs once."""
    a = np.concatenate([np.full(n // 2, 3.0, F32), np.full(n // 2, -7.5, F32), np.full(n % 2, 100.0, F32)])
    rng.shuffle(a)
    return a


def _overflow(n, rng):
    """4 * MODE_LDS_SLOTS + 3 distinct values, each 1 to 3 times: more distinct values per workgroup than its combiner holds."""
    v = ((np.arange(4 * _slots() + 3) - 2000) * 0.375 + 0.0625).astype(F32)
    a = np.repeat(v, rng.integers(1, 4, v.size))
    rng.shuffle(a)
    return a


def _weak_hash(n, rng):
    """Keys that differ in one middle mantissa byte only, and keys that differ in the exponent only (the powers of two)."""
    v = np.concatenate([_bits(0x3F800000 | (np.arange(256, dtype=np.uint32) << 8)), _bits(np.arange(1, 255, dtype=np.uint32) << 23)])
    a = np.repeat(v, rng.integers(1, 6, v.size))
    rng.shuffle(a)
    return a


KINDS = {
    'equal': lambda n, rng: np.full(n, -2.75, F32),
    'two': lambda n, rng: np.where(rng.random(n) < 0.3, F32(-1.5), F32(4.0)).astype(F32),
    'tie': _tie,
    'uint8': lambda n, rng: np.minimum(rng.poisson(9.0, n), 255).astype(np.uint8).astype(F32),
    'distinct': lambda n, rng: rng.permutation(((np.arange(n) - n // 2) * 0.25 + 0.125).astype(F32)),
    'overflow': _overflow,
    'weak-hash': _weak_hash,
    'zeros': lambda n, rng: np.array([-0.0] * 3 + [0.0] * 3 + [1.0] * 5, F32),
}
FIXED = ('overflow', 'weak-hash', 'zeros')                                  # kinds that bring their own size
MODE_CASES = [(k, n) for k in KINDS if k not in FIXED for n in SIZES if not (k == 'tie' and n == 1)] + [(k, 0) for k in FIXED]


@functools.lru_cache(maxsize=None)
def _mode_data(kind, n):
    a = KINDS[kind](n, np.random.default_rng(n + len(kind)))
    assert a.dtype == F32 and (n == 0 or a.size == n)
    a.setflags(write=False)
    return a, R.mode(a)


@pytest.mark.parametrize('kind,n', MODE_CASES, ids=['%s-%d' % c for c in MODE_CASES])
def test_value_mode_is_exact(kind, n):
    from van_gan_amd.preprocess import value_mode
    a, (want, want_count) = _mode_data(kind, n)
    x = _dev(a)
    before = x.clone()
    value, count = value_mode(x)
    assert value.is_cuda and value.dtype == torch.float32 and value.shape == (1,) and count.is_cuda and count.shape == (1,)
    got, got_count = value.cpu().numpy()[0], int(count.cpu()[0])
    print('%s n=%d: mode %r x %d (restatement %r x %d)' % (kind, a.size, got, got_count, want, want_count))
    assert got == want and got_count == want_count
    assert torch.equal(x, before)
    first, again = _result4(x), _result4(x)
    assert first.tobytes() == again.tobytes()                               # all four words, run to run
    assert first[0] == np.array([got], F32).view(np.uint32)[0] and first[1] == got_count and first[2] == 0 and first[3] == 0
    x2 = _dev(np.concatenate([np.zeros(1, F32), a]))[1:]                    # a pointer that is 4- but not 16-byte aligned: the scalar kernel
    assert x2.data_ptr() % 16 == 4
    assert _result4(x2).tobytes() == first.tobytes()
    if kind == 'tie':
        assert got == F32(-7.5) and got_count == a.size // 2
    if kind == 'distinct':
        assert got == a.min() and got_count == 1
    if kind == 'zeros':
        assert got == 0 and got_count == 6 and first[0] == 0                # +0.0
    if kind == 'overflow':
        assert np.unique(a).size == 4 * _slots() + 3


def test_value_mode_counts_non_finite_values_and_never_inserts_them():
    rng = np.random.default_rng(4)
    a = np.where(rng.random(5000) < 0.4, F32(2.5), F32(-3.0)).astype(F32)
    a[[7, 1900, 4999]] = [np.nan, np.inf, -np.inf]
    a[100:104] = _bits([0xFFFFFFFF, 0x7FC00000, 0xFFC00001, 0x7F800001])    # NaN patterns, the all-ones one among them
    want, want_count = R.mode(a)
    for x in (_dev(a), _dev(np.concatenate([np.zeros(1, F32), a]))[1:]):
        r = _result4(x)
        assert r[:1].view(F32)[0] == want and r[1] == want_count and r[2] == 0 and r[3] == 7
    r = _result4(_dev(np.full(300, np.nan, F32)))                          # nothing finite: count 0, a NaN, 300 refused
    assert r[1] == 0 and np.isnan(r[:1].view(F32)[0]) and r[2] == 0 and r[3] == 300


def test_normalised_counting_sees_the_collision():
    """The collision example padded to a few thousand values that occur once: the raw mode is 7 (five times); counted as
    (x - min) / (max - min), six values are exactly 1.0 and that is the mode -- only through the collision."""
    from van_gan_amd import ops
    from van_gan_amd.preprocess import value_mode
    x = np.concatenate([R.collision_example(), (np.arange(3000) * 0.05 - 90.013).astype(F32)])
    np.random.default_rng(2).shuffle(x)
    y, mn, mx = R.normalise(x)
    assert R.mode(x) == (7.0, 5) and R.mode(y) == (1.0, 6) and int((x == mx).sum()) == 3
    xd = _dev(x)
    mm = torch.zeros(1, 4, device=DEV)
    ops.minmax(xd, 1, x.size, mm)
    r = _result4(xd, mm)
    assert r[:1].view(F32)[0] == 1.0 and r[1] == 6 and r[2] == 0 and r[3] == 0
    assert r.tobytes() == _result4(xd, mm).tobytes()
    value, count = value_mode(xd)
    assert float(value.cpu()[0]) == 7.0 and int(count.cpu()[0]) == 5
    const = _dev(np.full(100, 3.0, F32))                                    # min == max while normalising: reported in the status word
    ops.minmax(const, 1, 100, mm)
    assert _result4(const, mm)[2] != 0


# ------------------------------------------------------------------------------------------------ prepare_segmentation
SHAPES = [(17, 9, 13), (33, 20, 64)]


def _fg(shape, rng, frac):
    return np.where(rng.random(shape) < frac, 255, 0).astype(np.uint8)


def _exact_tie(shape, rng):
    n = int(np.prod(shape))
    a = np.concatenate([np.zeros(n // 2, np.uint8), np.full(n // 2, 255, np.uint8), np.full(n % 2, 128, np.uint8)])
    return rng.permutation(a).reshape(shape)


LABELS = {
    'fg10': lambda s, rng: _fg(s, rng, 0.1),
    'fg70': lambda s, rng: _fg(s, rng, 0.7),
    'tie': _exact_tie,
    'multi': lambda s, rng: rng.choice(np.array([0, 255, 100, 17, 201], np.uint8), s, p=[0.1, 0.25, 0.4, 0.15, 0.1]),
    'uint16-distinct': lambda s, rng: (rng.permutation(int(np.prod(s))).reshape(s) + 300).astype(np.uint16),
    'f32-negative': lambda s, rng: rng.choice(np.array([-3.5, -1.0, 2.25], F32), s, p=[0.2, 0.35, 0.45]),
}
INVERTED = {'fg10': False, 'fg70': True, 'tie': False, 'multi': False, 'uint16-distinct': False, 'f32-negative': True}


@functools.lru_cache(maxsize=None)
def _label_case(name, shape):
    v = LABELS[name](shape, np.random.default_rng(sum(shape) + len(name)))
    v.setflags(write=False)
    return v, R.label(v)


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize('name', list(LABELS))
def test_prepare_segmentation_matches_the_restatement(name, shape):
    from van_gan_amd.preprocess import prepare_segmentation
    v, ref = _label_case(name, shape)
    assert ref['inverted'] == INVERTED[name]
    out_t, info = prepare_segmentation(v, return_info=True)
    assert out_t.is_cuda and out_t.dtype == torch.float32 and out_t.shape == shape + (1,)
    out = out_t.cpu().numpy()[..., 0]
    assert out.tobytes() == ref['out'].tobytes()
    assert info == {k: ref[k] for k in ('inverted', 'mode', 'count', 'min', 'max')}, (info, ref)
    if name == 'fg70':
        assert (out[v == 255] == -1).all() and (out[v == 0] == 1).all()
    if name == 'fg10':
        assert (out[v == 255] == 1).all() and (out[v == 0] == -1).all()
    if name == 'multi':
        assert int((v == 255).sum()) > int((v == 0).sum()) and info['mode'] == float(F32(100) / F32(255))
    if name == 'tie':
        assert int((v == 255).sum()) == int((v == 0).sum()) and info['mode'] == 0.0
    if name == 'uint16-distinct':
        assert info['count'] == 1 and info['mode'] == 0.0
    if name == 'f32-negative':                                              # no clamp without a resize: with it the volume would not be inverted
        assert not R.label(v, resized=True)['inverted'] and info['min'] == -3.5
    assert torch.equal(prepare_segmentation(v[..., None]), out_t)           # [X,Y,Z,1]
    assert torch.equal(prepare_segmentation(v, check=False), out_t)
    if v.dtype != np.uint16:                                                # a device tensor is taken as it is and left as it is
        vd = _dev(v)
        keep = vd.clone()
        assert torch.equal(prepare_segmentation(vd), out_t) and torch.equal(vd, keep)


def test_target_size_resizes_clamps_and_then_binarises():
    from van_gan_amd.preprocess import prepare_segmentation, resize_volume
    v = _fg((20, 20, 12), np.random.default_rng(6), 0.7)
    target = (32, 32, 16)
    resized = resize_volume(v, target).cpu().numpy()                        # the device's own Lanczos-4 output: the restatement starts from it
    assert resized.shape == target and resized.dtype == F32
    assert (resized < 0).any() or (resized > 255).any()                     # the filter overshoots: the clamp has something to do
    ref = R.label(resized, resized=True)
    out_t, info = prepare_segmentation(v, target_size=target, return_info=True)
    assert out_t.shape == target + (1,) and out_t.cpu().numpy()[..., 0].tobytes() == ref['out'].tobytes()
    assert info == {k: ref[k] for k in ('inverted', 'mode', 'count', 'min', 'max')} and info['inverted'] and (info['min'], info['max']) == (0.0, 255.0)
    assert torch.equal(prepare_segmentation(v, target_size=target, check=False), out_t)
    assert torch.equal(prepare_segmentation(v, target_size=(20, 20, 12)), prepare_segmentation(v))      # nothing to resize: today's bits
    assert torch.equal(prepare_segmentation(v, target_size=(20, 20, 12, 1)), prepare_segmentation(v))


def test_check_raises_on_a_constant_volume_and_on_a_nan():
    from van_gan_amd.preprocess import MINMAX_ERROR, prepare_segmentation
    const = np.full((16, 19, 7), 9, np.uint8)
    with pytest.raises(ValueError) as e:
        prepare_segmentation(const)
    assert str(e.value) == MINMAX_ERROR == R.MINMAX_ERROR
    v = np.where(np.random.default_rng(1).random((16, 19, 7)) < 0.3, F32(1), F32(0)).astype(F32)
    v[3, 4, 5] = np.nan
    with pytest.raises(ValueError, match='NaN detected'):
        prepare_segmentation(v)
    for bad in (const, v):
        out = prepare_segmentation(bad, check=False)                        # returns; whatever it holds, the device is fine afterwards
        assert isinstance(out, torch.Tensor) and out.shape == (16, 19, 7, 1)
        torch.cuda.synchronize()


def test_unchecked_call_makes_the_same_calls_whatever_the_data(monkeypatch):
    from van_gan_amd import preprocess
    calls = []
    for name in ('fg10', 'fg70', 'multi'):
        rec = _Recorder(preprocess.lib)
        monkeypatch.setattr(preprocess, 'lib', rec)
        preprocess.prepare_segmentation(_label_case(name, SHAPES[0])[0], check=False)
        monkeypatch.undo()
        calls.append(rec.names)
    assert calls[0] == calls[1] == calls[2]
    assert [n for n in calls[0] if not n.endswith('_scratch_bytes')] == ['vg_zscore_slices', 'vg_minmax', 'vg_value_mode', 'vg_label_finish']


# ------------------------------------------------------------------------------------------------ DataPipeline.from_raw
def test_from_raw_prepares_both_domains():
    from van_gan_amd.data import DataPipeline
    from van_gan_amd.preprocess import prepare_imaging, prepare_segmentation
    rng = np.random.default_rng(9)
    imaging = [np.minimum(rng.poisson(30.0, s), 255).astype(np.uint8) for s in ((40, 36, 34), (36, 40, 33))]
    labels = [_fg((40, 36, 34), rng, 0.2), _fg((34, 36, 40), rng, 0.75)]     # bright vessels on dark, and the inverted convention
    pipe = DataPipeline.from_raw(imaging, labels, (32, 32, 32), 2, seed=3)
    assert len(pipe.imaging) == 2 and len(pipe.segmentation) == 2 and pipe.patch == (32, 32, 32) and pipe.B == 2 and pipe.otf
    for got, raw in zip(pipe.imaging, imaging):
        assert torch.equal(got, prepare_imaging(raw))
    for got, raw in zip(pipe.segmentation, labels):
        assert torch.equal(got, prepare_segmentation(raw)) and got.shape == raw.shape + (1,)
    plain = DataPipeline.from_raw(imaging, labels, (32, 32, 32), 2, seed=3, otf_imaging=False, imaging_kw=dict(preprocess=None),
                                  segmentation_kw=dict(check=False))
    assert not plain.otf and torch.equal(plain.imaging[0], prepare_imaging(imaging[0], preprocess=None))
    assert torch.equal(plain.segmentation[1], pipe.segmentation[1])
    real_i, real_s = pipe.next_batch()
    assert real_i.shape == (2, 32, 32, 32, 1) and real_s.shape == (2, 32, 32, 32, 1)
    s = real_s.cpu().numpy()
    assert set(np.unique(s).tolist()) <= {-1.0, 1.0} and s.max() >= 0.8
    assert float(real_i.min()) == -1.0 and float(real_i.max()) == 1.0
