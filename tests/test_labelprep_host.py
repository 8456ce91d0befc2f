"""CPU: the host side of the label-volume preprocessing -- the float32 restatement the GPU tests compare against
(tests/labelprep_restate.py) pinned to scipy.stats.mode and to a literal numpy transcription of the recipe, the new entries' declaration /
prototype / export in both libraries, their argument checks (which launch nothing), and the input validation of prepare_segmentation and
value_mode, which runs before any device access."""
import os
import re

import numpy as np
import pytest
import scipy.stats
import torch

import labelprep_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _two(n, seed):
    return np.where(np.random.default_rng(seed).random(n) < 0.3, F32(-1.5), F32(4.0)).astype(F32)


def _tied(n, seed):
    a = np.repeat(np.array([3.0, -7.5, 0.25], F32), n // 3)              # three values, equally frequent
    np.random.default_rng(seed).shuffle(a)
    return a


def _uint8(n, seed):
    return np.minimum(np.random.default_rng(seed).poisson(9.0, n), 255).astype(np.uint8).astype(F32) / F32(255)


def _distinct(n, seed):
    a = ((np.arange(n) - n // 2) * 0.25 + 0.125).astype(F32)
    np.random.default_rng(seed).shuffle(a)
    return a


def _normalised_collision(n, seed):
    x = R.collision_example()
    return (x - x.min()) / (x.max() - x.min())


MODE_CASES = {'two': _two, 'tied': _tied, 'uint8': _uint8, 'distinct': _distinct, 'collision': _normalised_collision}


@pytest.mark.parametrize('n', [3, 999, 30000])
@pytest.mark.parametrize('kind', list(MODE_CASES))
def test_restated_mode_is_scipys(kind, n):
    a = MODE_CASES[kind](n, n)
    assert a.dtype == F32
    want = scipy.stats.mode(a, axis=None)
    value, count = R.mode(a)
    assert value == np.ravel(want.mode)[0] and count == int(np.ravel(want.count)[0]), (kind, n, value, count, want)
    value3, count3 = R.mode(a.reshape(-1, 1, 1))                             # any shape: the flattened values
    assert (value3, count3) == (value, count)
    if kind == 'tied':
        assert value == F32(-7.5) and count == n // 3
    if kind == 'distinct':
        assert value == a.min() and count == 1


def test_ties_go_to_the_smallest_value_and_the_zeros_are_one_value():
    a = np.array([1.0] * 994 + [0.0] * 994, F32)
    assert R.mode(a) == (0.0, 994) and scipy.stats.mode(a, axis=None).mode == 0
    z = np.array([-0.0] * 3 + [0.0] * 3 + [1.0] * 5, F32)
    value, count = R.mode(z)
    assert value == 0 and count == 6 and not np.signbit(value)
    assert R.mode(np.array([np.nan, np.inf, 2.0, -np.inf], F32)) == (2.0, 1)


def test_collision_example_is_what_it_claims():
    x = R.collision_example()
    y, mn, mx = R.normalise(x)
    assert (mn, mx) == (-100.0, 200.0)
    assert int((y == 1).sum()) == 6 and int((x == mx).sum()) == 3             # the normalisation merged three neighbours into the maximum
    assert R.mode(x) == (7.0, 5)
    assert R.mode(y) == (1.0, 6)
    want = scipy.stats.mode(y, axis=None)
    assert np.ravel(want.mode)[0] == 1 and int(np.ravel(want.count)[0]) == 6
    assert scipy.stats.mode(x, axis=None).mode == 7
    r = R.label(x.reshape(2, 1, 7))
    assert r['inverted'] and r['mode'] == 1.0 and r['count'] == 6


def _literal(s):
    """Steps 2-5 as the reference's user would type them, scipy's mode included."""
    s = s.astype('float32')
    y = (s - s.min()) / (s.max() - s.min())
    if scipy.stats.mode(y, axis=None).mode == 1:
        y -= 1.
        y = abs(y)
    y = (y - 0.5) / 0.5
    y[y < 0.] = -1.0
    y[y >= 0.] = 1.0
    assert y.dtype == F32
    return y


def _label_volumes():
    rng = np.random.default_rng(11)
    shape = (17, 9, 13)
    yield 'fg10', np.where(rng.random(shape) < 0.1, 255, 0).astype(np.uint8)
    yield 'fg70', np.where(rng.random(shape) < 0.7, 255, 0).astype(np.uint8)
    yield 'multi', rng.choice(np.array([0, 255, 100, 17, 201], np.uint8), shape, p=[0.1, 0.25, 0.4, 0.15, 0.1])
    yield 'uint16', (rng.permutation(int(np.prod(shape))).reshape(shape) + 300).astype(np.uint16)
    yield 'negative', rng.choice(np.array([-3.5, -1.0, 2.25], F32), shape, p=[0.2, 0.35, 0.45])
    yield 'collision', R.collision_example().reshape(2, 1, 7)


@pytest.mark.parametrize('name,vol', list(_label_volumes()), ids=[n for n, _ in _label_volumes()])
def test_restated_recipe_is_the_literal_transcription(name, vol):
    r = R.label(vol)
    want = _literal(vol)
    assert r['out'].dtype == F32 and r['out'].tobytes() == want.tobytes()
    assert set(np.unique(r['out']).tolist()) <= {-1.0, 1.0}
    assert r['inverted'] == (name in ('fg70', 'negative', 'collision'))
    assert np.array_equal(R.label(vol[..., None])['out'], r['out'])
    if name == 'negative':                                                   # the clamp belongs to the resize alone: with it the answer differs
        assert not R.label(vol, resized=True)['inverted']
        assert (r['out'][vol == F32(2.25)] == -1).all() and (r['out'][vol != F32(2.25)] == 1).all()


def test_restated_recipe_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError) as e:
        R.label(np.full((3, 3, 3), 9, np.uint8))
    assert str(e.value) == R.MINMAX_ERROR
    v = np.zeros((3, 3, 3), F32)
    v[1, 1, 1] = np.nan
    with pytest.raises(ValueError, match='NaN detected'):
        R.label(v)
    assert np.array_equal(R.clamp(np.array([-3, 0, 17.5, 255, 300], F32)), np.array([0, 0, 17.5, 255, 255], F32))


# ------------------------------------------------------------------------------------------------ the C ABI
ENTRIES = (('vg_value_mode_scratch_bytes', 1), ('vg_value_mode', 7), ('vg_label_finish', 7))
PTR = 1 << 20                              # never dereferenced: every call below is rejected on its arguments


def _libs():
    from van_gan_amd._lib import lib, lib_fp16
    return [lib, lib_fp16()]


def test_entry_points_declared_prototyped_and_exported():
    from van_gan_amd import _lib, build, preprocess
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    for name, nargs in ENTRIES:
        assert re.search(r'^(?:int|int64_t)\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name)
    assert 'vg_labelprep.hip' in build.SOURCES
    slots = int(re.search(r'^#define VG_MODE_LDS_SLOTS (\d+)', hdr, flags=re.M).group(1))
    assert preprocess.MODE_LDS_SLOTS == slots and slots >= 512 and slots & (slots - 1) == 0      # 256 uint8 levels with room to spare
    import van_gan_amd
    assert callable(van_gan_amd.value_mode) and callable(van_gan_amd.prepare_segmentation)
    from van_gan_amd.data import DataPipeline
    assert callable(DataPipeline.from_raw)


def _mode(L, x=PTR, n=1000, mm=None, result=PTR, scratch=PTR, short=0):
    nbytes = L.vg_value_mode_scratch_bytes(1000)
    assert nbytes > 0
    return L.vg_value_mode(x, n, mm, result, scratch, nbytes - short, None)


@pytest.mark.parametrize('bad', [dict(x=None), dict(result=None), dict(scratch=None), dict(n=0), dict(n=2 ** 31), dict(x=PTR + 2), dict(mm=PTR + 1),
                                 dict(result=PTR + 2), dict(short=1), dict(scratch=PTR + 8)],
                         ids=['x=NULL', 'result=NULL', 'scratch=NULL', 'n=0', 'n=2^31', 'x+2', 'mm4+1', 'result+2', 'scratch-1', 'scratch+8'])
def test_value_mode_rejects_bad_arguments_without_a_gpu(bad):
    for L in _libs():
        assert _mode(L, **bad) == -1, bad


def _finish(L, x=PTR, n=1000, mm=PTR, result=PTR, out=PTR, state=PTR):
    return L.vg_label_finish(x, n, mm, result, out, state, None)


@pytest.mark.parametrize('bad', [dict(x=None), dict(mm=None), dict(result=None), dict(out=None), dict(state=None), dict(n=0), dict(n=2 ** 31),
                                 dict(x=PTR + 2), dict(out=PTR + 1), dict(mm=PTR + 2), dict(result=PTR + 3), dict(state=PTR + 2)],
                         ids=['x=NULL', 'mm4=NULL', 'result=NULL', 'out=NULL', 'state=NULL', 'n=0', 'n=2^31', 'x+2', 'out+1', 'mm4+2', 'result+3',
                              'state+2'])
def test_label_finish_rejects_bad_arguments_without_a_gpu(bad):
    for L in _libs():
        assert _finish(L, **bad) == -1, bad


def test_scratch_query_is_monotonic_and_covers_the_range():
    for L in _libs():
        assert L.vg_value_mode_scratch_bytes(0) == -1 and L.vg_value_mode_scratch_bytes(-5) == -1 and L.vg_value_mode_scratch_bytes(2 ** 31) == -1
        ns = [1, 2, 3, 63, 64, 65, 1000, 1024, 1025, 10 ** 6, 2 ** 24, 2 ** 24 + 1, 2 ** 30, 2 ** 31 - 1]
        sizes = [L.vg_value_mode_scratch_bytes(n) for n in ns]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert all(s >= 16 * n for s, n in zip(sizes, ns))                  # at least two slots of eight bytes per value: load <= 0.5
        assert sizes[-1] > 2 ** 32


def test_prepare_segmentation_validates_before_touching_the_device(monkeypatch):
    from van_gan_amd import preprocess

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(preprocess, '_resolve_device', no_device)
    for bad in (np.zeros((4, 4, 4, 1, 1), np.uint8), np.zeros((4, 4, 4), np.float64), torch.zeros(4, 4, 4, 1, 1), torch.zeros(4, 4, 4, dtype=torch.float64),
                np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4, 2), np.float32), np.zeros((4, 4, 4), np.int16), torch.zeros(4, 4, 4, dtype=torch.int16),
                np.zeros((4, 0, 4), np.uint8), [[[1.0]]]):
        with pytest.raises(ValueError):
            preprocess.prepare_segmentation(bad)
    vol = np.zeros((4, 4, 4), np.uint8)
    for target in ((4, 4), (0, 4, 4), (4, 4, 4.5), 'abc', 7, (4, 4, 4, 2), (4, 4, 2 ** 20 + 1)):
        with pytest.raises(ValueError):
            preprocess.prepare_segmentation(vol, target_size=target)
    for bad in (torch.zeros(8), np.zeros(8, np.float32), torch.zeros(8, dtype=torch.float64)):     # host tensors, a numpy array
        with pytest.raises(ValueError):
            preprocess.value_mode(bad)
