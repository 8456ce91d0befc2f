"""CPU: the host side of the Lanczos-4 volume resize -- the filter table of van_gan_amd.preprocess.lanczos4_table and the restatement the
GPU tests compare against (tests/lanczos_restate.py) on known answers, against each other and against the analytic kernel
sinc(u) sinc(u / 4); vg_resample_axis's argument checks (which launch nothing) in both libraries; and the validation of target_size, which
runs before any device access.  The known answers were computed on a CPU from the filter's definition, not with OpenCV."""
import numpy as np
import pytest
import torch

import lanczos_restate as R

F32 = np.float32
W_HALF = [-0.01263015, 0.05976409, -0.16601135, 0.6188774, 0.6188774, -0.16601135, 0.05976409, -0.01263015]
W_35_64 = [-0.01107666, 0.05605678, -0.15666988, 0.55688393, 0.6786794, -0.17220172, 0.06229549, -0.01396742]
UNIT = [0, 0, 0, 1, 0, 0, 0, 0]


def _tables(L, T):
    from van_gan_amd.preprocess import lanczos4_table
    lib, res = lanczos4_table(L, T), R.table(L, T)
    for first, w8 in (lib, res):
        assert first.dtype == np.int32 and first.shape == (T,) and w8.dtype == F32 and w8.shape == (T, 8)
    assert np.array_equal(lib[0], res[0]) and lib[1].tobytes() == res[1].tobytes()           # the two tables: exactly equal
    return lib, res


def test_known_answers():
    from van_gan_amd.preprocess import lanczos4_weights
    for tabs in _tables(140, 128):
        first, w8 = tabs
        sx = first + 3
        t = np.array([F32((dx + 0.5) * (1.0 / (128 / 140)) - 0.5) for dx in range(128)], F32) - sx.astype(F32)
        assert list(sx[:5]) == [0, 1, 2, 3, 4] and list(sx[-5:]) == [134, 135, 136, 137, 138]
        assert list(t[:5]) == [0.046875, 0.140625, 0.234375, 0.328125, 0.421875]
        assert first.min() == -3 and first.max() + 7 == 142                              # the tap index range before clamping
        assert t[16] == 0.546875 and np.abs(w8[16] - np.array(W_35_64)).max() <= 1e-7
    for first, w8 in _tables(4, 8):
        assert list(first + 3) == [-1, 0, 0, 1, 1, 2, 2, 3]
        assert w8[0].tobytes() == R.weights(0.75).tobytes() and w8[1].tobytes() == R.weights(0.25).tobytes()
        assert all(w8[j].tobytes() == w8[j % 2].tobytes() for j in range(8))             # t alternates 0.75 / 0.25
    for first, w8 in _tables(2, 1):                                                      # fx = 0.5: sx = 0, t = 0.5
        assert list(first) == [-3] and np.abs(w8[0] - np.array(W_HALF)).max() <= 1e-7
    for first, w8 in _tables(5, 5) + _tables(1, 1):                                      # equal lengths: t = 0 everywhere, the unit tap
        assert np.array_equal(first + 3, np.arange(len(first))) and (w8 == np.array(UNIT, F32)).all()
    for fn in (lanczos4_weights, R.weights):
        assert np.abs(fn(0.5) - np.array(W_HALF)).max() <= 1e-7 and np.abs(fn(0.546875) - np.array(W_35_64)).max() <= 1e-7
        assert list(fn(0.0)) == UNIT and list(fn(F32(2.0 ** -24))) == UNIT and list(fn(F32(2.0 ** -23))) != UNIT      # t < FLT_EPSILON
        assert fn(0.25).dtype == F32


PHASES = (np.arange(1, 997) / 997.0).astype(F32)


def test_coefficients_against_the_analytic_kernel():
    """sinc(u) sinc(u / 4) at u = t + 3 - k, normalised in float64; 5e-7 is a few float32 roundings of numbers <= 0.68 (the coefficient, the
    sum of eight, the reciprocal, the product).  Measured over these 996 phases: 1.9e-7."""
    from van_gan_amd.preprocess import lanczos4_weights
    worst, l1 = 0.0, 0.0
    for t in PHASES:
        u = float(t) + 3 - np.arange(8)
        a = np.sinc(u) * np.sinc(u / 4)
        a /= a.sum()
        w, r = lanczos4_weights(t), R.weights(t)
        assert w.tobytes() == r.tobytes()
        worst = max(worst, np.abs(w.astype(np.float64) - a).max())
        l1 = max(l1, float(np.abs(w.astype(np.float64)).sum()))
        assert abs(w.astype(np.float64).sum() - 1.0) <= 4 * 2.0 ** -24
    print('max |w - analytic| over %d phases: %.3g; max sum |w|: %.5f' % (len(PHASES), worst, l1))
    assert worst <= 5e-7
    assert abs(l1 - 1.7146) <= 1e-4


@pytest.mark.parametrize('L,T', [(140, 128), (128, 140), (4, 8), (300, 17), (1031, 1000), (7, 7)])
def test_rows_sum_to_one_and_zero_phases_are_unit_taps(L, T):
    (first, w8), _ = _tables(L, T)
    assert (np.abs(w8.astype(np.float64).sum(axis=1) - 1.0) <= 4 * 2.0 ** -24).all()
    _, t = R.phases(L, T)
    zero = t < 2.0 ** -23
    assert (w8[zero] == np.array(UNIT, F32)).all() and (zero.any() or L != T)
    assert not w8.flags.writeable and not first.flags.writeable


PTR = 1 << 20                              # never dereferenced: every call below is rejected on its arguments


def _call(L_, x=PTR, outer=3, L=140, inner=5, T=128, first=PTR + 4096, w8=PTR + 8192, out=PTR + (1 << 16)):
    return L_.vg_resample_axis(x, outer, L, inner, T, first, w8, out, None)


BAD = [dict(x=None), dict(first=None), dict(w8=None), dict(out=None), dict(outer=0), dict(inner=0), dict(L=0), dict(T=0), dict(outer=-1),
       dict(L=2 ** 20 + 1), dict(T=2 ** 20 + 1), dict(outer=2 ** 20, L=2 ** 10, T=1, inner=2 ** 10), dict(outer=2 ** 30, L=1, T=2 ** 10, inner=1),
       dict(outer=2 ** 40, L=1, T=1, inner=1), dict(outer=1, L=1, T=1, inner=2 ** 40), dict(out=PTR), dict(x=PTR + 2), dict(out=PTR + 1)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join('%s=%s' % kv for kv in b.items()) for b in BAD])
def test_resample_axis_rejects_bad_arguments_without_a_gpu(bad):
    from van_gan_amd import _lib, build
    assert 'vg_resample.hip' in build.SOURCES and 'vg_resample_axis' in _lib.EXPORTS and len(_lib._SIGS['vg_resample_axis'][0]) == 9
    for L_ in (_lib.lib, _lib.lib_fp16()):
        assert _call(L_, **bad) == -1, bad


def test_target_size_is_validated_before_the_device_is_touched(monkeypatch):
    import van_gan_amd
    from van_gan_amd import preprocess

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(preprocess, '_resolve_device', no_device)
    vol = np.zeros((4, 4, 4), np.uint8)
    for bad in ((4, 4), (4, 4, 4, 4), (4, 4, 4, 2), (4, 0, 4), (4, -1, 4), (4, 4.5, 4), (4.0, 4, 4), 4, 'abc', (2 ** 20 + 1, 4, 4), None):
        with pytest.raises(ValueError):
            preprocess.resize_volume(vol, bad)
        if bad is not None:
            with pytest.raises(ValueError):
                preprocess.prepare_imaging(vol, target_size=bad)
    for ok in ((3, 5, 2), [3, 5, 2, 1], np.array([3, 5, 2]), torch.Size([3, 5, 2])):
        with pytest.raises(AssertionError, match='the device was touched'):             # past the validation
            preprocess.resize_volume(vol, ok)
        with pytest.raises(AssertionError, match='the device was touched'):
            preprocess.prepare_imaging(vol, target_size=ok)
    with pytest.raises(ValueError):
        preprocess.resize_volume(np.zeros((4, 4), np.uint8), (4, 4, 4))                  # a bad volume, as everywhere
    for bad in ((0, 5), (5, 0), (2 ** 20 + 1, 5), (5, 2 ** 20 + 1), (2.5, 5)):
        with pytest.raises((ValueError, TypeError)):
            preprocess.lanczos4_table(*bad)
    with pytest.raises(ValueError):
        preprocess.resample_axis(torch.zeros(2, 3, 4), 5)                               # a host tensor
    assert callable(van_gan_amd.resize_volume) and callable(van_gan_amd.lanczos4_table)
    import inspect
    assert 'target_size' in inspect.signature(van_gan_amd.VanGan.segment_volume).parameters
