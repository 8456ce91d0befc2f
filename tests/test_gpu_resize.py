"""GPU: the Lanczos-4 volume resize (csrc/vg_resample.hip, van_gan_amd.preprocess.resize_volume) against the float64 numpy restatement
(tests/lanczos_restate.py), and its place in prepare_imaging / segment_volume.

Tolerance, derived: a pass computes an 8-term dot product as one product and seven fmaf, whose error is at most gamma_8 <= 8.000004 * 2^-24
times sum |w| |x|, and stores it as the float32 intermediate of the next pass; 9 * 2^-24 covers both with one rounding to spare.  A later
pass multiplies an earlier pass's error by at most sum |w| per axis, which is what running the same passes with |w| on |x| does; so for p
executed passes |got - want| <= p * 9 * 2^-24 * A element-wise, A = abs_resize(x, target).  Every element of every case is compared."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lanczos_restate as R  # noqa: E402
import preproc_restate as P  # noqa: E402
import gpu_helpers  # noqa: E402
from gpu_helpers import _dev, _raw, _Recorder as _NamesRecorder  # noqa: E402

F32 = np.float32
U9 = 9.0 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _data(shape):
    """A smooth field, +-1e4 spikes (overshoot and cancellation) and an exact-zero region; seeded by the shape; read-only."""
    rng = np.random.default_rng(sum((i + 1) * s for i, s in enumerate(shape)) + len(shape))
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    x = sum(np.sin(0.37 * (i + 1) * a + i) for i, a in enumerate(g)) * 3.0 + rng.normal(0.0, 0.25, shape)
    spikes = rng.random(shape) < 0.04
    x[spikes] = rng.choice([-1e4, 1e4], int(spikes.sum()))
    flat = x.reshape(-1)
    n = flat.size
    flat[n // 3: n // 3 + max(n // 5, 1)] = 0.0
    x = x.astype(F32)
    x.setflags(write=False)
    return x


def _check_pass(x3, T, got, passes=1):
    """x3 [outer, L, inner] resampled along its middle axis."""
    want = R.apply_axis(x3, 1, T)
    A = R._apply(np.abs(x3.astype(np.float64)), 1, T, True)
    assert got.dtype == F32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    bound = passes * U9 * A
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    print('%s -> T = %d: max err %.3g, max err / bound %.3f' % (x3.shape, T, err.max(), ratio))
    assert (err <= bound).all()


ROWS = [(1, 1, 1), (3, 1, 5), (5, 2, 7), (7, 5, 3), (33, 140, 128), (2, 128, 140), (65, 9, 64), (4, 300, 17), (1, 1031, 1000),
        (70, 16, 300),                     # more rows than one LDS tile holds (64) and more outputs than a workgroup has threads
        (5, 1023, 40), (2, 1024, 33)]      # the longest row the LDS tile takes, and the shortest that is read directly


@pytest.mark.parametrize('outer,L,T', ROWS)
def test_single_pass_along_the_contiguous_axis(outer, L, T):
    from van_gan_amd.preprocess import resample_axis
    x = _data((outer, L, 1))
    xd = _dev(x)
    got = resample_axis(xd, T)
    assert got.is_cuda and got.shape == (outer, T, 1)
    _check_pass(x, T, got.cpu().numpy())
    assert np.array_equal(xd.cpu().numpy(), x)                             # the input is unchanged
    assert torch.equal(resample_axis(xd, T), got)                          # and the result reproducible bit for bit
    x2 = _dev(np.concatenate([np.zeros(1, F32), x.ravel()]))[1:].view(outer, L, 1)      # 4- but not 16-byte aligned: scalar staging loads
    assert x2.data_ptr() % 16 == 4
    assert torch.equal(resample_axis(x2, T), got)


STRIDED = [(1, 4, 3, 8), (2, 13, 5, 7), (1, 20, 140, 16), (3, 12, 128, 20), (1, 64, 8, 1),
           (300, 6, 2, 5),                 # more sub-volumes than a workgroup holds (128 of 2 columns): several o blocks
           (2, 9, 1100, 4)]                # more columns than a workgroup has threads: several i chunks of the 16-byte path


@pytest.mark.parametrize('outer,L,inner,T', STRIDED)
def test_single_pass_along_a_strided_axis(outer, L, inner, T):
    from van_gan_amd.preprocess import resample_axis
    x = _data((outer, L, inner))
    xd = _dev(x)
    got = resample_axis(xd, T)
    _check_pass(x, T, got.cpu().numpy())
    assert np.array_equal(xd.cpu().numpy(), x)
    assert torch.equal(resample_axis(xd, T), got)


def test_identity_table_copies_bit_for_bit():
    from van_gan_amd.preprocess import resample_axis
    x = _data((3, 8, 4))
    first = np.arange(8, dtype=np.int32) - 3
    w8 = np.zeros((8, 8), F32)
    w8[:, 3] = 1.0
    xd = _dev(x)
    got = resample_axis(xd, 8, table=(first, w8))
    assert got.cpu().numpy().tobytes() == x.tobytes()
    assert np.array_equal(xd.cpu().numpy(), x)
    rows = _dev(x.reshape(12, 8, 1))                                        # the same table along the contiguous axis
    assert resample_axis(rows, 8, table=(first, w8)).cpu().numpy().tobytes() == x.tobytes()


def test_vector_shape_from_a_misaligned_pointer():
    """inner % 4 == 0 would take the 16-byte path; from a pointer that is 4- but not 16-byte aligned the scalar kernel must serve it and
    give the same bits."""
    from van_gan_amd.preprocess import resample_axis
    x = _data((3, 12, 128))
    ref = resample_axis(_dev(x), 20)
    x2 = _dev(np.concatenate([np.zeros(1, F32), x.ravel()]))[1:].view(3, 12, 128)
    assert x2.data_ptr() % 16 == 4
    got = resample_axis(x2, 20)
    _check_pass(x, 20, got.cpu().numpy())
    assert torch.equal(got, ref)
    assert np.array_equal(x2.cpu().numpy(), x)


# ------------------------------------------------------------------------------------------------ whole volumes
class _Recorder(_NamesRecorder):
    """Also notes the vg_resample_axis calls' (outer, L, inner, T)."""

    def __init__(self, lib):
        super().__init__(lib)
        self.calls = []

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != 'vg_resample_axis':
            return fn

        def wrapped(x, outer, L, inner, T, *rest):
            self.calls.append((outer, L, inner, T))
            return fn(x, outer, L, inner, T, *rest)
        return wrapped


def _recorded(monkeypatch, fn, *a, **k):
    from van_gan_amd import preprocess
    rec = _Recorder(preprocess.lib)
    monkeypatch.setattr(preprocess, 'lib', rec)
    try:
        return fn(*a, **k), rec
    finally:
        monkeypatch.undo()


def _check_volume(x, target, got):
    want, p = R.resize(x, target)
    A = R.abs_resize(x, target)
    assert got.dtype == F32 and got.shape == tuple(target)
    err = np.abs(got.astype(np.float64) - want)
    bound = p * U9 * A
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    print('%s -> %s: %d passes, max err %.3g, max err / bound %.3f' % (x.shape, tuple(target), p, err.max(), ratio))
    assert (err <= bound).all()
    return p


def test_three_passes_in_the_order_y_x_z(monkeypatch):
    from van_gan_amd.preprocess import resize_volume
    x = _data((20, 12, 140))
    got, rec = _recorded(monkeypatch, resize_volume, x, (16, 16, 128))
    assert rec.calls == [(20, 12, 140, 16), (1, 20, 16 * 140, 16), (256, 140, 1, 128)]
    assert _check_volume(x, (16, 16, 128), got.cpu().numpy()) == 3


def test_z_only_is_one_call_and_the_single_pass_bitwise(monkeypatch):
    from van_gan_amd.preprocess import resample_axis, resize_volume
    x = _data((16, 16, 140))
    got, rec = _recorded(monkeypatch, resize_volume, x, (16, 16, 128))
    assert rec.calls == [(256, 140, 1, 128)]
    assert _check_volume(x, (16, 16, 128), got.cpu().numpy()) == 1
    assert torch.equal(got, resample_axis(_dev(x).view(256, 140, 1), 128).view(16, 16, 128))
    assert torch.equal(resize_volume(x, (16, 16, 128, 1)), got)            # a trailing 1 is tolerated


def test_equal_shape_makes_no_call(monkeypatch):
    from van_gan_amd.preprocess import resize_volume
    x = _data((9, 7, 5))
    got, rec = _recorded(monkeypatch, resize_volume, x, (9, 7, 5))
    assert rec.calls == [] and 'vg_resample_axis' not in rec.names
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), x)
    xd = _dev(x)
    assert resize_volume(xd, (9, 7, 5)).data_ptr() == xd.data_ptr()          # the fp32 volume itself


def test_upsampling():
    from van_gan_amd.preprocess import resize_volume
    x = _data((6, 5, 4))
    assert _check_volume(x, (12, 10, 9), resize_volume(x, (12, 10, 9)).cpu().numpy()) == 3


def test_constant_volume_stays_within_the_bound_of_its_constant():
    from van_gan_amd.preprocess import resize_volume
    c = F32(-731.25)
    x = np.full((10, 9, 12), c, F32)
    got = resize_volume(x, (7, 12, 10)).cpu().numpy()
    assert _check_volume(x, (7, 12, 10), got) == 3
    # the rows of |w| sum to at most 1.7146 + 1e-4 per axis (tests/test_resize_host.py), and a row of w to 1 within 4 * 2^-24
    assert (np.abs(got.astype(np.float64) - float(c)) <= 3 * (U9 * 1.7147 ** 3 + 4 * 2.0 ** -24 * 1.7147 ** 2) * abs(float(c))).all()


@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_integer_stacks_equal_their_float32_copy_bitwise(dtype):
    from van_gan_amd.preprocess import resize_volume
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 256 if dtype == 'uint8' else 65536, (12, 10, 35)).astype(dtype)
    got = resize_volume(raw, (8, 8, 32))
    assert got.shape == (8, 8, 32) and got.dtype == torch.float32
    assert torch.equal(got, resize_volume(raw.astype(F32), (8, 8, 32)))
    _check_volume(raw.astype(F32), (8, 8, 32), got.cpu().numpy())


# ------------------------------------------------------------------------------------------------ prepare_imaging / segment_volume
@pytest.mark.parametrize('dtype,pre', [('uint16', 'rsom'), ('uint8', None)])
def test_prepare_imaging_with_a_target(dtype, pre, monkeypatch):
    from van_gan_amd.preprocess import prepare_imaging, preprocess_rsom_images, resize_volume
    raw, tgt = _raw(dtype), (16, 16, 32)
    out_t, rec = _recorded(monkeypatch, prepare_imaging, raw, preprocess=pre, target_size=tgt)
    assert out_t.is_cuda and out_t.dtype == torch.float32 and out_t.shape == (16, 16, 32, 1)
    assert rec.calls == [(24, 20, 35, 16), (1, 24, 16 * 35, 16), (256, 35, 1, 32)]
    names = [n for n in rec.names if not n.endswith('_scratch_bytes')]
    head = ['vg_slice_moments', 'vg_zscore_slices', 'vg_order_stats', 'vg_clip_rescale'] if pre else ['vg_zscore_slices']
    assert names == head + ['vg_resample_axis'] * 3 + ['vg_minmax', 'vg_clip_rescale']
    # stage-wise: the device's own resized volume through the device-order restatement of min-max and (x - 0.5) / 0.5, bit for bit
    r = resize_volume(preprocess_rsom_images(raw), tgt) if pre else resize_volume(raw, tgt)
    r = r.cpu().numpy()
    lo, hi, want = P.device_order(r, 0.0, 100.0)
    assert lo == r.min() and hi == r.max()
    out = out_t.cpu().numpy()[..., 0]
    assert out.tobytes() == want.tobytes()
    assert out.min() == -1.0 and out.max() == 1.0
    assert torch.equal(prepare_imaging(raw, preprocess=pre, target_size=tgt, check=False), out_t)


@pytest.mark.parametrize('dtype,pre', [('uint16', 'rsom'), ('uint8', None), ('uint8', 'rsom')])
def test_target_equal_to_the_shape_gives_the_bits_of_no_target(dtype, pre, monkeypatch):
    from van_gan_amd.preprocess import prepare_imaging
    raw = _raw(dtype)
    got, rec = _recorded(monkeypatch, prepare_imaging, raw, preprocess=pre, target_size=(24, 20, 35))
    assert rec.calls == []
    assert torch.equal(got, prepare_imaging(raw, preprocess=pre))


def test_check_keeps_its_messages_with_a_target():
    from van_gan_amd.preprocess import MINMAX_ERROR, prepare_imaging
    v = _raw('uint8').astype(F32)
    v[3, 4, 5] = np.nan
    for pre in ('rsom', None):
        with pytest.raises(ValueError, match='NaN detected'):
            prepare_imaging(v, preprocess=pre, target_size=(16, 16, 32))
    const = np.full((24, 20, 35), 9, np.uint8)          # every z-score is exactly 0, and so is every resampled value
    with pytest.raises(ValueError) as e:
        prepare_imaging(const, target_size=(16, 16, 32))
    assert str(e.value) == MINMAX_ERROR
    for bad in (v, const):
        out = prepare_imaging(bad, target_size=(16, 16, 32), check=False)
        assert out.shape == (16, 16, 32, 1)
    torch.cuda.synchronize()


_engine = functools.lru_cache(maxsize=None)(gpu_helpers._engine)           # one engine per test module, as before


def test_segment_volume_passes_the_target_through(monkeypatch):
    """Raw (40, 36, 44) uint8 -> (32, 32, 32), a 32^3-window engine.  segment_volume(gen, raw, size, target_size=t) is
    stitch_subvolumes(gen, prepare_imaging(raw, target_size=t), size): torch.equal holds on ONE run of the stitch -- the tensor handed to it
    equals prepare_imaging(raw, target_size=t) bit for bit and what it returns is returned as it is.  Two separate runs of the generator
    differ in their last bits (float atomics in its InstanceNorm sums; tests/test_gpu_preproc.py compares the same way), so
    a second run is held to the bound of the stitch's own parity tests, 0.05 on the 0..255 scale, and its difference is printed."""
    from van_gan_amd.preprocess import prepare_imaging
    eng = _engine()
    raw = _raw('uint8', (40, 36, 44))
    tgt = (32, 32, 32)
    stitch, seen = eng.stitch_subvolumes, []

    def recording(gen, img, subvol_size=None, **kw):
        out = stitch(gen, img, subvol_size, **kw)
        seen.append((gen, img, subvol_size, kw, out))
        return out
    monkeypatch.setattr(eng, 'stitch_subvolumes', recording)
    got = eng.segment_volume('gen_IS', raw, (32, 32, 32), target_size=tgt)
    assert len(seen) == 1
    gen, img, subvol_size, kw, out = seen[0]
    assert gen == 'gen_IS' and subvol_size == (32, 32, 32) and kw == {}
    assert img.shape == (32, 32, 32, 1) and torch.equal(img, prepare_imaging(raw, target_size=tgt))
    assert got is out and torch.equal(got, out)
    assert got.shape == (32, 32, 32, 1) and bool(torch.isfinite(got).all())
    again = stitch('gen_IS', prepare_imaging(raw, target_size=tgt), (32, 32, 32))
    diff = float((again - got).abs().max())
    print('segment_volume(target_size) against a second stitch: max difference %.3g on the 0..255 scale, bitwise equal: %s' % (diff, torch.equal(again, got)))
    assert diff <= 0.05
