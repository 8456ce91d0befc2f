"""GPU: the mask measurements (csrc/vg_edt.hip; van_gan_amd.postprocess distance_transform_edt, fill_holes, vessel_radius) against the
numpy restatement (tests/edt_restate.py, pinned to scipy on the CPU by tests/test_edt_host.py).  The integer transform and the hole
filling are compared by equality; the weighted transform within one fp32 ulp of the float64 reference, |dev - fp32(ref)| <= 2^-23 |ref|:
both sides evaluate the same minimum in fp64, possibly in a different order, which can move the fp32 rounding by one place at most.

Shapes: the smallest that can break the indexing -- unit axes, rows just over one wave, Y over 128, one long row -- and one shape on
each side of every edge the kernels introduce: pass Z cuts a row into pieces of 64 voxels (Z = 63, 64, 65) and takes four rows per
workgroup (4 rows: (1,4,64), (2,2,1500); 5 rows: (5,1,3)); the passes along Y and X and the hole-filling kernels run 256 threads per
workgroup over the flat volume (255, 256 and 257 voxels: (5,17,3), (1,4,64), (1,1,257)), the hole filling four voxels per thread where
the pointers allow (voxel counts that are no multiple of 4, and an unaligned direct call)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edt_restate as R  # noqa: E402
from gpu_helpers import DEV, _dev, _Recorder  # noqa: E402

SHAPES = [(1, 1, 1), (5, 1, 3), (9, 17, 70), (16, 9, 65), (3, 130, 67), (2, 2, 1500),
          (4, 1, 63), (1, 4, 64), (5, 17, 3), (1, 1, 257)]
CONTENTS = ['zeros', 'ones', 'corner', 'plane', 'p0.5', 'p0.9', 'p0.999']
SAMPLING = (2.0, 0.5, 1.25)
_ids = dict(ids=lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s))


@functools.lru_cache(maxsize=None)
def _mask(shape, content):
    if content == 'zeros':
        m = np.zeros(shape, np.uint8)
    elif content == 'ones':
        m = np.ones(shape, np.uint8)
    elif content == 'corner':
        m = R.one_background_corner(shape)
    elif content == 'plane':
        m = R.background_plane(shape)
    elif content == 'tubes':
        m = R.tubes(shape)
    else:
        m = R.bernoulli(shape, float(content[1:]))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref(shape, content):
    """(squared int64, fp32 distances, float64 weighted distances) of the restatement, computed once"""
    m = _mask(shape, content)
    sq, wd = R.edt_sq(m), R.edt_weighted(m, SAMPLING)
    dist = np.where(sq == R.INF, np.inf, np.sqrt(sq.astype(np.float64))).astype(np.float32)
    for a in (sq, dist, wd):
        a.setflags(write=False)
    return sq, dist, wd


def _check_edt(shape, content):
    from van_gan_amd.postprocess import distance_transform_edt
    m = _mask(shape, content)
    sq, dist, wd = _ref(shape, content)
    md = _dev(m)
    got_sq = distance_transform_edt(md, squared=True)
    assert got_sq.is_cuda and got_sq.dtype == torch.int32 and tuple(got_sq.shape) == shape
    assert np.array_equal(got_sq.cpu().numpy().astype(np.int64), sq), (shape, content)
    got = distance_transform_edt(md)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), dist), (shape, content)
    got_w = distance_transform_edt(md, SAMPLING).cpu().numpy()
    assert got_w.dtype == np.float32
    inf = np.isinf(wd)
    assert np.array_equal(np.isinf(got_w), inf) and not np.isnan(got_w).any()
    err = np.abs(got_w.astype(np.float64)[~inf] - wd.astype(np.float32).astype(np.float64)[~inf])
    worst = float((err / np.maximum(wd[~inf], 1e-300)).max()) if err.size else 0.0
    print('weighted %s %s: largest |dev - fp32(ref)| / |ref| = %.3g' % (shape, content, worst))
    assert np.all(err <= 2.0 ** -23 * np.abs(wd[~inf])), (shape, content, worst)
    assert np.array_equal(md.cpu().numpy(), m)                                      # the mask is only read


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_distances_are_the_restatements(shape, content):
    _check_edt(shape, content)


def test_distances_of_a_tube_volume():
    shape = (24, 33, 70)
    m = _mask(shape, 'tubes')
    assert 0.01 < m.mean() < 0.5                                                    # a network, not an empty or a full volume
    _check_edt(shape, 'tubes')


def test_what_the_crafted_masks_exercise():
    """The corner mask reaches the largest distance of its shape in the last voxel; the plane mask keeps the sentinel in every row and
    column off the plane until the last pass; a volume without background is the sentinel, +inf as a distance."""
    from van_gan_amd.postprocess import EDT_INF, distance_transform_edt
    shape = (9, 17, 70)
    sq = _ref(shape, 'corner')[0]
    assert sq[-1, -1, -1] == 8 * 8 + 16 * 16 + 69 * 69 == sq.max()
    plane = _mask(shape, 'plane')
    assert plane[:4].all() and plane[5:].all() and (_ref(shape, 'plane')[0] < R.INF).all()
    ones = _dev(_mask(shape, 'ones'))
    assert EDT_INF == R.INF and bool((distance_transform_edt(ones, squared=True) == EDT_INF).all())
    assert bool(torch.isposinf(distance_transform_edt(ones)).all()) and bool(torch.isposinf(distance_transform_edt(ones, 1.5)).all())
    twos = _dev(_mask(shape, 'p0.9') * 2)                                           # any non-zero value is foreground; bool and [X,Y,Z,1] are taken
    want = _ref(shape, 'p0.9')[1]
    assert np.array_equal(distance_transform_edt(twos).cpu().numpy(), want)
    assert np.array_equal(distance_transform_edt(twos != 0).cpu().numpy(), want)
    assert np.array_equal(distance_transform_edt(twos[..., None]).cpu().numpy(), want)
    unit = distance_transform_edt(twos, (1.0, 1.0, 1.0)).cpu().numpy()              # weight 1 on the fp64 path: the integer form's result
    assert np.array_equal(unit, want)


def test_edt_entry_directly_scratch_and_refusals(monkeypatch):
    """vg_edt called as the wrapper calls it: the scratch the wrapper allocates is what vg_edt_scratch_bytes says, the result does not
    depend on what the scratch or the output held, and bad arguments are refused before anything is launched."""
    import ctypes
    from van_gan_amd import postprocess
    from van_gan_amd._lib import lib
    shape = (9, 17, 70)
    n = int(np.prod(shape))
    sq, dist, wd = _ref(shape, 'p0.9')
    md = _dev(_mask(shape, 'p0.9'))
    st = torch.cuda.current_stream().cuda_stream
    for weighted, esz in ((0, 4), (1, 8)):
        nbytes = int(lib.vg_edt_scratch_bytes(*shape, weighted))
        assert nbytes == 2 * ((esz * n + 15) // 16 * 16)
        scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
        out = torch.full(shape, -7.0, dtype=torch.float32, device=DEV)
        s3 = (ctypes.c_double * 3)(*SAMPLING) if weighted else None
        assert lib.vg_edt(md.data_ptr(), *shape, s3, out.data_ptr(), 1, scratch.data_ptr(), nbytes, st) == 0
        if weighted:
            assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - wd.astype(np.float32)) <= 2.0 ** -23 * wd)
        else:
            assert np.array_equal(out.cpu().numpy(), dist)
            out_i = torch.full(shape, -7, dtype=torch.int32, device=DEV)
            assert lib.vg_edt(md.data_ptr(), *shape, None, out_i.data_ptr(), 0, scratch.data_ptr(), nbytes, st) == 0
            assert np.array_equal(out_i.cpu().numpy(), sq)
        assert lib.vg_edt(md.data_ptr(), *shape, s3, out.data_ptr(), 1, scratch.data_ptr(), nbytes - 1, st) < 0
        assert lib.vg_edt(md.data_ptr(), *shape, s3, out.data_ptr(), 2, scratch.data_ptr(), nbytes, st) < 0
    assert lib.vg_edt_scratch_bytes(46341, 1, 1, 0) < 0 and lib.vg_edt_scratch_bytes(0, 1, 1, 0) < 0
    seen = []
    real = postprocess._scratch

    def spy(query, *args, dev):
        buf, b = real(query, *args, dev=dev)
        seen.append((query, args, buf.numel(), b))
        return buf, b
    monkeypatch.setattr(postprocess, '_scratch', spy)
    postprocess.distance_transform_edt(md)
    postprocess.distance_transform_edt(md, SAMPLING)
    b4, b8 = 2 * ((4 * n + 15) // 16 * 16), 2 * ((8 * n + 15) // 16 * 16)
    assert seen == [('vg_edt_scratch_bytes', shape + (0,), b4, b4), ('vg_edt_scratch_bytes', shape + (1,), b8, b8)]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ hole filling
HOLE_SHAPES = [((9, 17, 70), 0.5), ((16, 9, 65), 0.85), ((5, 1, 3), 0.5), ((1, 1, 1), 0.0), ((1, 4, 64), 0.6), ((5, 17, 3), 0.7), ((1, 1, 257), 0.5),
               ((12, 11, 10), 0.7)]


def test_fill_holes_is_the_restatement():
    from van_gan_amd.postprocess import fill_holes
    cases = dict(R.hole_cases())
    for shape, p in HOLE_SHAPES:
        cases['bernoulli %s %s' % (shape, p)] = R.bernoulli(shape, p)
    cases['zeros'], cases['ones'] = np.zeros((9, 8, 65), np.uint8), np.ones((9, 8, 65), np.uint8)
    filled = 0
    for name, m in cases.items():
        md = _dev(m)
        got = fill_holes(md)
        want = R.fill_holes(m)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == md.shape
        assert np.array_equal(got.cpu().numpy(), want), name
        assert np.array_equal(md.cpu().numpy(), m), name
        filled += int(want.sum() - m.sum())
        assert torch.equal(fill_holes(md * 3), got) and torch.equal(fill_holes(md != 0), got), name      # non-zero is foreground; bool is taken
    assert filled > 1000                                                            # the cases do hold holes


def test_fill_holes_entries_directly_with_unaligned_buffers():
    """vg_fill_holes_mark zeroes its flags itself; vg_fill_holes_apply on pointers that are not 16- / 4-byte aligned takes the scalar
    kernel: the same result.  labels are vg_cc_label's of the inverted mask at connectivity 1."""
    from van_gan_amd._lib import lib
    from van_gan_amd.postprocess import label_components, sizes_capacity
    shape = (9, 17, 70)
    n = int(np.prod(shape))
    m = R.bernoulli(shape, 0.5)
    want = R.fill_holes(m)
    assert want.sum() > m.sum()
    md = _dev(m)
    labels, _ = label_components(md == 0, 1)
    st = torch.cuda.current_stream().cuda_stream
    flags = torch.full((sizes_capacity(n),), 0xAB, dtype=torch.uint8, device=DEV)   # garbage: mark zeroes it
    assert lib.vg_fill_holes_mark(labels.data_ptr(), *shape, flags.data_ptr(), st) == 0
    out = torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    assert lib.vg_fill_holes_apply(md.data_ptr(), labels.data_ptr(), flags.data_ptr(), n, out.data_ptr(), st) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    lab1 = _dev(np.concatenate([np.zeros(1, np.int32), labels.cpu().numpy().ravel()]))[1:]
    m1 = _dev(np.concatenate([np.zeros(1, np.uint8), m.ravel()]))[1:]
    out1 = torch.full((n + 1,), 9, dtype=torch.uint8, device=DEV)[1:]
    assert lab1.data_ptr() % 16 == 4 and m1.data_ptr() % 4 == 1 and out1.data_ptr() % 4 == 1
    assert lib.vg_fill_holes_apply(m1.data_ptr(), lab1.data_ptr(), flags.data_ptr(), n, out1.data_ptr(), st) == 0
    assert np.array_equal(out1.cpu().numpy().reshape(shape), want)
    assert lib.vg_fill_holes_mark(labels.data_ptr(), 9, 0, 70, flags.data_ptr(), st) < 0
    assert lib.vg_fill_holes_apply(md.data_ptr(), labels.data_ptr(), flags.data_ptr(), 0, out.data_ptr(), st) < 0


# ------------------------------------------------------------------------------------------------ the chained recipes
@functools.lru_cache(maxsize=None)
def _prediction(shape=(40, 33, 50)):
    """Prediction-like: hollow bright tubes on a dark background, fp32 in [0, 255], so that the threshold leaves cavities to close."""
    rng = np.random.default_rng(11)
    v = rng.normal(40.0, 12.0, shape)
    seeds = R.bernoulli(shape, 0.004, seed=5).astype(bool)
    wall = np.zeros(shape, bool)
    for x, y, z in zip(*np.nonzero(seeds)):
        wall[max(x - 2, 0):x + 3, max(y - 2, 0):y + 3, max(z - 4, 0):z + 5] = True
    lumen = np.zeros(shape, bool)
    for x, y, z in zip(*np.nonzero(seeds)):
        lumen[max(x - 1, 0):x + 2, max(y - 1, 0):y + 2, max(z - 3, 0):z + 4] = True
    wall &= ~lumen
    v[wall] = rng.normal(200.0, 10.0, int(wall.sum()))
    p = np.clip(v, 0.0, 255.0).astype(np.float32)
    p.setflags(write=False)
    return p


def test_vessel_radius_and_vessel_mask_are_the_functions_chained():
    from van_gan_amd.postprocess import distance_transform_edt, fill_holes, vessel_mask, vessel_radius
    p = _prediction()
    pd = _dev(p)
    plain = vessel_mask(pd, 127.5, 8, 1)
    by_hand = fill_holes(plain)
    assert int(by_hand.sum()) > int(plain.sum())                                    # there are cavities to close
    got = vessel_mask(pd, 127.5, 8, 1, fill_holes=True)
    assert torch.equal(got, by_hand) and np.array_equal(got.cpu().numpy(), R.fill_holes(plain.cpu().numpy()))
    got2, info = vessel_mask(pd, 127.5, 8, 1, return_info=True, fill_holes=True)
    _, info_plain = vessel_mask(pd, 127.5, 8, 1, return_info=True)
    assert torch.equal(got2, by_hand) and info == info_plain                        # the info counts what was there before the filling
    assert torch.equal(vessel_mask(pd, 127.5, 1, 1, fill_holes=True), fill_holes(vessel_mask(pd, 127.5, 1, 1)))
    for sampling in (None, SAMPLING):
        assert torch.equal(vessel_radius(plain, sampling), distance_transform_edt(by_hand, sampling))
        assert torch.equal(vessel_radius(plain, sampling, fill=False), distance_transform_edt(plain, sampling))
    assert float(vessel_radius(plain).max()) > float(vessel_radius(plain, fill=False).max())      # a closed lumen is measured to the wall
    assert np.array_equal(vessel_radius(plain).cpu().numpy(), R.edt(R.fill_holes(plain.cpu().numpy())))


def _calls(monkeypatch, fn, *args, **kw):
    from van_gan_amd import postprocess
    rec = _Recorder(postprocess.lib)
    monkeypatch.setattr(postprocess, 'lib', rec)
    try:
        getattr(postprocess, fn)(*args, **kw)
    finally:
        monkeypatch.undo()
    return rec.names


LABEL_CALLS = ['vg_cc_scratch_bytes', 'vg_cc_label']
FILL_CALLS = LABEL_CALLS + ['vg_fill_holes_mark', 'vg_fill_holes_apply']
EDT_CALLS = ['vg_edt_scratch_bytes', 'vg_edt']


def test_the_calls_of_every_recipe(monkeypatch):
    """vessel_mask with the default keyword issues what it issued before; the new recipes issue a fixed list whatever the data."""
    pd = _dev(_prediction())
    md = _dev(_mask((9, 17, 70), 'p0.9'))
    before = ['vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'vessel_mask', pd) == before
    assert _calls(monkeypatch, 'vessel_mask', pd, fill_holes=False) == before
    assert _calls(monkeypatch, 'vessel_mask', pd, 127.5, 1) == ['vg_threshold_mask']
    assert _calls(monkeypatch, 'vessel_mask', pd, 'otsu', 64, 1, return_info=True) == ['vg_hist256', 'vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'vessel_mask', pd, fill_holes=True) == before + FILL_CALLS
    assert _calls(monkeypatch, 'vessel_mask', pd, 127.5, 1, fill_holes=True) == ['vg_threshold_mask'] + FILL_CALLS
    assert _calls(monkeypatch, 'distance_transform_edt', md) == EDT_CALLS
    assert _calls(monkeypatch, 'distance_transform_edt', md, SAMPLING) == EDT_CALLS
    assert _calls(monkeypatch, 'distance_transform_edt', md, squared=True) == EDT_CALLS
    assert _calls(monkeypatch, 'fill_holes', md) == FILL_CALLS
    assert _calls(monkeypatch, 'vessel_radius', md) == FILL_CALLS + EDT_CALLS
    assert _calls(monkeypatch, 'vessel_radius', md, fill=False) == EDT_CALLS
    assert _calls(monkeypatch, 'vessel_radius', torch.zeros_like(md)) == FILL_CALLS + EDT_CALLS      # the calls do not depend on the data
    torch.cuda.synchronize()


def test_non_contiguous_and_oversized_volumes_are_refused():
    from van_gan_amd import postprocess as P
    m = _dev(_mask((9, 17, 70), 'p0.9'))
    for fn in (P.distance_transform_edt, P.fill_holes, P.vessel_radius):
        with pytest.raises(ValueError, match='contiguous'):
            fn(m.transpose(0, 2))
    with pytest.raises(ValueError, match='squared'):
        P.distance_transform_edt(m, SAMPLING, squared=True)
    with pytest.raises(ValueError, match=r'X\^2'):
        P.distance_transform_edt(torch.zeros(46341, 1, 1, dtype=torch.uint8, device=DEV))
