"""GPU: the prediction post-processing (csrc/vg_components.hip; van_gan_amd.postprocess) against the numpy / scipy restatement
(tests/components_restate.py, pinned on the CPU by tests/test_components_host.py).  Every result is an integer, and every comparison
is by equality: labels as scipy.ndimage.label numbers them (not up to a permutation), K, sizes, the masks, the histogram, Otsu's
threshold.  The labelling kernel's tile is 8 x 8 x 64 voxels (Z innermost) and its flat passes take 2048 voxels per workgroup: the
shapes below are one tile, one voxel more than a tile along each axis in turn, shapes that are no multiple of anything, and 64^3 (128
tiles, 128 chunks); the contents are chosen to break a tiled union-find, not to resemble a workload."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import components_restate as R  # noqa: E402
from gpu_helpers import DEV, _dev, _engine, _raw, _Recorder  # noqa: E402

F32 = np.float32
SHAPES = [(1, 1, 1), (1, 1, 300), (128, 3, 5), (8, 8, 64), (9, 8, 64), (8, 9, 64), (8, 8, 65), (37, 29, 70), (64, 64, 64)]
CONTENTS = ['zeros', 'ones', 'p0.1', 'p0.31', 'p0.6', 'checker']        # p = 0.31: the 6-neighbour percolation threshold
CONNS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _mask(shape, content):
    if content == 'zeros':
        m = np.zeros(shape, np.uint8)
    elif content == 'ones':
        m = np.ones(shape, np.uint8)
    elif content == 'checker':
        m = R.checkerboard(shape)
    elif content == 'snake':
        m = R.snake(shape)
    elif content in ('edge', 'corner'):
        m = R.rods(shape, content)
    elif content == 'chain':
        m = R.corner_chain(shape)
    else:
        m = R.bernoulli(shape, float(content[1:]))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref(shape, content, conn):
    lab, K = R.label(_mask(shape, content), conn)
    sz = R.sizes(lab, K)
    lab.setflags(write=False), sz.setflags(write=False)
    return lab, K, sz


def _check_labels(shape, content, conn):
    from van_gan_amd.postprocess import label_components
    m = _mask(shape, content)
    md = _dev(m)
    labels, K, sizes = label_components(md, conn, return_sizes=True)          # the read-back raises on a non-zero status
    want, wantK, want_sizes = _ref(shape, content, conn)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == shape
    assert np.array_equal(labels.cpu().numpy(), want), (shape, content, conn)
    assert K == wantK
    assert np.array_equal(sizes.cpu().numpy().astype(np.int64), want_sizes)
    assert np.array_equal(md.cpu().numpy(), m)                                # the mask is only read
    return labels


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_labels_are_scipys(shape, content):
    for conn in CONNS:
        _check_labels(shape, content, conn)


def test_the_checkerboard_separates_the_connectivities():
    assert [_ref((8, 8, 8), 'checker', c)[1] for c in CONNS] == [256, 1, 1]
    for conn in CONNS:
        _check_labels((8, 8, 8), 'checker', conn)


@pytest.mark.parametrize('content,shape,counts', [
    ('snake', (37, 29, 70), (1, 1, 1)),              # one path, one voxel wide, through every tile: the longest chains of parents
    ('edge', (16, 16, 128), (2, 1, 1)),              # two rods that touch by edges only, across a tile edge
    ('corner', (16, 16, 128), (2, 2, 1)),            # ... by one corner only, across a tile corner
    ('chain', (16, 16, 128), (16, 16, 1)),           # a component whose every link is a corner link, one of them across a tile corner
])
def test_crafted_paths(content, shape, counts):
    assert tuple(_ref(shape, content, c)[1] for c in CONNS) == counts
    if content == 'snake':
        m = _mask(shape, content)
        tiles = [(x, y, z) for x in range(0, shape[0], 8) for y in range(0, shape[1], 8) for z in range(0, shape[2], 64)]
        assert all(m[x:x + 8, y:y + 8, z:z + 64].any() for x, y, z in tiles)
    for conn in CONNS:
        _check_labels(shape, content, conn)


def test_label_entry_directly_status_scratch_and_a_second_call(monkeypatch):
    """vg_cc_label called as the wrapper calls it: result4 = (K, status 0, foreground, 0); the scratch the wrapper allocates is what
    vg_cc_scratch_bytes says; labels do not depend on what the scratch held; a bool mask and a trailing axis are taken."""
    from van_gan_amd import postprocess
    from van_gan_amd._lib import lib
    shape = (37, 29, 70)
    n = int(np.prod(shape))
    m = _mask(shape, 'p0.31')
    want, K, sz = _ref(shape, 'p0.31', 2)
    md = _dev(m)
    nbytes = int(lib.vg_cc_scratch_bytes(n))
    assert nbytes == 64 + 3 * ((4 * n + 15) // 16 * 16) + (4 * ((n + 2047) // 2048) + 15) // 16 * 16
    assert lib.vg_cc_scratch_bytes(0) < 0 and lib.vg_cc_scratch_bytes(2 ** 31) < 0
    labels = torch.empty(shape, dtype=torch.int32, device=DEV)
    sizes = torch.full((n // 2 + 2,), -7, dtype=torch.int32, device=DEV)
    result = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)            # garbage: the contents are irrelevant on entry
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vg_cc_label(md.data_ptr(), *shape, 2, labels.data_ptr(), sizes.data_ptr(), result.data_ptr(), scratch.data_ptr(), nbytes, st) == 0
    assert result.cpu().tolist() == [K, 0, int(m.sum()), 0]
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(sizes[:K + 1].cpu().numpy(), sz) and bool((sizes[K + 1:] == -7).all())      # entries beyond K are left alone
    assert lib.vg_cc_label(md.data_ptr(), *shape, 4, labels.data_ptr(), sizes.data_ptr(), result.data_ptr(), scratch.data_ptr(), nbytes, st) < 0
    assert lib.vg_cc_label(md.data_ptr(), *shape, 2, labels.data_ptr(), sizes.data_ptr(), result.data_ptr(), scratch.data_ptr(), nbytes - 1, st) < 0
    seen = []
    real = postprocess._scratch

    def spy(query, *args, dev):
        buf, b = real(query, *args, dev=dev)
        seen.append((query, args, buf.numel(), b))
        return buf, b
    monkeypatch.setattr(postprocess, '_scratch', spy)
    got, Kd = postprocess.label_components(md != 0, 2)                              # bool mask; enqueue-only: K stays on the device
    assert seen == [('vg_cc_scratch_bytes', (n,), nbytes, nbytes)]
    assert Kd.is_cuda and Kd.numel() == 1 and int(Kd) == K and torch.equal(got, labels)
    assert torch.equal(postprocess.label_components(md[..., None], 2)[0], labels)


@functools.lru_cache(maxsize=None)
def _min_sizes(shape, content, conn):
    sz = _ref(shape, content, conn)[2][1:]
    return (0, 1, 2, int(np.median(sz)), int(sz.max()), int(sz.max()) + 1)


@pytest.mark.parametrize('conn', (1, 3))
@pytest.mark.parametrize('shape,content', [((37, 29, 70), 'p0.1'), ((37, 29, 70), 'p0.31'), ((37, 29, 70), 'snake'), ((9, 8, 64), 'p0.6')])
def test_remove_small_objects(shape, content, conn):
    from van_gan_amd.postprocess import remove_small_objects
    m = _mask(shape, content)
    md = _dev(m)
    for min_size in _min_sizes(shape, content, conn):
        out = remove_small_objects(md, min_size, conn)
        assert out.dtype == torch.uint8 and tuple(out.shape) == shape
        assert np.array_equal(out.cpu().numpy(), R.remove_small(m, min_size, conn)), min_size
        out2, relab, K2 = remove_small_objects(md, min_size, conn, return_labels=True)
        want_lab, want_K = R.relabel_kept(m, min_size, conn)
        assert torch.equal(out2, out) and int(K2) == want_K and np.array_equal(relab.cpu().numpy(), want_lab), min_size
    assert np.array_equal(md.cpu().numpy(), m)
    twos = _dev(m * 2)                                                              # any non-zero value is foreground; the copy is 0 / 1
    assert np.array_equal(remove_small_objects(twos, 1, conn).cpu().numpy(), m)
    assert np.array_equal(remove_small_objects(twos, 2, conn).cpu().numpy(), R.remove_small(m, 2, conn))


def test_remove_small_objects_of_nothing_and_of_everything():
    """K = 0 (the filter's walk over sizes has no round) and one component that is the whole volume."""
    from van_gan_amd.postprocess import remove_small_objects, vessel_mask
    shape = (9, 8, 65)
    n = int(np.prod(shape))
    zeros, ones = _dev(np.zeros(shape, np.uint8)), _dev(np.ones(shape, np.uint8))
    for min_size in (0, 2, 64):
        out, relab, K2 = remove_small_objects(zeros, min_size, 3, return_labels=True)
        assert not bool(out.any()) and not bool(relab.any()) and int(K2) == 0
    assert bool(remove_small_objects(ones, n, 1).all()) and not bool(remove_small_objects(ones, n + 1, 1).any())
    pred = torch.zeros(shape, device=DEV)
    out, info = vessel_mask(pred, 127.5, 64, 3, return_info=True)
    assert not bool(out.any()) and info == dict(threshold=127.5, components=0, kept=0, voxels=0, kept_voxels=0)
    out, info = vessel_mask(pred + 200.0, 127.5, 64, 1, return_info=True)
    assert bool(out.all()) and info == dict(threshold=127.5, components=1, kept=1, voxels=n, kept_voxels=n)


def test_filter_entry_directly_with_unaligned_buffers():
    """vg_cc_filter on labels / out that are not 16- / 4-byte aligned takes the scalar kernel: the same results."""
    from van_gan_amd._lib import lib
    shape, conn, min_size = (37, 29, 70), 1, 5
    n = int(np.prod(shape))
    m = _mask(shape, 'p0.31')
    lab, K, sz = _ref(shape, 'p0.31', conn)
    labels = _dev(np.concatenate([np.zeros(1, np.int32), lab.ravel()]))[1:]
    sizes = _dev(sz.astype(np.int32))
    result = _dev(np.array([K, 0, int(m.sum()), 0], np.int32))
    out = torch.empty(n + 1, dtype=torch.uint8, device=DEV)[1:]
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    assert labels.data_ptr() % 16 == 4 and out.data_ptr() % 4 == 1
    st = torch.cuda.current_stream().cuda_stream
    assert lib.vg_cc_filter(labels.data_ptr(), n, sizes.data_ptr(), result.data_ptr(), min_size, out.data_ptr(), counts.data_ptr(), None, None, st) == 0
    want = R.remove_small(m, min_size, conn)
    assert np.array_equal(out.cpu().numpy().reshape(shape), want)
    assert counts.cpu().tolist() == [int(want.sum()), int((sz[1:] >= min_size).sum())]


# ------------------------------------------------------------------------------------------------ histogram, Otsu, threshold
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000003])
def test_hist256_is_bincount(n):
    from van_gan_amd.postprocess import histogram256
    from van_gan_amd._lib import lib
    rng = np.random.default_rng(n)
    one = np.full((1, 1, n), 77.9, F32)                                             # one bin takes every voxel
    h, bad = histogram256(_dev(one), return_count=True)
    assert np.array_equal(h.cpu().numpy(), R.hist256(one)) and int(h[77]) == n and int(bad) == 0
    x = (rng.random((1, 1, n)) * 256).astype(F32)
    x = np.minimum(x, np.nextafter(F32(256), F32(0)))
    x[0, 0, :: 7] = np.floor(x[0, 0, :: 7])                                         # values that sit exactly on a bin edge
    x[0, 0, 0] = 255.0
    want = R.hist256(x)
    assert want.sum() == n and np.array_equal(want, np.bincount(x.astype(np.uint8).ravel(), minlength=256))
    if n > 100000:
        assert (want > 0).all()                                                     # all 256 bins are hit
    xd = _dev(x)
    assert np.array_equal(histogram256(xd).cpu().numpy(), want)
    assert np.array_equal(xd.cpu().numpy(), x)
    # an unaligned pointer (the scalar kernel), two non-finite voxels, and a histogram buffer that held garbage
    y = np.concatenate([np.zeros(1, F32), x.ravel()])
    if n > 2:
        y[1], y[n] = np.nan, -np.inf
    yd = _dev(y)[1:]
    hist = torch.full((256,), 12345, dtype=torch.int32, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.vg_hist256(yd.data_ptr(), n, hist.data_ptr(), bad.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(hist.cpu().numpy(), R.hist256(y[1:])) and int(bad) == (2 if n > 2 else 0)


@functools.lru_cache(maxsize=None)
def _prediction(shape=(40, 33, 50)):
    """Prediction-like: 255 * minmax of a dark background and bright tubes, fp32 in [0, 255] with both ends attained."""
    rng = np.random.default_rng(11)
    v = rng.normal(40.0, 12.0, shape)
    tubes = R.bernoulli(shape, 0.02, seed=5).astype(bool)
    for s in range(1, 6):
        tubes[..., s:] |= tubes[..., :-s]
    v[tubes] = rng.normal(200.0, 25.0, int(tubes.sum()))
    v = (v - v.min()) / (v.max() - v.min())
    p = (255.0 * v).astype(F32)
    p.setflags(write=False)
    return p


def test_otsu_threshold_is_the_restatement():
    from van_gan_amd.postprocess import binarise_prediction
    p = _prediction()
    t_want = R.otsu(R.hist256(p))
    assert 60 < t_want < 200                                                        # between the two modes
    pd = _dev(p)
    mask, t = binarise_prediction(pd, 'otsu', return_threshold=True)
    assert t == t_want
    assert np.array_equal(mask.cpu().numpy(), R.binarise(p, 'otsu')) and np.array_equal(mask.cpu().numpy(), (p.astype(np.uint8) > t_want).astype(np.uint8))
    assert torch.equal(binarise_prediction(pd[..., None], 'otsu'), mask) and np.array_equal(pd.cpu().numpy(), p)
    flat = np.full((5, 6, 7), 200.0, F32)                                           # one occupied bin: every variance is 0, t = 0
    mask, t = binarise_prediction(_dev(flat), 'otsu', return_threshold=True)
    assert t == 0.0 == R.otsu(R.hist256(flat)) and bool(mask.all())
    three = np.zeros((3, 5, 64), F32)                                               # three occupied bins
    three[1], three[2, :2] = 100.5, 255.0
    mask, t = binarise_prediction(_dev(three), 'otsu', return_threshold=True)
    assert t == R.otsu(R.hist256(three)) and np.array_equal(mask.cpu().numpy(), R.binarise(three, 'otsu'))


def test_binarise_with_thresholds_that_sit_on_a_voxel_value():
    from van_gan_amd.postprocess import binarise_prediction
    p = _prediction((9, 8, 65)).copy()
    p.ravel()[:8] = [127.5, np.nextafter(F32(127.5), F32(200)), np.nextafter(F32(127.5), F32(0)), 127.0, 128.0, 127.99, 0.0, 255.0]
    p[3, 3, 3], p[4, 4, 4] = np.nan, np.inf                                         # non-finite: background
    pd = _dev(p)
    for thr in (127.5, 127.0, 0.0, 255.0, float(p[5, 5, 5]), -1.0, 127, 128, 0, 255):
        got = binarise_prediction(pd, thr)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.binarise(p, thr)), thr
    assert binarise_prediction(pd, 127.5).cpu().numpy().ravel()[:6].tolist() == [0, 1, 0, 0, 1, 1]
    assert binarise_prediction(pd, 127).cpu().numpy().ravel()[:6].tolist() == [0, 0, 0, 0, 1, 0]      # uint8(pred) > 127
    t_dev = torch.tensor([127.5], device=DEV)
    assert torch.equal(binarise_prediction(pd, t_dev), binarise_prediction(pd, 127.5))
    assert binarise_prediction(pd, 127.5, return_threshold=True)[1] == 127.5
    assert np.array_equal(pd.cpu().numpy(), p, equal_nan=True)
    # an unaligned prediction (the scalar kernel)
    q = _dev(np.concatenate([np.zeros(1, F32), p.ravel()]))[1:].view(p.shape)
    assert q.data_ptr() % 16 == 4 and torch.equal(binarise_prediction(q, 127.5), binarise_prediction(pd, 127.5))


@pytest.mark.parametrize('threshold,min_size,conn', [(127.5, 64, 3), ('otsu', 5, 1), (100, 1, 2), (90.0, 0, 3)])
def test_vessel_mask_is_the_three_functions_chained(threshold, min_size, conn):
    from van_gan_amd.postprocess import binarise_prediction, label_components, remove_small_objects, vessel_mask
    p = _prediction()
    pd = _dev(p)
    by_hand = remove_small_objects(binarise_prediction(pd, threshold), min_size, conn)
    got = vessel_mask(pd, threshold, min_size, conn)
    assert torch.equal(got, by_hand)
    assert np.array_equal(got.cpu().numpy(), R.vessel_mask(p, threshold, min_size, conn))
    got2, info = vessel_mask(pd[..., None], threshold, min_size, conn, return_info=True)
    assert torch.equal(got2, got)
    b = R.binarise(p, threshold)
    lab, K = R.label(b, conn)
    sz = R.sizes(lab, K)
    t_want = float(R.otsu(R.hist256(p))) if threshold == 'otsu' else float(threshold)
    assert info == dict(threshold=t_want, components=K, kept=int((sz[1:] >= min_size).sum()), voxels=int(b.sum()), kept_voxels=int(got.sum()))
    assert label_components(binarise_prediction(pd, threshold), conn, return_sizes=True)[1] == K
    assert np.array_equal(pd.cpu().numpy(), p)


def test_non_contiguous_device_tensors_are_refused():
    from van_gan_amd import postprocess as P
    m = _dev(_mask((37, 29, 70), 'p0.31'))
    p = _dev(_prediction())
    for fn, x in ((P.label_components, m), (P.remove_small_objects, m), (P.binarise_prediction, p), (P.vessel_mask, p), (P.histogram256, p)):
        with pytest.raises(ValueError, match='contiguous'):
            fn(x.transpose(0, 2))
        with pytest.raises(ValueError, match='contiguous'):
            fn(x[:, :, ::2])
    got = P.label_components(m.transpose(0, 2).contiguous(), 3)[0]                   # made contiguous, the same data is taken
    assert np.array_equal(got.cpu().numpy(), R.label(_mask((37, 29, 70), 'p0.31').transpose(2, 1, 0), 3)[0])
    torch.cuda.synchronize()


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


def test_the_calls_of_every_recipe(monkeypatch):
    pd = _dev(_prediction())
    md = _dev(_mask((37, 29, 70), 'p0.31'))
    assert _calls(monkeypatch, 'binarise_prediction', pd) == ['vg_threshold_mask']
    assert _calls(monkeypatch, 'binarise_prediction', pd, 100) == ['vg_threshold_mask']
    assert _calls(monkeypatch, 'binarise_prediction', pd, 'otsu') == ['vg_hist256', 'vg_threshold_mask']
    assert _calls(monkeypatch, 'histogram256', pd) == ['vg_hist256']
    assert _calls(monkeypatch, 'label_components', md, 2) == LABEL_CALLS
    assert _calls(monkeypatch, 'label_components', md, 2, return_sizes=True) == LABEL_CALLS
    assert _calls(monkeypatch, 'remove_small_objects', md) == LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'remove_small_objects', md, 1) == []                  # a copy
    assert _calls(monkeypatch, 'vessel_mask', pd) == ['vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'vessel_mask', pd, 'otsu', 64, 1, return_info=True) == ['vg_hist256', 'vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'vessel_mask', pd, 127.5, 1) == ['vg_threshold_mask']
    # the calls do not depend on the data
    assert _calls(monkeypatch, 'vessel_mask', torch.zeros_like(pd)) == _calls(monkeypatch, 'vessel_mask', pd)
    torch.cuda.synchronize()


def test_segment_mask_is_vessel_mask_of_segment_volume(monkeypatch):
    """VanGan.segment_mask hands vessel_mask exactly what segment_volume returns for the same keywords (one run of the stitch: two runs
    differ in their last bits, see tests/test_gpu_preproc.py), and returns vessel_mask's result."""
    from van_gan_amd.postprocess import vessel_mask
    eng = _engine()
    raw = _raw('uint8', (48, 40, 36))
    segment, seen = eng.segment_volume, []

    def recording(gen, raw, subvol_size=None, **kw):
        out = segment(gen, raw, subvol_size, **kw)
        seen.append((gen, subvol_size, kw, out))
        return out
    monkeypatch.setattr(eng, 'segment_volume', recording)
    got, info = eng.segment_mask('gen_IS', raw, (32, 32, 32), threshold='otsu', min_size=4, connectivity=2, return_info=True, stride=(8, 8, 4))
    assert len(seen) == 1
    gen, subvol_size, kw, pred = seen[0]
    assert gen == 'gen_IS' and subvol_size == (32, 32, 32) and kw == dict(stride=(8, 8, 4)) and pred.shape == (48, 40, 36, 1)
    want, want_info = vessel_mask(pred, 'otsu', 4, 2, return_info=True)
    assert got.dtype == torch.uint8 and got.shape == (48, 40, 36) and torch.equal(got, want) and info == want_info
    assert np.array_equal(got.cpu().numpy(), R.vessel_mask(pred.cpu().numpy(), 'otsu', 4, 2))
    plain = eng.segment_mask('gen_IS', raw, (32, 32, 32), stride=(8, 8, 4))          # the defaults: 127.5, 64 voxels, 26 neighbours
    assert len(seen) == 2 and torch.equal(plain, vessel_mask(seen[1][3]))
