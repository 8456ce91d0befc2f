"""CPU: what the GPU suite of the prediction post-processing rests on (tests/test_gpu_components.py compares the kernels with
tests/components_restate.py by equality, so the restatement itself is pinned here): scipy.ndimage.label's numbering, remove_small against
a flood fill written out, Otsu's threshold against its definition in exact arithmetic; and the host side of van_gan_amd.postprocess:
the argument checks, which come before any device access, and the scratch arithmetic through the query entry, which launches nothing."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import components_restate as R


# ------------------------------------------------------------------------------------------------ the numbering claim
@pytest.mark.parametrize('conn', (1, 2, 3))
@pytest.mark.parametrize('shape,p', [((37, 29, 70), 0.31), ((1, 1, 300), 0.6), ((128, 3, 5), 0.1), ((12, 9, 70), 0.6)])
def test_scipy_numbers_components_by_their_first_voxel(shape, p, conn):
    lab, K = R.label(R.bernoulli(shape, p), conn)
    flat = lab.ravel()
    first = np.full(K + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    assert K >= 1 and np.all(np.diff(first[1:]) > 0)               # label k's first voxel precedes label k + 1's
    assert np.array_equal(R.sizes(lab, K), np.bincount(flat)) and R.sizes(lab, K).sum() == flat.size


def test_the_crafted_masks_are_what_they_claim():
    assert [R.label(R.checkerboard((8, 8, 8)), c)[1] for c in (1, 2, 3)] == [256, 1, 1]
    assert [R.label(R.rods((16, 16, 128), 'edge'), c)[1] for c in (1, 2, 3)] == [2, 1, 1]
    assert [R.label(R.rods((16, 16, 128), 'corner'), c)[1] for c in (1, 2, 3)] == [2, 2, 1]
    assert [R.label(R.corner_chain((16, 16, 128)), c)[1] for c in (1, 2, 3)] == [16, 16, 1]
    m = R.snake((37, 29, 70))
    assert R.label(m, 1)[1] == 1
    import scipy.ndimage as ndi
    faces = ndi.convolve(m.astype(np.int64), R.structure(1).astype(np.int64), mode='constant') - 1
    assert sorted(np.unique(faces[m > 0], return_counts=True)[1].tolist()) == [2, int(m.sum()) - 2]      # a path: two ends, no branch


# ------------------------------------------------------------------------------------------------ remove_small against a flood fill
def _flood_sizes(mask, conn):
    """size of the component of every foreground voxel, by a flood fill over the neighbours with at most conn differing axes"""
    offs = [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, d)) <= conn]
    size = np.zeros(mask.shape, np.int64)
    seen = np.zeros(mask.shape, bool)
    for start in zip(*np.nonzero(mask)):
        if seen[start]:
            continue
        comp, todo = [start], [start]
        seen[start] = True
        while todo:
            v = todo.pop()
            for d in offs:
                u = tuple(a + b for a, b in zip(v, d))
                if all(0 <= c < s for c, s in zip(u, mask.shape)) and mask[u] and not seen[u]:
                    seen[u] = True
                    comp.append(u)
                    todo.append(u)
        for v in comp:
            size[v] = len(comp)
    return size


@pytest.mark.parametrize('conn', (1, 2, 3))
@pytest.mark.parametrize('shape,p', [((6, 6, 6), 0.31), ((4, 5, 6), 0.5), ((1, 6, 6), 0.4), ((6, 6, 6), 0.15)])
def test_remove_small_is_a_flood_fill(shape, p, conn):
    m = R.bernoulli(shape, p, seed=conn)
    size = _flood_sizes(m, conn)
    for min_size in (0, 1, 2, 3, int(size.max()), int(size.max()) + 1):
        want = ((m != 0) & (size >= min_size)).astype(np.uint8)
        assert np.array_equal(R.remove_small(m, min_size, conn), want), min_size
        relab, K2 = R.relabel_kept(m, min_size, conn)
        assert np.array_equal(relab != 0, want != 0) and K2 == (len(np.unique(relab)) - (1 if (relab == 0).any() else 0))
        assert np.array_equal(relab, R.label(want, conn)[0])       # dropping components keeps the order of the others


# ------------------------------------------------------------------------------------------------ Otsu in exact arithmetic
def _exact_variances(hist):
    """The between-class variance of all 255 splits as Fractions: w1 w2 (m1 - m2)^2, 0 where a class is empty."""
    h = [int(v) for v in hist]
    out = []
    for i in range(255):
        w1, w2 = sum(h[:i + 1]), sum(h[i + 1:])
        if w1 == 0 or w2 == 0:
            out.append(Fraction(0))
            continue
        m1 = Fraction(sum(b * h[b] for b in range(i + 1)), w1)
        m2 = Fraction(sum(b * h[b] for b in range(i + 1, 256)), w2)
        out.append(w1 * w2 * (m1 - m2) ** 2)
    return out


def _hist(pairs):
    h = np.zeros(256, np.int64)
    for b, c in pairs:
        h[b] = c
    return h


_rng = np.random.default_rng(3)
# Between two occupied bins that are not neighbours every split gives the same two classes, hence the same variance: a maximiser can
# only be unique where no empty bin lies between occupied ones.  DENSE: such histograms; GAPPED: the plateau case, below.
DENSE = {
    'bimodal': 1 + np.bincount(np.clip(np.concatenate([_rng.normal(40, 12, 90000), _rng.normal(200, 25, 7000)]), 0, 255).astype(np.uint8), minlength=256),
    'three bins': _hist([(99, 500), (100, 30), (101, 80)]),
    'three bins, the middle one heavy': _hist([(127, 3), (128, 1000), (129, 5)]),
    'two bins': _hist([(77, 5), (78, 6)]),
    'a full volume': _hist([(0, 2 ** 31 - 2000), (1, 1000), (2, 999)]),             # weights near 2^31: the products round in float64
}
GAPPED = {
    'three bins': _hist([(10, 500), (100, 30), (250, 80)]),
    'three bins, the middle one heavy': _hist([(0, 3), (128, 1000), (255, 4)]),
    'a full volume': _hist([(0, 2 ** 31 - 2000), (200, 1000), (255, 999)]),
}


@pytest.mark.parametrize('name', sorted(DENSE))
def test_otsu_is_the_exact_maximiser(name):
    hist = DENSE[name]
    exact = _exact_variances(hist)
    best = max(exact)
    assert best > 0 and exact.count(best) == 1                     # the maximiser is unique, so the float64 evaluation has one answer to find
    assert R.otsu(hist) == exact.index(best)
    got = R.otsu_var12(hist)
    assert got.dtype == np.float64 and np.all(np.isfinite(got)) and int(np.argmax(got)) == exact.index(best)


@pytest.mark.parametrize('name', sorted(GAPPED))
def test_otsu_takes_the_first_split_of_a_plateau(name):
    """Empty bins between occupied ones: the exact maximum is attained on one run of splits i .. j with bins i + 1 .. j empty -- the same
    two classes throughout, so float64 computes the same number for each of them -- and the threshold is the first, i."""
    hist = GAPPED[name]
    exact = _exact_variances(hist)
    best = max(exact)
    where = [i for i, v in enumerate(exact) if v == best]
    assert best > 0 and where == list(range(where[0], where[-1] + 1)) and not hist[where[0] + 1:where[-1] + 1].any() and hist[where[0]] > 0
    got = R.otsu_var12(hist)
    assert len(set(got[where].tolist())) == 1 and R.otsu(hist) == where[0]


def test_otsu_of_one_occupied_bin_and_of_nothing():
    """One occupied bin: one class is empty or both means coincide at every split, so every variance is exactly 0 and there is no unique
    maximiser; the contract is the first maximum, t = 0 (skimage returns the image's only value there; vessel_mask's user gets an
    all-foreground or all-background mask either way)."""
    for b in (0, 1, 200, 255):
        hist = _hist([(b, 1234)])
        assert set(_exact_variances(hist)) == {Fraction(0)}
        assert not R.otsu_var12(hist).any() and R.otsu(hist) == 0
    assert R.otsu(np.zeros(256, np.int64)) == 0


def test_hist256_and_binarise_truncate_as_the_reference_does():
    p = np.array([0.0, 0.99, 1.0, 127.5, 127.99, 128.0, 254.999, 255.0, np.nan, np.inf], np.float32)
    h = R.hist256(p)
    assert h.sum() == 8 and h[0] == 2 and h[1] == 1 and h[127] == 2 and h[128] == 1 and h[254] == 1 and h[255] == 1
    assert R.binarise(p, 127.5).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0]
    assert R.binarise(p, 127).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ the host side of the module
def test_argument_checks_come_before_the_device():
    """Every bad argument is a ValueError raised on the host: these run without a GPU.  A host tensor is itself a bad argument."""
    from van_gan_amd import postprocess as P
    mask = torch.zeros(4, 5, 6, dtype=torch.uint8)
    pred = torch.zeros(4, 5, 6)
    for conn in (0, 4, -1, 1.5, '1', None):
        with pytest.raises(ValueError, match='connectivity'):
            P.label_components(mask, conn)
        with pytest.raises(ValueError, match='connectivity'):
            P.vessel_mask(pred, connectivity=conn)
    for ms in (-1, 2.5, None, 'small'):
        with pytest.raises(ValueError, match='min_size'):
            P.remove_small_objects(mask, ms)
        with pytest.raises(ValueError, match='min_size'):
            P.vessel_mask(pred, min_size=ms)
    for thr in ('li', None, float('nan'), float('inf'), True, [1.0], torch.zeros(1), torch.zeros(2)):
        with pytest.raises(ValueError, match='threshold'):
            P.binarise_prediction(pred, thr)
        with pytest.raises(ValueError, match='threshold'):
            P.vessel_mask(pred, thr)
    for fn, good in ((P.label_components, mask), (P.remove_small_objects, mask), (P.binarise_prediction, pred), (P.vessel_mask, pred),
                     (P.histogram256, pred)):
        with pytest.raises(ValueError, match='on the device'):
            fn(good)                                               # a host tensor
        with pytest.raises(ValueError, match='on the device'):
            fn(good.numpy())
        with pytest.raises(ValueError, match=r'\[X,Y,Z\]'):
            fn(good[0])
        with pytest.raises(ValueError, match='must be'):
            fn(good.to(torch.float64))
    assert P._threshold(127.5) == ('f32', 127.5) and P._threshold(100) == ('u8', 100.0) and P._threshold(np.float32(3)) == ('f32', 3.0)
    assert P._threshold(np.int64(7)) == ('u8', 7.0) and P._threshold('otsu') == ('otsu', None)
    assert P._min_size(0) == 0 and P._min_size(np.int64(64)) == 64 and P._min_size(2 ** 40) == 2 ** 32 - 1
    assert [P._connectivity(c) for c in (1, 2, np.int32(3))] == [1, 2, 3]


def test_layout_size_and_tile_checks_need_no_device():
    """Layout, size and the tile limit are checked before the device of the tensor is looked at, so a host tensor (or one on the 'meta'
    device: a shape and strides, no storage) is refused for them, by name."""
    from van_gan_amd import postprocess as P
    big = torch.empty(2 ** 11, 2 ** 10, 2 ** 10, dtype=torch.uint8, device='meta')
    assert big.numel() == 2 ** 31
    for fn in (P.label_components, P.remove_small_objects):
        with pytest.raises(ValueError, match=r'2\^31'):
            fn(big)
        with pytest.raises(ValueError, match='contiguous'):
            fn(torch.zeros(4, 5, 6, dtype=torch.uint8).transpose(0, 2))
    for fn in (P.binarise_prediction, P.vessel_mask, P.histogram256):
        with pytest.raises(ValueError, match=r'2\^31'):
            fn(big.to(torch.float32))
        with pytest.raises(ValueError, match='contiguous'):
            fn(torch.zeros(4, 5, 6).transpose(0, 2))
        with pytest.raises(ValueError, match='contiguous'):
            fn(torch.zeros(4, 5, 12)[..., ::2])
    # one 256-thread workgroup per 8 x 8 x 64 tile and fewer than 2^32 threads in a grid: at most 2^24 - 1 tiles
    assert P.MAX_TILES == 2 ** 24 - 1 and P.label_tiles((37, 29, 70)) == 5 * 4 * 2 and P.label_tiles((8, 8, 64)) == 1 and P.label_tiles((9, 9, 65)) == 8
    for shape in ((2 ** 27, 1, 1), (2 ** 27, 9, 1), (2 ** 24 * 8, 1, 1)):
        thin = torch.empty(shape, dtype=torch.uint8, device='meta')
        assert P.label_tiles(shape) > P.MAX_TILES
        with pytest.raises(ValueError, match='tiles'):
            P.label_components(thin)
        with pytest.raises(ValueError, match='tiles'):
            P.vessel_mask(thin.to(torch.float32))
    ok = torch.empty((2 ** 24 - 1) * 8, 1, 1, dtype=torch.uint8, device='meta')       # the most tiles that are served: refused for its device alone
    with pytest.raises(ValueError, match='on the device'):
        P.label_components(ok)


def test_scratch_arithmetic_through_the_query():
    from van_gan_amd import postprocess as P
    from van_gan_amd._lib import lib, lib_fp16
    for n in (1, 2047, 2048, 2049, 37 * 29 * 70, 512 * 512 * 140, 2 ** 31 - 1):
        want = 64 + 3 * ((4 * n + 15) // 16 * 16) + (4 * ((n + 2047) // 2048) + 15) // 16 * 16
        assert lib.vg_cc_scratch_bytes(n) == want == lib_fp16().vg_cc_scratch_bytes(n)
        assert P.sizes_capacity(n) == n // 2 + 2 >= -(-n // 2) + 1                      # ceil(n / 2) components and the background
    for n in (0, -5, 2 ** 31, 2 ** 40):
        assert lib.vg_cc_scratch_bytes(n) < 0
    # the entries refuse bad arguments on the host before any launch (no GPU here: a launch would fail differently)
    assert lib.vg_cc_label(None, 4, 4, 4, 1, None, None, None, None, 0, None) == -1
    fake = 1 << 20                                                 # non-NULL, aligned, never dereferenced: every call below is refused on the host
    for shape, n in (((2 ** 27, 1, 1), 2 ** 27), ((2 ** 27, 9, 1), 9 * 2 ** 27)):
        assert lib.vg_cc_label(fake, *shape, 1, fake, fake, fake, fake, lib.vg_cc_scratch_bytes(n), None) == -1      # more than 2^24 - 1 tiles
    assert lib.vg_cc_label(fake, 4, 4, 4, 0, fake, fake, fake, fake, 1 << 30, None) == -1 and lib.vg_cc_label(fake, 4, 4, 4, 1, fake, fake, fake, fake, 8, None) == -1
    assert lib.vg_cc_filter(None, 8, None, None, 1, None, None, None, None, None) == -1
    assert lib.vg_hist256(None, 8, None, None, None) == -1
    assert lib.vg_threshold_mask(None, 8, 0, 0.0, None, 0, None, None, None, None, None) == -1
