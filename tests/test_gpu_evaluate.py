"""GPU: scoring a mask against a ground truth (csrc/vg_evaluate.hip: vg_mask_counts, vg_mask_surface, vg_euler_characteristic,
vg_flags_count, vg_masked_stats with vg_masked_stats_scratch_bytes; van_gan_amd.postprocess overlap_counts, mask_surface,
euler_characteristic, betti_numbers, surface_distances, cldice_score, evaluate_segmentation; VanGan.evaluate_volume) against the numpy +
scipy restatement (tests/evaluate_restate.py, pinned on the CPU by tests/test_evaluate_host.py).  Every integer, every order statistic
(an int32 squared distance or the bits of an fp32 distance), the surface volumes and every score formed from integers are compared by
equality.  The fp64 sums are compared within D * 2^-53 * sum, D derived from the reduction below (_sum_depth).

Shapes: the unit axes and Z below the packed width ((1,1,1), (1,1,64), (2,3,5)); the word edge and the last planes ((9,10,129),
(17,9,65)); the labelling tile and one past it ((8,8,64), (9,9,65)); 40x40x131, more than one workgroup per reduction with a tail, also
at an odd offset into a larger buffer so that the unaligned heads of the 16-byte loaders run."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import edt_restate as E  # noqa: E402
import evaluate_restate as R  # noqa: E402
import skeleton_restate as S  # noqa: E402
from gpu_helpers import DEV, _dev, _engine, _raw, _Recorder  # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 64), (2, 3, 5), (9, 10, 129), (17, 9, 65), (8, 8, 64), (9, 9, 65), (40, 40, 131)]
CONTENTS = ['p0.02', 'p0.3', 'p0.5', 'p0.9', 'p0.98', 'zeros', 'ones', 'corner']
CRAFTED = {'torus': S.torus, 'hollow shell': S.hollow_shell, 'tubes and torus': S.tubes_and_torus}
SAMPLING = (0.5, 1.0, 2.5)
BIG = (40, 40, 131)
_ids = dict(ids=lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s))


@functools.lru_cache(maxsize=None)
def _mask(shape, content, seed=0):
    if content in CRAFTED:
        m = CRAFTED[content]()
    elif content == 'zeros':
        m = np.zeros(shape, np.uint8)
    elif content == 'ones':
        m = np.ones(shape, np.uint8)
    elif content == 'corner':
        m = np.zeros(shape, np.uint8)
        m[-1, -1, -1] = 1
    else:
        m = S.bernoulli(shape, float(content[1:]), seed)
    m.setflags(write=False)
    return m


def _other(m):
    """a second mask of the same shape: the first rolled along every axis and cropped"""
    o = np.roll(m, (1, 1, 2), (0, 1, 2)).copy()
    o[..., :1] = 0
    return o


def _st():
    return torch.cuda.current_stream().cuda_stream


def _garbage(n, dtype, fill=0x5A):
    return torch.full((n,), fill, dtype=torch.uint8, device=DEV).view(dtype) if dtype != torch.uint8 else torch.full((n,), fill, dtype=torch.uint8, device=DEV)


def _counts(lib, a, b, n):
    out = _garbage(32, torch.int64)
    assert lib.vg_mask_counts(a, b, n, out.data_ptr(), _st()) == 0
    return tuple(out.tolist())


def _surface(lib, m, shape, surf, nsurf):
    count = _garbage(8, torch.int64)
    assert lib.vg_mask_surface(m, *shape, None if surf is None else surf.data_ptr(), None if nsurf is None else nsurf.data_ptr(), count.data_ptr(), _st()) == 0
    return count.item()


def _cells(lib, m, shape):
    out = _garbage(40, torch.int64)
    assert lib.vg_euler_characteristic(m, *shape, out.data_ptr(), _st()) == 0
    return tuple(out.tolist())


# ------------------------------------------------------------------------------------------------ counts, surface, cells
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_counts_surface_and_cells(shape, content):
    from van_gan_amd._lib import lib
    from van_gan_amd.postprocess import euler_characteristic, mask_surface, overlap_counts
    m = _mask(shape, content)
    o = _other(m)
    md, od = _dev(m), _dev(o)
    n = m.size
    assert _counts(lib, md.data_ptr(), od.data_ptr(), n) == R.counts(m, o) == overlap_counts(md, od)
    assert overlap_counts(md * 255, od != 0) == R.counts(m, o)                       # any non-zero value is foreground; bool is served
    want = R.surface(m)
    surf, nsurf = torch.full(shape, 9, dtype=torch.uint8, device=DEV), torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    assert _surface(lib, md.data_ptr(), shape, surf, nsurf) == int(want.sum())
    assert np.array_equal(surf.cpu().numpy(), want) and np.array_equal(nsurf.cpu().numpy(), 1 - want)
    got, count = mask_surface(md * 7, return_count=True)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want) and count == int(want.sum())
    assert _cells(lib, md.data_ptr(), shape) == R.cells(m)
    assert euler_characteristic(md) == R.euler(m)
    assert np.array_equal(md.cpu().numpy(), m)                                       # the mask is only read


def test_either_output_of_the_surface_entry_may_be_left_out():
    from van_gan_amd._lib import lib, lib_fp16
    shape = (9, 10, 128)
    m = _mask(shape, 'p0.5')
    md, want = _dev(m), R.surface(m)
    surf, nsurf = torch.full(shape, 9, dtype=torch.uint8, device=DEV), torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    assert _surface(lib, md.data_ptr(), shape, surf, None) == int(want.sum()) and np.array_equal(surf.cpu().numpy(), want)
    assert _surface(lib, md.data_ptr(), shape, None, nsurf) == int(want.sum()) and np.array_equal(nsurf.cpu().numpy(), 1 - want)
    assert _surface(lib, md.data_ptr(), shape, None, None) == int(want.sum())
    h = torch.full(shape, 9, dtype=torch.uint8, device=DEV)                          # the fp16 build exports the same code
    assert _surface(lib_fp16(), md.data_ptr(), shape, h, None) == int(want.sum()) and torch.equal(h, surf)
    assert _cells(lib_fp16(), md.data_ptr(), shape) == R.cells(m)


def test_odd_offsets_into_a_larger_buffer():
    """the heads of the 16-byte loaders (both masks equally far from a boundary), their scalar form (not equally far), and the byte forms
    of the surface and cell kernels at a Z that is a multiple of four"""
    from van_gan_amd._lib import lib
    for shape in (BIG, (12, 20, 132)):
        m, o = _mask(shape, 'p0.3'), _other(_mask(shape, 'p0.5'))
        n = m.size
        buf_a, buf_b = torch.zeros(n + 64, dtype=torch.uint8, device=DEV), torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
        for off_a, off_b in ((1, 1), (3, 2), (0, 16), (5, 0), (1, 17)):
            buf_a[off_a:off_a + n] = _dev(m).reshape(-1)
            buf_b[off_b:off_b + n] = _dev(o).reshape(-1)
            a, b = buf_a.data_ptr() + off_a, buf_b.data_ptr() + off_b
            assert _counts(lib, a, b, n) == R.counts(m, o), (shape, off_a, off_b)
        for k in (1, 15, 16, 17, 33):                                                # fewer voxels than a head and a vector
            assert _counts(lib, a, b, k) == R.counts(m.reshape(-1)[:k], o.reshape(-1)[:k]), k
        want = R.surface(m)
        surf = torch.full((n + 1,), 9, dtype=torch.uint8, device=DEV)[1:]
        assert _surface(lib, a, shape, surf, None) == int(want.sum()) and np.array_equal(surf.cpu().numpy().reshape(shape), want)
        assert _cells(lib, a, shape) == R.cells(m)


# ------------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_betti_numbers(shape, content):
    from van_gan_amd.postprocess import betti_numbers
    m = _mask(shape, content)
    assert betti_numbers(_dev(m)) == R.betti(m), (shape, content)


def test_betti_numbers_of_known_shapes_and_of_cavities():
    from van_gan_amd.postprocess import betti_numbers, euler_characteristic
    for name, betti, chi in (('torus', (1, 1, 0), 0), ('hollow shell', (1, 0, 1), 2), ('tubes and torus', (2, 1, 0), 1)):
        md = _dev(_mask(None, name))
        assert betti_numbers(md) == betti and euler_characteristic(md) == chi, name
    assert betti_numbers(_dev(_mask((9, 10, 129), 'p0.3'))) == (8, 825, 3) and betti_numbers(_dev(_mask((17, 9, 65), 'p0.3'))) == (11, 728, 3)
    for name, m in E.hole_cases().items():
        assert betti_numbers(_dev(m)) == R.betti(m), name


def test_flags_count_entry():
    """vg_flags_count directly: the labels 1 .. K whose flag is 0, with K read on the device and capped by the room of the flags"""
    from van_gan_amd._lib import lib
    from van_gan_amd.postprocess import _label, sizes_capacity
    m = E.hole_cases()['nested shells']
    shape, n = m.shape, m.size
    labels, _, result = _label(_dev((m == 0).astype(np.uint8)), shape, 1)
    flags = torch.full((sizes_capacity(n),), 9, dtype=torch.uint8, device=DEV)
    assert lib.vg_fill_holes_mark(labels.data_ptr(), *shape, flags.data_ptr(), _st()) == 0
    out = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    assert lib.vg_flags_count(flags.data_ptr(), result.data_ptr(), n, out.data_ptr(), _st()) == 0
    assert out.item() == R.betti(m)[2] == 2
    K = int(result[0])
    fake = torch.tensor([K + 5, 0, 0, 0], dtype=torch.int32, device=DEV)            # labels past K: their flags are 0 since the mark
    assert lib.vg_flags_count(flags.data_ptr(), fake.data_ptr(), n, out.data_ptr(), _st()) == 0 and out.item() == 2 + 5
    huge = torch.tensor([2 ** 31 - 1, 0, 0, 0], dtype=torch.int32, device=DEV)      # capped at n / 2 + 1: no read leaves the flags
    assert lib.vg_flags_count(flags.data_ptr(), huge.data_ptr(), n, out.data_ptr(), _st()) == 0 and out.item() == 2 + (n // 2 + 1 - K)
    zero = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.vg_flags_count(flags.data_ptr(), zero.data_ptr(), n, out.data_ptr(), _st()) == 0 and out.item() == 0
    for args in ((None, result.data_ptr(), n, out.data_ptr()), (flags.data_ptr(), None, n, out.data_ptr()), (flags.data_ptr(), result.data_ptr(), n, None),
                 (flags.data_ptr(), result.data_ptr(), 0, out.data_ptr()), (flags.data_ptr(), result.data_ptr(), 2 ** 31, out.data_ptr()),
                 (flags.data_ptr(), result.data_ptr() + 2, n, out.data_ptr()), (flags.data_ptr(), result.data_ptr(), n, out.data_ptr() + 1)):
        assert lib.vg_flags_count(*args, _st()) == -1, args


# ------------------------------------------------------------------------------------------------ statistics over a selection
def _sum_depth(n, keys_ptr, sel_ptr):
    """D of the bound |sum - exact| <= D 2^-53 sum: the longest chain of additions of vg_masked_stats as built, plus one.  A thread of
    the reduce kernel adds, one after the other, four values per 16-byte vector it owns and one per head or tail element it owns --
    ceil(nv / threads) vectors and ceil(rest / threads) elements with threads = 256 G, G = min(2048, ceil((nv + rest) / 256)) workgroups
    --; a tree of 8 levels adds the 256 threads; thread t of the final workgroup adds ceil(G / 256) partials, and a tree of 8 levels adds
    those.  Every term is a correctly rounded square root (or an fp32 number), the same as the restatement's; the one more covers the
    rounding of the reference sum."""
    head = (16 - keys_ptr % 16) % 16 // 4
    nv = (n - head) // 4 if (sel_ptr + head) % 4 == 0 and head < n else 0
    rest = n - 4 * nv
    G = min(2048, -(-(nv + rest) // 256))
    threads = 256 * G
    return 4 * -(-nv // threads) + -(-rest // threads) + 8 + -(-G // 256) + 8 + 1


def _stats(lib, keys, sel, kind, qs, fill=0x5A):
    """vg_masked_stats called raw on device tensors, the result block and the scratch full of garbage"""
    n = sel.numel()
    nbytes = int(lib.vg_masked_stats_scratch_bytes(n, len(qs)))
    assert nbytes > 0
    scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    out = torch.full((40,), fill, dtype=torch.uint8, device=DEV)
    assert lib.vg_masked_stats(keys.data_ptr(), sel.data_ptr(), n, kind, (ctypes.c_double * len(qs))(*qs), len(qs), out.data_ptr(), scratch.data_ptr(), nbytes, _st()) == 0
    h = out.cpu().numpy()
    return dict(m=int(h[0:8].view(np.uint64)[0]), max_key=int(h[8:12].view(np.uint32)[0]), pad=int(h[12:16].view(np.uint32)[0]),
                sum=float(h[16:24].view(np.float64)[0]), stats=[int(v) for v in h[24:40].view(np.uint32)])


def _same_stats(got, want, qs, depth, where):
    assert (got['m'], got['max_key'], got['pad']) == (want['m'], want['max_key'], 0), where
    assert got['stats'] == want['stats'] + [0] * (4 - len(qs)), (where, got['stats'], want['stats'])
    assert abs(got['sum'] - want['sum']) <= depth * 2.0 ** -53 * want['sum'], (where, got['sum'], want['sum'], depth)


QS = [0.5, 0.95, 1.0, 0.25]


def _key_cases(n, rng):
    ties = rng.integers(0, 7, n).astype(np.uint32) ** 2
    wide = rng.integers(0, 2 ** 31, n).astype(np.uint32)
    low = (np.uint32(0x12345600) + rng.integers(0, 256, n).astype(np.uint32))
    high = ((rng.integers(0, 128, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00ABCDEF))
    return dict(ties=ties, wide=wide, low_byte=low, high_byte=high)


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 5), (9, 10, 129), BIG], **_ids)
def test_masked_stats_on_integer_keys(shape):
    from van_gan_amd._lib import lib
    n = math.prod(shape)
    rng = np.random.default_rng(n)
    sels = dict(some=(rng.random(n) < 0.3).astype(np.uint8), all=np.full(n, 3, np.uint8), none=np.zeros(n, np.uint8), one=np.zeros(n, np.uint8))
    sels['one'][n // 2] = 255
    for kname, keys in _key_cases(n, rng).items():
        kd = _dev(keys.view(np.int32))
        for sname, sel in sels.items():
            sd = _dev(sel)
            got = _stats(lib, kd, sd, 0, QS)
            _same_stats(got, R.masked_stats(keys, sel, 0, QS), QS, _sum_depth(n, kd.data_ptr(), sd.data_ptr()), (shape, kname, sname))
    m = int(sels['some'].sum())
    if m >= 20:                                                                      # q m an exact integer: rank m / 4 - 1, not m / 4
        sel = sels['some'].copy()
        sel[np.nonzero(sel)[0][m - m % 20:]] = 0
        keys = _key_cases(n, rng)['wide']
        assert int(sel.sum()) % 20 == 0
        got = _stats(lib, _dev(keys.view(np.int32)), _dev(sel), 0, [0.25, 0.05])
        assert got['stats'][:2] == R.masked_stats(keys, sel, 0, [0.25, 0.05])['stats']
        assert got['stats'][0] == int(np.sort(keys[sel != 0])[int(sel.sum()) // 4 - 1])


def test_masked_stats_at_an_odd_offset():
    from van_gan_amd._lib import lib
    n = math.prod(BIG)
    rng = np.random.default_rng(5)
    keys, sel = _key_cases(n, rng)['ties'], (rng.random(n) < 0.4).astype(np.uint8)
    want = R.masked_stats(keys, sel, 0, QS)
    kbuf, sbuf = torch.zeros(n + 8, dtype=torch.int32, device=DEV), torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
    for koff, soff in ((1, 1), (3, 3), (1, 2), (0, 1), (2, 6)):                      # (1, 1), (3, 3), (2, 6): a head, then vectors; else single keys
        kbuf[koff:koff + n] = _dev(keys.view(np.int32))
        sbuf[soff:soff + n] = _dev(sel)
        kd, sd = kbuf[koff:koff + n], sbuf[soff:soff + n]
        _same_stats(_stats(lib, kd, sd, 0, QS), want, QS, _sum_depth(n, kd.data_ptr(), sd.data_ptr()), (koff, soff))


def test_masked_stats_on_the_devices_own_distances():
    """the fp32 kind on what vg_edt writes under a sampling, so that the distance transform's own rounding is not tested again"""
    from van_gan_amd._lib import lib
    from van_gan_amd.postprocess import distance_transform_edt
    for shape in ((9, 10, 129), BIG):
        m = _mask(shape, 'p0.98')
        dist = distance_transform_edt(_dev(m), SAMPLING)
        keys = dist.cpu().numpy().view(np.uint32).reshape(-1)
        sel = _mask(shape, 'p0.3', 1).reshape(-1)
        n = sel.size
        sd = _dev(sel)
        got = _stats(lib, dist, sd, 1, QS)
        _same_stats(got, R.masked_stats(keys, sel, 1, QS), QS, _sum_depth(n, dist.data_ptr(), sd.data_ptr()), shape)
        assert got['max_key'] == int(keys[sel != 0].max()) and got['m'] == int(sel.sum())


def test_masked_stats_refusals():
    from van_gan_amd._lib import lib
    n = 1000
    keys, sel = torch.zeros(n, dtype=torch.int32, device=DEV), torch.ones(n, dtype=torch.uint8, device=DEV)
    nbytes = int(lib.vg_masked_stats_scratch_bytes(n, 4))
    scratch, out = torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV), torch.full((48,), 7, dtype=torch.uint8, device=DEV)
    q = (ctypes.c_double * 4)(0.5, 0.95, 1.0, 0.25)
    good = dict(keys=keys.data_ptr(), sel=sel.data_ptr(), n=n, kind=0, q=q, R=4, out=out.data_ptr(), scratch=scratch.data_ptr(), nbytes=nbytes)
    assert lib.vg_masked_stats(*good.values(), _st()) == 0
    torch.cuda.synchronize()
    out.fill_(7)
    scratch.zero_()
    for kw in (dict(keys=None), dict(sel=None), dict(q=None), dict(out=None), dict(scratch=None), dict(n=0), dict(n=2 ** 31), dict(kind=2), dict(R=0), dict(R=5),
               dict(nbytes=nbytes - 1), dict(scratch=scratch.data_ptr() + 8), dict(keys=keys.data_ptr() + 2), dict(out=out.data_ptr() + 4),
               dict(q=(ctypes.c_double * 4)(0.5, 0.0, 1.0, 1.0)), dict(q=(ctypes.c_double * 4)(0.5, 1.5, 1.0, 1.0)),
               dict(q=(ctypes.c_double * 4)(0.5, float('nan'), 1.0, 1.0))):
        args = dict(good)
        args.update(kw)
        assert lib.vg_masked_stats(*args.values(), _st()) == -1, kw
    assert lib.vg_masked_stats_scratch_bytes(0, 1) < 0 and lib.vg_masked_stats_scratch_bytes(n, 0) < 0 and lib.vg_masked_stats_scratch_bytes(n, 5) < 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and not bool(scratch.any())                        # nothing was launched


def test_refusals_of_the_mask_entries():
    from van_gan_amd._lib import lib
    shape = (4, 5, 8)
    n = math.prod(shape)
    m = torch.ones(shape, dtype=torch.uint8, device=DEV)
    o = torch.full((n + 16,), 9, dtype=torch.uint8, device=DEV)
    w = torch.full((8,), 77, dtype=torch.int64, device=DEV)
    p, q, c = m.data_ptr(), o.data_ptr(), w.data_ptr()
    for args in ((None, p, n, c), (p, None, n, c), (p, p, n, None), (p, p, 0, c), (p, p, 2 ** 31, c), (p, p, n, c + 4)):
        assert lib.vg_mask_counts(*args, _st()) == -1, args
    for args in ((None, 4, 5, 8, q, None, c), (p, 4, 5, 8, q, None, None), (p, 0, 5, 8, q, None, c), (p, 4, 5, -8, q, None, c), (p, 2048, 1024, 1024, q, None, c),
                 (p, 4, 5, 8, p, None, c), (p, 4, 5, 8, None, p + 8, c), (p, 4, 5, 8, q, q + 8, c), (p, 4, 5, 8, q, None, c + 4)):
        assert lib.vg_mask_surface(*args, _st()) == -1, args
    for args in ((None, 4, 5, 8, c), (p, 4, 5, 8, None), (p, 4, 0, 8, c), (p, 2048, 1024, 1024, c), (p, 4, 5, 8, c + 4)):
        assert lib.vg_euler_characteristic(*args, _st()) == -1, args
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((w == 77).all())                            # nothing was launched


# ------------------------------------------------------------------------------------------------ the public functions
def _device_keys(P, T, sampling):
    """the fp32 distances of the device's own transform for both directions, as bit patterns (None without a sampling: exact integers)"""
    if sampling is None:
        return (None, None)
    from van_gan_amd.postprocess import distance_transform_edt
    return tuple(distance_transform_edt(_dev(1 - R.surface(x)), sampling).cpu().numpy().view(np.uint32) for x in (T, P))


def _same_scores(got, want, P, T, sampling, where):
    """got: a dict of the fields.  Equality everywhere except the two means and assd, which hold a sum."""
    depth = _sum_depth(P.size, 0, 0)                                                 # fresh allocations are 16-byte aligned
    for f, w in want.items():
        g = got[f]
        if f in ('pred_to_truth', 'truth_to_pred'):
            assert {k: v for k, v in g.items() if k != 'mean'} == {k: v for k, v in w.items() if k != 'mean'}, (where, f, g, w)
            assert g['mean'] == w['mean'] or abs(g['mean'] - w['mean']) <= (depth + 1) * 2.0 ** -53 * w['mean'], (where, f)       # one more: the division
        elif f == 'assd':
            assert g == w or abs(g - w) <= (depth + 2) * 2.0 ** -53 * w, (where, g, w)                               # the sum of two sums, the division
        elif isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (where, f)
        else:
            assert g == w and type(g) is type(w), (where, f, g, w)


PAIRS = {'shifted tubes and torus': R.shifted_pair, 'bernoulli': lambda: (_mask((9, 10, 129), 'p0.3'), _other(_mask((9, 10, 129), 'p0.3')))}


@pytest.mark.parametrize('pair', sorted(PAIRS))
def test_evaluate_segmentation(pair):
    from van_gan_amd.postprocess import SegmentationScores, cldice_score, evaluate_segmentation, surface_distances
    P, T = PAIRS[pair]()
    pd, td = _dev(P), _dev(T)
    for sampling, percentile in ((None, 95.0), (SAMPLING, 50.0)):
        want = R.evaluate(P, T, sampling, percentile, keys=_device_keys(P, T, sampling))
        got = evaluate_segmentation(pd, td, sampling, percentile)
        assert isinstance(got, SegmentationScores) and set(got.as_dict()) == set(want) == set(SegmentationScores.FIELDS)
        _same_scores(got.as_dict(), want, P, T, sampling, (pair, sampling))
        part = surface_distances(pd, td, sampling, percentile)
        assert part == {k: got.as_dict()[k] for k in part}                           # the same launches: the same bits
    assert cldice_score(pd, td) == {k: want[k] for k in ('skeleton_pred', 'skeleton_truth', 'skeleton_pred_in_truth', 'skeleton_truth_in_pred', 'tprec', 'tsens', 'cldice')}
    bare = evaluate_segmentation(pd != 0, td * 255, topology=False, surface=False, cldice=False)
    assert bare.dice == want['dice'] and bare.tp == want['tp'] and bare.cldice is None and bare.betti_pred is None and bare.hausdorff is None and bare.assd is None
    two = evaluate_segmentation(pd, td, max_passes=2, topology=False, surface=False)
    assert two.as_dict()['cldice'] == R.cldice(P, T, 2)['cldice'] and two.skeleton_pred == R.cldice(P, T, 2)['skeleton_pred']
    if pair.startswith('shifted'):                                                   # the known answers
        assert (got.tp, got.fp, got.fn, got.tn) == (856, 362, 401, 21421) and got.dice == 1712 / 2475 and (got.surface_truth, got.surface_pred) == (862, 838)
        first = evaluate_segmentation(pd, td)
        assert (first.truth_to_pred['max_key'], first.pred_to_truth['max_key']) == (10, 2) and first.hausdorff == math.sqrt(10)
        assert (first.tprec, first.tsens, first.cldice) == (0.9795918367346939, 0.9504950495049505, 0.964824120603015)
        assert first.betti_truth == (2, 1, 0) and first.euler_truth == 1


def test_degenerate_cases():
    from van_gan_amd.postprocess import evaluate_segmentation
    shape = (5, 6, 12)
    z, m, full = np.zeros(shape, np.uint8), _mask(shape, 'p0.3'), np.ones(shape, np.uint8)
    for sampling in (None, SAMPLING):
        both = evaluate_segmentation(_dev(z), _dev(z), sampling)
        assert all(getattr(both, k) == 1.0 for k in ('dice', 'iou', 'precision', 'recall', 'cldice', 'tprec', 'tsens', 'specificity', 'accuracy'))
        assert both.hausdorff == both.hausdorff_percentile == both.assd == 0.0 and both.pred_to_truth['mean'] == 0.0 and both.pred_to_truth['count'] == 0
        assert both.betti_pred == (0, 0, 0) and both.euler_error == 0
        for P, T in ((z, m), (m, z)):
            one = evaluate_segmentation(_dev(P), _dev(T), sampling)
            _same_scores(one.as_dict(), R.evaluate(P, T, sampling, keys=_device_keys(P, T, sampling)), P, T, sampling, 'one empty')
            assert all(getattr(one, k) == 0.0 for k in ('dice', 'iou', 'precision', 'recall', 'cldice'))
            assert one.hausdorff == one.hausdorff_percentile == one.assd == math.inf and one.pred_to_truth['max'] == math.inf
    same = evaluate_segmentation(_dev(full), _dev(full))
    assert math.isnan(same.specificity) and same.dice == same.cldice == 1.0 and same.hausdorff == 0.0 and same.assd == 0.0
    a, b = np.zeros((3, 3, 9), np.uint8), np.zeros((3, 3, 9), np.uint8)
    a[1, 1, 0:3] = 1
    b[1, 1, 6:9] = 1
    apart = evaluate_segmentation(_dev(a), _dev(b))
    assert apart.dice == 0.0 and apart.tprec == apart.tsens == 0.0 and math.isnan(apart.cldice) and apart.hausdorff == 6.0


LABEL = ['vg_cc_scratch_bytes', 'vg_cc_label']
THIN = ['vg_skeleton_scratch_bytes', 'vg_skeleton_begin', 'vg_skeleton_passes', 'vg_skeleton_end']
TOPOLOGY = ['vg_euler_characteristic'] + LABEL * 2 + ['vg_fill_holes_mark', 'vg_flags_count']
DISTANCES = ['vg_edt_scratch_bytes', 'vg_edt', 'vg_masked_stats_scratch_bytes', 'vg_masked_stats']
SURFACE = ['vg_mask_surface'] * 2 + DISTANCES * 2


def test_everything_is_enqueued_before_the_one_read_back(monkeypatch):
    """the entries in the order they are enqueued, and one copy to the host in the whole call (thinning by a fixed number of passes;
    thinning until nothing changes reads its counts back, as skeletonize does)"""
    from van_gan_amd import postprocess
    P, T = R.shifted_pair()
    pd, td = _dev(P), _dev(T)
    torch.cuda.synchronize()
    rec = _Recorder(postprocess.lib)
    reads = []
    cpu, item, tolist = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(postprocess, 'lib', rec)
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: (reads.append((len(rec.names), t.numel())), cpu(t, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, 'item', lambda t: (reads.append((len(rec.names), 'item')), item(t))[1])
    monkeypatch.setattr(torch.Tensor, 'tolist', lambda t: (reads.append((len(rec.names), 'tolist')), tolist(t))[1])
    try:
        postprocess.evaluate_segmentation(pd, td, SAMPLING, max_passes=3)
        full, full_reads = list(rec.names), list(reads)
        del rec.names[:], reads[:]
        postprocess.evaluate_segmentation(pd, td, cldice=False)
        plain, plain_reads = list(rec.names), list(reads)
    finally:
        monkeypatch.undo()
    assert full == ['vg_mask_counts'] + (THIN + ['vg_mask_counts']) * 2 + TOPOLOGY * 2 + SURFACE
    assert plain == ['vg_mask_counts'] + TOPOLOGY * 2 + SURFACE
    assert len(full_reads) == 1 and full_reads[0][0] == len(full) and full_reads[0][1] <= 512           # one small block, after the last entry
    assert len(plain_reads) == 1 and plain_reads[0][0] == len(plain)


def test_two_runs_give_the_same_bits():
    from van_gan_amd.postprocess import evaluate_segmentation
    for P, T in (R.shifted_pair(), (_mask(BIG, 'p0.3'), _other(_mask(BIG, 'p0.5')))):
        pd, td = _dev(P), _dev(T)
        for sampling in (None, SAMPLING):
            a, b = (evaluate_segmentation(pd, td, sampling, cldice=P.size < 50000).as_dict() for _ in range(2))
            assert repr(a) == repr(b) and a['assd'] > 0.0, sampling                  # repr: bit for bit, and a nan equals itself


def test_wrong_arguments_before_the_device():
    from van_gan_amd import postprocess as P
    md = _dev(_mask((5, 4, 65), 'p0.3'))
    pairs = (P.overlap_counts, P.surface_distances, P.cldice_score, P.evaluate_segmentation)
    for fn in pairs:
        for bad, match in ((md.to(torch.int32), 'must be'), (md.cpu(), 'on the device'), (md[0], r'\[X,Y,Z\]'), (md.transpose(0, 1), 'contiguous')):
            with pytest.raises(ValueError, match=match):
                fn(bad, md)
            with pytest.raises(ValueError, match=match):
                fn(md, bad)
        with pytest.raises(ValueError, match='truth has shape'):
            fn(md, md[:, :, :64].contiguous())
    for fn in (P.mask_surface, P.euler_characteristic, P.betti_numbers):
        for bad, match in ((md.to(torch.int32), 'must be'), (md.cpu(), 'on the device'), (md[0], r'\[X,Y,Z\]'), (md.transpose(0, 1), 'contiguous')):
            with pytest.raises(ValueError, match=match):
                fn(bad)
    for fn in (P.surface_distances, P.evaluate_segmentation):
        with pytest.raises(ValueError, match='percentile'):
            fn(md, md, None, 0.0)
        with pytest.raises(ValueError, match='percentile'):
            fn(md, md, None, 101)
        with pytest.raises(ValueError, match='sampling'):
            fn(md, md, (1.0, 2.0))
    with pytest.raises(ValueError, match='max_passes'):
        P.evaluate_segmentation(md, md, max_passes=0)
    with pytest.raises(ValueError, match='max_passes'):
        P.cldice_score(md, md, max_passes='all')


def test_evaluate_volume_is_segment_mask_then_evaluate_segmentation(monkeypatch):
    from van_gan_amd import postprocess
    eng = _engine()
    raw = _raw('uint8', (48, 40, 36))
    truth = _dev(S.bernoulli((48, 40, 36), 0.4))
    segment_mask, seen = eng.segment_mask, []

    def recording(gen, raw, subvol_size=None, **kw):
        out = segment_mask(gen, raw, subvol_size, **kw)
        seen.append((kw, out))
        return out
    monkeypatch.setattr(eng, 'segment_mask', recording)
    mask, scores = eng.evaluate_volume('gen_IS', raw, truth, (32, 32, 32), sampling=SAMPLING, percentile=90.0, min_size=4, stride=(8, 8, 4))
    assert len(seen) == 1
    kw, made = seen[0]
    assert kw == dict(threshold=127.5, min_size=4, connectivity=3, fill_holes=False, stride=(8, 8, 4)) and made is mask
    want = postprocess.evaluate_segmentation(mask, truth, SAMPLING, 90.0)
    assert isinstance(scores, postprocess.SegmentationScores) and repr(scores.as_dict()) == repr(want.as_dict())
    assert scores.tp + scores.fp == int(mask.sum()) and scores.tp + scores.fn == int(truth.sum()) and scores.voxels == 48 * 40 * 36
    with pytest.raises(ValueError, match='percentile'):
        eng.evaluate_volume('gen_IS', raw, truth, (32, 32, 32), percentile=0)
    with pytest.raises(ValueError, match='truth must be'):
        eng.evaluate_volume('gen_IS', raw, truth.float(), (32, 32, 32))
    assert len(seen) == 1                                                            # refused before anything ran
