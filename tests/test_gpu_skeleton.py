"""GPU: the thinning and the degree kernels (csrc/vg_skeleton.hip; van_gan_amd.postprocess skeletonize, skeleton_nodes,
vessel_centreline, vessel_mask(skeleton=True)) against the numpy restatement (tests/skeleton_restate.py, pinned to scipy.ndimage.label
and to the topological invariants on the CPU by tests/test_skeleton_host.py).  Everything is compared by equality: the skeleton, the
voxels each pass deleted, the number of passes and the degree volume.  Nothing here is floating point except the radius along the
centreline, which is a radius the device computed kept or dropped.

Shapes: the smallest at which the kernels can go wrong -- unit axes; odd and even extents on x and y (the parity subfields at the faces
of the volume: a subfield without rows is not launched); Z on both sides of one word (63, 64, 65) and of two (128, 129), where a voxel's
neighbour along z lies in the next word; rows of three and four words (140, 200); the degree kernel cuts a row into pieces of 62 voxels
(63, 65, 128, 129 and 140 are all beside such an edge).  Every volume is a few thousand voxels; a case is some hundred launches."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import components_restate as C  # noqa: E402
import edt_restate as E  # noqa: E402
import skeleton_restate as R  # noqa: E402
from gpu_helpers import DEV, _dev, _engine, _raw, _Recorder  # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 70), (2, 3, 64), (3, 2, 63), (5, 4, 65), (4, 5, 128), (9, 10, 129), (16, 16, 16), (11, 11, 140), (24, 24, 40), (3, 3, 200)]
CONTENTS = ['p0.3', 'p0.6', 'p0.9', 'ones', 'zeros']
CRAFTED = {
    'the z disc of radius 3 across two word edges': lambda: R.disc_along_z((11, 11, 140), 3),
    'crossed tubes with a torus': lambda: R.tubes_and_torus((24, 24, 40)),
    'a hollow shell': lambda: R.hollow_shell(),
    'a plate two voxels thick': lambda: R.plate((2, 12, 12)),
    'a thin diagonal line': lambda: R.diagonal_line((9, 10, 129)),
    'a tube whose axis lies between z = 63 and 64': lambda: R.tube_on_a_word_edge((9, 10, 129)),
}
_ids = dict(ids=lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s))


@functools.lru_cache(maxsize=None)
def _mask(shape, content):
    if content in CRAFTED:
        m = CRAFTED[content]()
    elif content == 'zeros':
        m = np.zeros(shape, np.uint8)
    elif content == 'ones':
        m = np.ones(shape, np.uint8)
    else:
        m = R.bernoulli(shape, float(content[1:]))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref(shape, content, max_passes=None):
    """(skeleton, deleted per pass, degree of the skeleton) of the restatement, computed once"""
    skel, deleted = R.skeletonize(_mask(shape, content), max_passes)
    deg = R.degree(skel)
    skel.setflags(write=False)
    deg.setflags(write=False)
    return skel, deleted, deg


def _check(shape, content):
    from van_gan_amd.postprocess import skeleton_nodes, skeletonize
    m = _mask(shape, content)
    skel, deleted, deg = _ref(m.shape, content)
    md = _dev(m)
    got, info = skeletonize(md, return_info=True)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == m.shape
    assert info == dict(passes=len(deleted), deleted=deleted, converged=True), (shape, content, info, deleted)
    assert np.array_equal(got.cpu().numpy(), skel), (shape, content)
    nodes = skeleton_nodes(got)
    assert nodes.is_cuda and nodes.dtype == torch.uint8 and tuple(nodes.shape) == m.shape
    assert np.array_equal(nodes.cpu().numpy(), deg), (shape, content)
    assert np.array_equal(skeleton_nodes(md).cpu().numpy(), R.degree(m)), (shape, content)      # of a mask that is not thin: up to 26
    assert np.array_equal(md.cpu().numpy(), m)                                      # the mask is only read


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('shape', SHAPES, **_ids)
def test_skeletons_are_the_restatements(shape, content):
    _check(shape, content)


@pytest.mark.parametrize('content', sorted(CRAFTED))
def test_skeletons_of_crafted_masks(content):
    _check(None, content)


def test_what_the_crafted_masks_exercise():
    line = np.zeros((11, 11, 140), np.uint8)
    line[5, 5, 1:139] = 1
    key = 'the z disc of radius 3 across two word edges'
    assert np.array_equal(_ref((11, 11, 140), key)[0], line) and len(_ref((11, 11, 140), key)[1]) == 3
    diag = _mask(None, 'a thin diagonal line')
    assert np.array_equal(_ref(diag.shape, 'a thin diagonal line')[0], diag) and (diag.sum((0, 1)) == 1).all()      # one voxel at every z, the word edges included
    tube = _mask(None, 'a tube whose axis lies between z = 63 and 64')
    assert tube[:, :, 63].any() and tube[:, :, 64].any() and np.array_equal(tube[:, :, 63], tube[:, :, 64])
    deg = _ref((24, 24, 40), 'crossed tubes with a torus')[2]
    assert (deg == 1).sum() >= 2 and (deg >= 3).sum() >= 2
    assert (R.degree(np.ones((3, 3, 3), np.uint8)) == np.array(26, np.uint8)).any()
    assert len(_ref((24, 24, 40), 'ones')[1]) > 8                                   # more than two chunks of four passes


@pytest.mark.parametrize('shape,content', [((9, 10, 129), 'p0.9'), ((16, 16, 16), 'ones'), ((5, 4, 65), 'p0.6'), ((1, 1, 70), 'ones')], **_ids)
def test_a_fixed_number_of_passes(shape, content):
    """max_passes=k: the restatement stopped after k passes; passes after the one that deleted nothing leave 0; nothing is read back
    unless the info is asked for."""
    from van_gan_amd.postprocess import skeletonize
    md = _dev(_mask(shape, content))
    full = _ref(shape, content)
    for k in (1, 2, len(full[1]) + 3):
        skel, deleted, _ = _ref(shape, content, k)
        got, info = skeletonize(md, k, return_info=True)
        assert np.array_equal(got.cpu().numpy(), skel), (shape, content, k)
        assert info == dict(passes=k, deleted=deleted, converged=0 in deleted), (k, info, deleted)
        assert torch.equal(skeletonize(md, max_passes=k), got)
    assert np.array_equal(_ref(shape, content, len(full[1]) + 3)[0], full[0])


def test_chunks_repeats_and_input_types():
    """Thinning in chunks of another size gives the same bits; so do two runs; bool and values other than 1 are taken; [X,Y,Z,1] is."""
    from van_gan_amd import postprocess as P
    shape = (9, 10, 129)
    m = _mask(shape, 'p0.9')
    skel, deleted, _ = _ref(shape, 'p0.9')
    md = _dev(m)
    first = P.skeletonize(md)
    assert np.array_equal(first.cpu().numpy(), skel)
    assert torch.equal(P.skeletonize(md), first)
    for content in ('ones', 'p0.6'):
        a, b = P.skeletonize(_dev(_mask((24, 24, 40), content))), P.skeletonize(_dev(_mask((24, 24, 40), content)))
        assert torch.equal(a, b)
    for chunk in (1, 3, 7):
        old = P.SKELETON_CHUNK
        P.SKELETON_CHUNK = chunk
        try:
            got, info = P.skeletonize(md, return_info=True)
        finally:
            P.SKELETON_CHUNK = old
        assert torch.equal(got, first) and info['deleted'] == deleted, chunk
    assert torch.equal(P.skeletonize(md != 0), first) and torch.equal(P.skeletonize(md * 7), first) and torch.equal(P.skeletonize(md * 255), first)
    assert torch.equal(P.skeletonize(md[..., None]), first)
    assert torch.equal(P.skeleton_nodes(first != 0), P.skeleton_nodes(first * 9))
    with pytest.raises(ValueError, match='contiguous'):
        P.skeletonize(md.transpose(0, 2))
    with pytest.raises(ValueError, match='max_passes'):
        P.skeletonize(md, 0)


def test_entries_directly_scratch_and_refusals():
    """Every entry called raw, as the wrapper calls it: with the scratch its query tells, filled with garbage; continued in a second
    call without repacking; with the counts beside the scratch and in its tail; unpacked to an output that is not 16-byte aligned; with
    one byte less and with bad extents (refused, nothing launched)."""
    from van_gan_amd._lib import lib
    shape = (9, 10, 129)
    X, Y, Z = shape
    n = X * Y * Z
    m = _mask(shape, 'p0.9')
    skel, deleted, deg = _ref(shape, 'p0.9')
    assert len(deleted) == 5
    md = _dev(m)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = int(lib.vg_skeleton_scratch_bytes(X, Y, Z, 3))
    assert nbytes == 2 * (8 * X * Y * 3) + 16
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    beside = torch.full((3,), 77, dtype=torch.int32, device=DEV)
    assert lib.vg_skeleton_begin(md.data_ptr(), X, Y, Z, scratch.data_ptr(), nbytes, st) == 0
    assert lib.vg_skeleton_passes(X, Y, Z, 3, scratch.data_ptr(), nbytes, beside.data_ptr(), st) == 0
    assert beside.cpu().tolist() == deleted[:3]
    part = torch.full((n + 1,), 9, dtype=torch.uint8, device=DEV)[1:]               # not 16-byte aligned: the byte-store kernel
    assert part.data_ptr() % 16 == 1
    assert lib.vg_skeleton_end(X, Y, Z, scratch.data_ptr(), nbytes, part.data_ptr(), st) == 0
    assert np.array_equal(part.cpu().numpy().reshape(shape), _ref(shape, 'p0.9', 3)[0])
    tail = scratch[nbytes - 16:].view(torch.int32)[:3]                              # the room the query leaves behind the two bit volumes
    assert lib.vg_skeleton_passes(X, Y, Z, 3, scratch.data_ptr(), nbytes, tail.data_ptr(), st) == 0      # goes on where the first call stopped
    assert tail.cpu().tolist() == (deleted + [0])[3:6]
    out = torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    assert lib.vg_skeleton_end(X, Y, Z, scratch.data_ptr(), nbytes, out.data_ptr(), st) == 0
    assert np.array_equal(out.cpu().numpy(), skel)
    nodes = torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    assert lib.vg_neighbour_count26(out.data_ptr(), X, Y, Z, nodes.data_ptr(), st) == 0
    assert np.array_equal(nodes.cpu().numpy(), deg)
    before = scratch.clone()
    for bad in ((X, 0, Z), (-1, Y, Z), (X, Y, 0), (2048, 1024, 1024)):
        assert lib.vg_skeleton_scratch_bytes(*bad, 3) < 0
        assert lib.vg_skeleton_begin(md.data_ptr(), *bad, scratch.data_ptr(), nbytes, st) < 0
        assert lib.vg_skeleton_passes(*bad, 3, scratch.data_ptr(), nbytes, beside.data_ptr(), st) < 0
        assert lib.vg_skeleton_end(*bad, scratch.data_ptr(), nbytes, out.data_ptr(), st) < 0
        assert lib.vg_neighbour_count26(md.data_ptr(), *bad, nodes.data_ptr(), st) < 0
    assert lib.vg_skeleton_scratch_bytes(X, Y, Z, 0) < 0
    one = int(lib.vg_skeleton_scratch_bytes(X, Y, Z, 1))
    assert lib.vg_skeleton_begin(md.data_ptr(), X, Y, Z, scratch.data_ptr(), one - 1, st) < 0
    assert lib.vg_skeleton_passes(X, Y, Z, 3, scratch.data_ptr(), nbytes - 1, beside.data_ptr(), st) < 0
    assert lib.vg_skeleton_passes(X, Y, Z, 0, scratch.data_ptr(), nbytes, beside.data_ptr(), st) < 0
    assert lib.vg_skeleton_end(X, Y, Z, scratch.data_ptr(), one - 1, out.data_ptr(), st) < 0
    assert lib.vg_skeleton_begin(None, X, Y, Z, scratch.data_ptr(), nbytes, st) < 0 and lib.vg_neighbour_count26(md.data_ptr(), X, Y, Z, None, st) < 0
    assert torch.equal(scratch, before) and np.array_equal(out.cpu().numpy(), skel) and beside.cpu().tolist() == deleted[:3]      # nothing was launched


# ------------------------------------------------------------------------------------------------ the chained recipes
@functools.lru_cache(maxsize=None)
def _prediction(shape=(40, 33, 50)):
    """Prediction-like: hollow bright tubes on a dark background, fp32 in [0, 255], so that the threshold leaves cavities to close."""
    rng = np.random.default_rng(11)
    v = rng.normal(40.0, 12.0, shape)
    seeds = E.bernoulli(shape, 0.004, seed=5).astype(bool)
    wall, lumen = np.zeros(shape, bool), np.zeros(shape, bool)
    for x, y, z in zip(*np.nonzero(seeds)):
        wall[max(x - 2, 0):x + 3, max(y - 2, 0):y + 3, max(z - 4, 0):z + 5] = True
        lumen[max(x - 1, 0):x + 2, max(y - 1, 0):y + 2, max(z - 3, 0):z + 4] = True
    wall &= ~lumen
    v[wall] = rng.normal(200.0, 10.0, int(wall.sum()))
    p = np.clip(v, 0.0, 255.0).astype(np.float32)
    p.setflags(write=False)
    return p


def test_vessel_centreline_and_vessel_mask_are_the_functions_chained():
    from van_gan_amd.postprocess import fill_holes, skeletonize, vessel_centreline, vessel_mask, vessel_radius
    pd = _dev(_prediction())
    plain = vessel_mask(pd, 127.5, 8, 1)
    want_plain = C.vessel_mask(_prediction(), 127.5, 8, 1)
    assert np.array_equal(plain.cpu().numpy(), want_plain)                          # the default keyword: the bits of before
    filled = fill_holes(plain)
    assert int(filled.sum()) > int(plain.sum())                                     # there are cavities to close
    for sampling in (None, (2.0, 0.5, 1.25)):
        skel, radius = vessel_centreline(plain, sampling)
        assert skel.dtype == torch.uint8 and radius.dtype == torch.float32 and skel.shape == radius.shape == plain.shape
        assert torch.equal(skel, skeletonize(filled)) and torch.equal(radius, vessel_radius(plain, sampling) * skel)
        skel_open, radius_open = vessel_centreline(plain, sampling, fill=False)
        assert torch.equal(skel_open, skeletonize(plain)) and torch.equal(radius_open, vessel_radius(plain, sampling, fill=False) * skel_open)
    skel, radius = vessel_centreline(plain)
    assert np.array_equal(skel.cpu().numpy(), R.skeletonize(E.fill_holes(want_plain))[0])
    assert int(skel_open.sum()) > int(skel.sum())                                   # a hollow lumen leaves a shell of skeleton around its cavity
    assert bool((radius[skel != 0] >= 1).all()) and not bool(radius[skel == 0].any())
    mask, sk = vessel_mask(pd, 127.5, 8, 1, skeleton=True)
    assert torch.equal(mask, plain) and torch.equal(sk, skeletonize(plain))
    mask, info, sk = vessel_mask(pd, 127.5, 8, 1, return_info=True, fill_holes=True, skeleton=True)
    assert torch.equal(mask, filled) and torch.equal(sk, skel) and info == vessel_mask(pd, 127.5, 8, 1, return_info=True)[1]
    ones = torch.ones(4, 5, 6, dtype=torch.uint8, device=DEV)                       # no background: the radius is +inf on the skeleton, 0 off it
    sk1, r1 = vessel_centreline(ones)
    assert bool(torch.isposinf(r1[sk1 != 0]).all()) and not bool(r1[sk1 == 0].any()) and not bool(torch.isnan(r1).any())


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


def _thin_calls(passes_calls):
    return ['vg_skeleton_scratch_bytes', 'vg_skeleton_begin'] + ['vg_skeleton_passes'] * passes_calls + ['vg_skeleton_end']


def test_the_calls_of_every_recipe(monkeypatch):
    """Thinning until nothing changes issues one call of vg_skeleton_passes per four passes the restatement needs; a fixed number of
    passes issues one; vessel_mask with the default keyword issues what it issued before."""
    shape = (9, 10, 129)
    md = _dev(_mask(shape, 'p0.9'))
    passes = len(_ref(shape, 'p0.9')[1])
    assert passes == 5
    assert _calls(monkeypatch, 'skeletonize', md) == _thin_calls(2)
    assert _calls(monkeypatch, 'skeletonize', md, return_info=True) == _thin_calls(2)
    assert _calls(monkeypatch, 'skeletonize', md, 3) == _thin_calls(1) == _calls(monkeypatch, 'skeletonize', md, 300, return_info=True)
    assert _calls(monkeypatch, 'skeletonize', torch.zeros_like(md)) == _thin_calls(1)
    assert _calls(monkeypatch, 'skeleton_nodes', md) == ['vg_neighbour_count26']
    block = _dev(_mask((24, 24, 40), 'ones'))
    assert _calls(monkeypatch, 'skeletonize', block) == _thin_calls(-(-len(_ref((24, 24, 40), 'ones')[1]) // 4))
    pd = _dev(_prediction())
    before = ['vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert _calls(monkeypatch, 'vessel_mask', pd) == before
    assert _calls(monkeypatch, 'vessel_mask', pd, skeleton=False) == before
    assert _calls(monkeypatch, 'vessel_mask', pd, 127.5, 1) == ['vg_threshold_mask']
    assert _calls(monkeypatch, 'vessel_mask', pd, fill_holes=True) == before + FILL_CALLS
    kept = C.vessel_mask(_prediction())
    k = -(-len(R.skeletonize(kept)[1]) // 4)
    assert _calls(monkeypatch, 'vessel_mask', pd, skeleton=True) == before + _thin_calls(k)
    assert _calls(monkeypatch, 'vessel_mask', pd, return_info=True, skeleton=True) == before + _thin_calls(k)
    filled = E.fill_holes(kept)
    kf = -(-len(R.skeletonize(filled)[1]) // 4)
    assert _calls(monkeypatch, 'vessel_mask', pd, fill_holes=True, skeleton=True) == before + FILL_CALLS + _thin_calls(kf)
    md2 = _dev(kept)
    assert _calls(monkeypatch, 'vessel_centreline', md2) == FILL_CALLS + _thin_calls(kf) + EDT_CALLS
    assert _calls(monkeypatch, 'vessel_centreline', md2, (2.0, 0.5, 1.25), fill=False) == _thin_calls(k) + EDT_CALLS
    torch.cuda.synchronize()


def test_segment_mask_with_and_without_the_skeleton(monkeypatch):
    """VanGan.segment_mask: the default keyword hands vessel_mask what it handed before and returns its mask alone; skeleton=True returns
    vessel_mask(..., skeleton=True) of the same prediction (one run of the stitch each: two runs differ in their last bits)."""
    from van_gan_amd import postprocess
    eng = _engine()
    raw = _raw('uint8', (48, 40, 36))
    segment, seen = eng.segment_volume, []

    def recording(gen, raw, subvol_size=None, **kw):
        out = segment(gen, raw, subvol_size, **kw)
        seen.append(out)
        return out
    monkeypatch.setattr(eng, 'segment_volume', recording)
    rec = _Recorder(postprocess.lib)
    monkeypatch.setattr(postprocess, 'lib', rec)
    plain = eng.segment_mask('gen_IS', raw, (32, 32, 32), min_size=4, stride=(8, 8, 4))
    names = [c for c in rec.names if c in ('vg_threshold_mask', 'vg_cc_filter') or c.startswith(('vg_cc_', 'vg_skeleton', 'vg_fill', 'vg_neighbour'))]
    assert names == ['vg_threshold_mask'] + LABEL_CALLS + ['vg_cc_filter']
    assert isinstance(plain, torch.Tensor) and np.array_equal(plain.cpu().numpy(), C.vessel_mask(seen[0].cpu().numpy(), 127.5, 4, 3))
    mask, skel = eng.segment_mask('gen_IS', raw, (32, 32, 32), min_size=4, stride=(8, 8, 4), skeleton=True)
    assert len(seen) == 2
    want = C.vessel_mask(seen[1].cpu().numpy(), 127.5, 4, 3)
    assert np.array_equal(mask.cpu().numpy(), want) and np.array_equal(skel.cpu().numpy(), R.skeletonize(want)[0])
