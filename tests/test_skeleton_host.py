"""CPU: what the GPU suite of the thinning rests on (tests/test_gpu_skeleton.py compares the kernels with tests/skeleton_restate.py by
equality, so the restatement is pinned here to definitions that do not share its code): the two counts of the simple-point test
against scipy.ndimage.label on 3x3x3 windows; whole skeletons against the three topological invariants computed with scipy and numpy
alone; thinness, idempotence and independence of the order inside a sub-step; known answers; the degree against a convolution.  Then
the host side of van_gan_amd.postprocess: the argument checks, which come before any device access, and the scratch arithmetic and
refusals of the library entries, which launch nothing."""
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import skeleton_restate as R

FULL = np.ones((3, 3, 3), bool)
CROSS = ndi.generate_binary_structure(3, 1)
FACE_AT = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]


def _windows(codes):
    """bool [N, 3, 3, 3]: window[dx + 1, dy + 1, dz + 1] is bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1), the centre cleared"""
    w = ((np.asarray(codes, np.int64)[:, None] >> np.arange(27)) & 1).astype(bool).reshape(-1, 3, 3, 3)
    w[:, 1, 1, 1] = False
    return w


def _labels_per_window(windows, structure):
    """int [N, 3, 3, 3]: scipy's labels of every window on its own -- the windows lie in one volume with a slab of background between
    them, so that one call labels them all and no component spans two"""
    N = len(windows)
    vol = np.zeros((N, 4, 3, 3), bool)
    vol[:, :3] = windows
    lab, _ = ndi.label(vol.reshape(N * 4, 3, 3), structure=structure)
    return lab.reshape(N, 4, 3, 3)[:, :3]


def _distinct(lab):
    """per row of int [N, k]: the number of distinct non-zero values"""
    s = np.sort(lab, 1)
    return ((s > 0) & np.concatenate([np.ones((len(s), 1), bool), s[:, 1:] != s[:, :-1]], 1)).sum(1)


def scipy_t26(codes):
    return _distinct(_labels_per_window(_windows(codes), FULL).reshape(len(codes), 27))


def scipy_t6bar(codes):
    n18 = R.N18.reshape(3, 3, 3)
    lab = _labels_per_window(~_windows(codes) & n18, CROSS)
    return _distinct(np.stack([lab[:, a, b, c] for a, b, c in FACE_AT], 1))


def _codes_with_at_most(k, of_background):
    bits = [b for b in range(27) if b != R.CENTRE]
    out = []
    for j in range(k + 1):
        for combo in itertools.combinations(bits, j):
            c = sum(1 << b for b in combo)
            out.append(R.ALL26 - c if of_background else c)
    return np.array(out, np.int64)


def _random_codes(n, density, seed):
    rng = np.random.default_rng(seed)
    bits = rng.random((n, 27)) < density
    bits[:, R.CENTRE] = False
    return (bits.astype(np.int64) << np.arange(27)).sum(1)


def _check_predicate(codes):
    a, b = scipy_t26(codes), scipy_t6bar(codes)
    assert np.array_equal(R.t26(codes), a) and np.array_equal(R.t6bar(codes), b)
    assert np.array_equal(R.simple(codes), (a == 1) & (b == 1))
    return int(((a == 1) & (b == 1)).sum())


def test_the_label_helper_counts_what_single_calls_count():
    codes = _random_codes(300, 0.5, 1)
    for c, a, b in zip(codes, scipy_t26(codes), scipy_t6bar(codes)):
        w = _windows([c])[0]
        assert ndi.label(w, structure=FULL)[1] == a
        lab, _ = ndi.label(~w & R.N18.reshape(3, 3, 3), structure=CROSS)
        assert len({int(lab[p]) for p in FACE_AT} - {0}) == b


def test_the_predicate_on_sparse_and_on_dense_codes():
    few = _codes_with_at_most(3, False)
    assert len(few) == 1 + 26 + 325 + 2600
    assert _check_predicate(few) > 0
    assert _check_predicate(_codes_with_at_most(3, True)) > 0
    assert not R.simple(np.array([0]))[0] and not R.simple(np.array([R.ALL26]))[0]      # an isolated voxel, an interior voxel


@pytest.mark.parametrize('density', [0.2, 0.5, 0.8])
def test_the_predicate_on_random_codes(density):
    n_simple = _check_predicate(_random_codes(200000, density, int(density * 10)))
    assert 0 < n_simple < 200000


def test_the_adjacency_tables():
    assert R.ADJ26[0] == 0x161a and R.ADJ6[1] == 0x410 and R.ADJ26[R.CENTRE] == 0 and R.ADJ6[0] == 0
    # a corner of the window touches 7 of its cells, an edge 11, a face 17 -- the centre, which is no neighbour, among them
    assert [bin(a).count('1') for a in R.ADJ26] == [6, 10, 6, 10, 16, 10, 6, 10, 6, 10, 16, 10, 16, 0, 16, 10, 16, 10, 6, 10, 6, 10, 16, 10, 6, 10, 6]
    assert [bin(a).count('1') for a in R.ADJ6] == [0, 2, 0, 2, 4, 2, 0, 2, 0, 2, 4, 2, 4, 0, 4, 2, 4, 2, 0, 2, 0, 2, 4, 2, 0, 2, 0]
    assert sorted(np.nonzero(R.FACE)[0]) == [4, 10, 12, 14, 16, 22] and R.N18.sum() == 18
    assert all((R.ADJ26[b] >> c) & 1 == (R.ADJ26[c] >> b) & 1 and (R.ADJ6[b] >> c) & 1 == (R.ADJ6[c] >> b) & 1 for b in range(27) for c in range(27))


# ------------------------------------------------------------------------------------------------ whole skeletons
def invariants(m):
    """(26-components of the foreground, 6-components of the background of the padded volume, Euler characteristic V - E + F - C of the
    cubical complex of closed voxels)"""
    p = np.pad(np.asarray(m) != 0, 1)

    def cells(axes):                                                 # the cells shared along these axes that some voxel touches
        q = p
        for a in axes:
            q = q | np.roll(q, 1, a)                                 # the padding keeps the wrap-around empty
        return int(q.sum())
    V, C = cells((0, 1, 2)), cells(())
    E = cells((0, 1)) + cells((0, 2)) + cells((1, 2))
    F = cells((0,)) + cells((1,)) + cells((2,))
    return ndi.label(p, structure=FULL)[1], ndi.label(~p, structure=CROSS)[1], V - E + F - C


def test_the_euler_characteristic_of_known_solids():
    assert invariants(np.ones((3, 4, 5)))[2] == 1 and invariants(np.zeros((3, 4, 5)))[2] == 0
    assert invariants(R.hollow_shell()) == (1, 2, 2) and invariants(R.torus()) == (1, 1, 0)
    two = np.zeros((3, 3, 3), np.uint8)
    two[0, 0, 0] = two[1, 1, 1] = 1                                  # joined through a corner: one component, one complex
    assert invariants(two) == (1, 1, 1)


def _bernoulli_cases():
    return {'p%s %s' % (p, 'x'.join(map(str, s))): R.bernoulli(s, p) for s in ((9, 10, 11), (7, 9, 70), (12, 12, 20), (16, 16, 16)) for p in (0.5, 0.6, 0.7, 0.9)}


def _crafted_cases():
    return {'tubes and torus': R.tubes_and_torus(), 'hollow shell': R.hollow_shell(), 'torus': R.torus(), 'plate': R.plate(), 'diagonal': R.diagonal_line(),
            'tube on a word edge': R.tube_on_a_word_edge(), 'disc': R.disc_along_z(), 'block': np.ones((8, 8, 8), np.uint8)}


CASES = dict(_bernoulli_cases(), **_crafted_cases())


def _deletable(skel):
    """the voxels of skel that a further pass could delete: a background face neighbour, at least two neighbours, simple"""
    m = skel != 0
    p = np.pad(m, 1)
    X, Y, Z = m.shape
    border = np.zeros_like(m)
    for d in R.DIRECTIONS:
        border |= m & ~p[1 + d[0]:1 + d[0] + X, 1 + d[1]:1 + d[1] + Y, 1 + d[2]:1 + d[2] + Z]
    x, y, z = np.nonzero(border)
    codes = R.codes_of(m, x, y, z)
    a, b = scipy_t26(codes), scipy_t6bar(codes)
    n = np.array([bin(int(c)).count('1') for c in codes])
    return int(((a == 1) & (b == 1) & (n >= 2)).sum())


@pytest.mark.parametrize('name', sorted(CASES))
def test_skeletons_keep_the_topology_and_are_thin(name):
    m = CASES[name]
    skel, deleted = R.skeletonize(m)
    assert skel.dtype == np.uint8 and set(np.unique(skel)) <= {0, 1} and deleted[-1] == 0 and all(d > 0 for d in deleted[:-1])
    assert not (skel & ~(m != 0)).any()                              # a subset of the mask
    assert int(m.astype(bool).sum()) - int(skel.sum()) == sum(deleted)
    assert invariants(skel) == invariants(m), name
    assert _deletable(skel) == 0
    again, d2 = R.skeletonize(skel)
    assert np.array_equal(again, skel) and d2 == [0]                 # idempotent
    for k in (1, 2):
        part, dk = R.skeletonize(m, max_passes=k)
        assert dk == (deleted + [0, 0])[:k] and invariants(part) == invariants(m)


@pytest.mark.parametrize('name', ['p0.6 9x10x11', 'p0.9 9x10x11', 'p0.7 7x9x70', 'hollow shell', 'block', 'plate'])
def test_the_order_inside_a_sub_step_does_not_matter(name):
    m = CASES[name]
    want = R.skeletonize(m)
    for order in (+1, -1):
        got = R.skeletonize(m, order=order)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (name, order)


def test_known_answers():
    skel, deleted = R.skeletonize(R.disc_along_z((11, 11, 140), 3))
    line = np.zeros((11, 11, 140), np.uint8)
    line[5, 5, 1:139] = 1
    assert np.array_equal(skel, line) and len(deleted) == 3
    ones = np.ones((1, 1, 70), np.uint8)
    assert np.array_equal(R.skeletonize(ones)[0], ones)
    skel, deleted = R.skeletonize(np.ones((8, 8, 8), np.uint8))
    assert skel.sum() == 2 and len(deleted) == 5
    assert R.skeletonize(np.zeros((3, 4, 5), np.uint8))[1] == [0] and not R.skeletonize(np.zeros((3, 4, 5), np.uint8))[0].any()
    one = np.zeros((3, 4, 5), np.uint8)
    one[1, 2, 3] = 1
    assert np.array_equal(R.skeletonize(one)[0], one) and np.array_equal(R.skeletonize(np.ones((1, 1, 1), np.uint8))[0], np.ones((1, 1, 1), np.uint8))
    shell = R.skeletonize(R.hollow_shell())[0]
    assert invariants(shell)[1] == 2 and shell[6, 6, 6] == 0         # the cavity is still enclosed
    ring = R.skeletonize(R.torus())[0]
    deg = R.degree(ring)
    assert invariants(ring) == (1, 1, 0) and set(np.unique(deg[ring != 0])) == {2}      # one closed curve round the tunnel
    diag = R.diagonal_line()
    assert np.array_equal(R.skeletonize(diag)[0], diag)


def test_degree_is_the_convolution():
    for m in (R.bernoulli((9, 10, 11), 0.5), R.bernoulli((3, 3, 200), 0.9), np.ones((4, 4, 4), np.uint8), np.zeros((2, 3, 4), np.uint8), R.skeletonize(R.tubes_and_torus())[0]):
        conv = ndi.convolve(m.astype(np.int64), np.ones((3, 3, 3), np.int64), mode='constant', cval=0)
        want = np.where(m != 0, conv - 1, 0)
        got = R.degree(m)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    nodes = R.degree(R.skeletonize(R.tubes_and_torus())[0])
    assert (nodes == 1).sum() >= 2 and (nodes >= 3).sum() >= 2       # the tubes end, and they meet the ring


# ------------------------------------------------------------------------------------------------ the host side of the package
def test_argument_checks_come_before_the_device():
    from van_gan_amd import postprocess as P
    mask = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for fn in (P.skeletonize, P.skeleton_nodes, P.vessel_centreline):
        with pytest.raises(ValueError, match='on the device'):
            fn(mask)
        with pytest.raises(ValueError, match='on the device'):
            fn(mask.numpy())
        with pytest.raises(ValueError, match=r'\[X,Y,Z\]'):
            fn(mask[0])
        with pytest.raises(ValueError, match='must be'):
            fn(mask.to(torch.float32))
        with pytest.raises(ValueError, match='contiguous'):
            fn(mask.transpose(0, 2))
        with pytest.raises(ValueError, match=r'2\^31'):
            fn(torch.empty(2 ** 11, 2 ** 10, 2 ** 10, dtype=torch.uint8, device='meta'))
    for bad in (0, -1, 1.5, 'abc', True, (1,)):
        with pytest.raises(ValueError, match='max_passes'):
            P.skeletonize(mask, bad)
    assert P._max_passes(None) is None and P._max_passes(np.int64(3)) == 3
    with pytest.raises(ValueError, match='sampling'):
        P.vessel_centreline(mask, (1.0, 2.0))
    pred = torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match='on the device'):
        P.vessel_mask(pred, skeleton=True)
    with pytest.raises(ValueError, match='connectivity'):
        P.vessel_mask(pred, connectivity=4, skeleton=True)
    import van_gan_amd
    assert van_gan_amd.skeletonize is P.skeletonize and van_gan_amd.skeleton_nodes is P.skeleton_nodes and van_gan_amd.vessel_centreline is P.vessel_centreline


def test_the_entries_refuse_on_the_host():
    from van_gan_amd import _lib, build
    from van_gan_amd._lib import lib, lib_fp16
    from van_gan_amd import postprocess as P
    for name, nargs in (('vg_skeleton_scratch_bytes', 4), ('vg_skeleton_begin', 7), ('vg_skeleton_passes', 8), ('vg_skeleton_end', 7), ('vg_neighbour_count26', 6)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(lib, name) and hasattr(lib_fp16(), name)
    assert 'vg_skeleton.hip' in build.SOURCES and P.SKELETON_MAX_PASSES == 4096

    def al16(b):
        return (b + 15) // 16 * 16
    for shape in ((1, 1, 1), (1, 1, 64), (3, 2, 65), (9, 10, 129), (512, 512, 140), (1, 1, 2 ** 31 - 1), (2 ** 15, 2 ** 15, 1)):
        words = shape[0] * shape[1] * ((shape[2] + 63) // 64)
        for k in (1, 4, 5, 4096):
            assert lib.vg_skeleton_scratch_bytes(*shape, k) == 2 * al16(8 * words) + al16(4 * k) == lib_fp16().vg_skeleton_scratch_bytes(*shape, k)
    assert lib.vg_skeleton_scratch_bytes(512, 512, 140, 4) == 2 * 512 * 512 * 3 * 8 + 16        # 6.3 MB a bit volume
    for shape in ((0, 1, 1), (1, -1, 1), (1, 1, 0), (2048, 1024, 1024), (2 ** 16, 2 ** 15, 1), (2 ** 20, 2 ** 20, 2 ** 20)):
        assert lib.vg_skeleton_scratch_bytes(*shape, 1) < 0
    assert lib.vg_skeleton_scratch_bytes(4, 4, 4, 0) < 0 and lib.vg_skeleton_scratch_bytes(4, 4, 4, -3) < 0 and lib.vg_skeleton_scratch_bytes(4, 4, 4, 4097) < 0
    fake, big = 1 << 20, 1 << 40                                   # non-NULL, aligned, never dereferenced: every call below is refused on the host
    need = lib.vg_skeleton_scratch_bytes(4, 4, 4, 1)
    assert need == 2 * 128 + 16
    assert lib.vg_skeleton_begin(None, 4, 4, 4, fake, big, None) == -1 and lib.vg_skeleton_begin(fake, 4, 4, 4, None, big, None) == -1
    assert lib.vg_skeleton_begin(fake, 4, 0, 4, fake, big, None) == -1 and lib.vg_skeleton_begin(fake, 2048, 1024, 1024, fake, big, None) == -1
    assert lib.vg_skeleton_begin(fake, 4, 4, 4, fake, need - 1, None) == -1 and lib.vg_skeleton_begin(fake, 4, 4, 4, fake + 8, big, None) == -1
    assert lib.vg_skeleton_passes(4, 4, 4, 1, None, big, fake, None) == -1 and lib.vg_skeleton_passes(4, 4, 4, 1, fake, big, None, None) == -1
    assert lib.vg_skeleton_passes(4, 4, 4, 0, fake, big, fake, None) == -1 and lib.vg_skeleton_passes(4, 4, 4, 4097, fake, big, fake, None) == -1
    assert lib.vg_skeleton_passes(4, 4, -4, 1, fake, big, fake, None) == -1 and lib.vg_skeleton_passes(4, 4, 4, 1, fake, big, fake + 2, None) == -1
    assert lib.vg_skeleton_passes(4, 4, 4, 5, fake, lib.vg_skeleton_scratch_bytes(4, 4, 4, 5) - 1, fake, None) == -1
    assert lib.vg_skeleton_passes(4, 4, 4, 5, fake, lib.vg_skeleton_scratch_bytes(4, 4, 4, 4), fake, None) == -1      # sized for fewer passes
    assert lib.vg_skeleton_end(4, 4, 4, None, big, fake, None) == -1 and lib.vg_skeleton_end(4, 4, 4, fake, big, None, None) == -1
    assert lib.vg_skeleton_end(4, 4, 4, fake, need - 1, fake, None) == -1 and lib.vg_skeleton_end(0, 4, 4, fake, big, fake, None) == -1
    assert lib.vg_neighbour_count26(None, 4, 4, 4, fake, None) == -1 and lib.vg_neighbour_count26(fake, 4, 4, 4, None, None) == -1
    assert lib.vg_neighbour_count26(fake, 4, 4, 0, fake, None) == -1 and lib.vg_neighbour_count26(fake, 2048, 1024, 1024, fake, None) == -1
