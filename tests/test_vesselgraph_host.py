"""CPU: what the GPU suite of the vessel graph rests on (tests/test_gpu_vesselgraph.py compares the kernels with
tests/vesselgraph_restate.py by equality, so the restatement is pinned here to things that share no code with it): a sequential tracer
that walks every segment voxel by voxel; the invariants of the definitions (include/vangan_hip.h "The vessel graph"); the fixed-point
radius against the plain fp64 mean; pruning against the topological invariants of tests/test_skeleton_host.py; known answers.  Then the
host side of van_gan_amd.postprocess: the argument checks, which come before any device access, and the refusals of the library
entries, which launch nothing."""
import functools
import math

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import skeleton_restate as S
import vesselgraph_restate as G
from test_skeleton_host import invariants

FULL = np.ones((3, 3, 3), bool)
SAMPLING = (0.5, 2.0, 3.0)


@functools.lru_cache(maxsize=None)
def _masks():
    """the five masks of the pruning and invariant checks: three skeletons and two raw random masks"""
    out = {'skeleton of tubes and torus': S.skeletonize(S.tubes_and_torus())[0], 'skeleton of p0.6 12x12x20': S.skeletonize(S.bernoulli((12, 12, 20), 0.6))[0],
           'skeleton of the torus': S.skeletonize(S.torus())[0], 'raw p0.1 9x10x129': S.bernoulli((9, 10, 129), 0.1), 'raw p0.3 5x4x65': S.bernoulli((5, 4, 65), 0.3)}
    for m in out.values():
        m.setflags(write=False)
    return out


MASKS = sorted(_masks())


@functools.lru_cache(maxsize=None)
def _graph(name, sampling=None):
    return G.graph(_masks()[name], None, sampling)


# ------------------------------------------------------------------------------------------------ the tracer
def trace(mask, sampling=None):
    """[(node a, node b, voxels, length, a voxel of the segment)] by walking: from every (node voxel, adjacent segment voxel) pair along
    the voxels with two neighbours to the next node voxel, summing Euclidean steps in fp64; then every cycle from its smallest voxel
    (nodes 0, 0).  Python sets and loops only; the nodes are numbered by scipy."""
    m = np.asarray(mask) != 0
    s = np.ones(3) if sampling is None else np.asarray(sampling, np.float64)
    fg = {tuple(int(c) for c in p) for p in np.argwhere(m)}

    def nbrs(p):
        return [q for q in ((p[0] + dx, p[1] + dy, p[2] + dz) for dx, dy, dz in G.OFFSETS) if q in fg]
    around = {p: nbrs(p) for p in fg}
    B = {p for p in fg if len(around[p]) == 2}
    nodes = np.zeros(m.shape, bool)
    for p in fg - B:
        nodes[p] = True
    label = ndi.label(nodes, structure=FULL)[0]

    def dist(p, q):
        return math.sqrt(sum(((a - b) * w) ** 2 for a, b, w in zip(p, q, s)))
    seen, out = set(), []
    for q in sorted(fg - B):
        for p in around[q]:
            if p not in B or p in seen:
                continue
            prev, cur, length, count = q, p, dist(q, p), 0
            while True:
                count += 1
                seen.add(cur)
                a, b = around[cur]
                nxt = b if a == prev else a
                length += dist(cur, nxt)
                if nxt not in B:
                    out.append((int(label[q]), int(label[nxt]), count, length, p))
                    break
                prev, cur = cur, nxt
    for start in sorted(B):
        if start in seen:
            continue
        prev, cur, length, count = around[start][0], start, 0.0, 0
        while True:
            count += 1
            seen.add(cur)
            a, b = around[cur]
            nxt = b if a == prev else a
            length += dist(cur, nxt)
            if nxt == start:
                out.append((0, 0, count, length, start))
                break
            prev, cur = cur, nxt
    assert seen == B
    return out


@pytest.mark.parametrize('sampling', [None, SAMPLING], ids=['unit', 'anisotropic'])
@pytest.mark.parametrize('name', MASKS)
def test_the_tracer_finds_the_same_segments(name, sampling):
    g = _graph(name, sampling)
    walked = trace(_masks()[name], sampling)
    assert len(walked) == g['E']
    assert sorted((min(a, b), max(a, b), k) for a, b, k, _, _ in walked) == \
        sorted((int(min(n)), int(max(n)), int(k)) for n, k in zip(g['seg_nodes'][1:], g['seg_voxels'][1:]))
    for a, b, k, length, p in walked:
        e = int(g['segment_labels'][p])
        assert {a, b} == {int(v) for v in g['seg_nodes'][e]} and k == g['seg_voxels'][e]
        steps = k + 1
        assert abs(g['seg_length'][e] - length) <= steps * 2.0 ** -52 * length, (name, e, g['seg_length'][e], length)


# ------------------------------------------------------------------------------------------------ invariants
def _graph_components(g):
    """connected components of the graph: union-find over seg_nodes, plus the cycles, plus (through their own root) the nodes without
    a segment"""
    parent = list(range(g['V'] + 1))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    cycles = 0
    for a, b in g['seg_nodes'][1:]:
        if a == 0:
            cycles += 1
        else:
            parent[find(int(a))] = find(int(b))
    return len({find(i) for i in range(1, g['V'] + 1)}) + cycles


@pytest.mark.parametrize('name', MASKS)
def test_the_invariants_of_the_definitions(name):
    m = _masks()[name] != 0
    g = _graph(name)
    seg, node = g['segment_labels'], g['node_labels']
    assert ((seg > 0) ^ (node > 0))[m].all() and not (seg[~m].any() or node[~m].any())      # every voxel of S in exactly one segment or node
    assert np.array_equal(g['degree'], S.degree(m)) and ((g['degree'] == 2) == (seg > 0)).all()
    assert set(np.unique(g['attachments'][1:])) <= {0, 2}
    path = g['attachments'] == 2
    rows = g['seg_half_steps'].sum(1)
    assert np.array_equal(rows[1:], np.where(path, 2 * (g['seg_voxels'] + 1), 2 * g['seg_voxels'])[1:]) and not g['seg_half_steps'][0].any()
    assert int(g['node_degree'].sum()) == 2 * int(path.sum())
    assert np.array_equal(path[1:], g['seg_ends'][1:, 0] >= 0) and np.array_equal(path[1:], g['seg_nodes'][1:, 0] > 0)
    assert _graph_components(g) == ndi.label(m, structure=FULL)[1]
    assert int(g['seg_voxels'].sum()) + int(g['node_voxels'].sum()) == int(m.sum())
    # two different nodes are never adjacent: dilating one node's voxels meets no other node
    for k in range(1, min(g['V'], 40) + 1):
        assert set(np.unique(node[ndi.binary_dilation(node == k, structure=FULL)])) <= {0, k}
    kinds = g['node_kind'][1:]
    assert np.array_equal(kinds == G.ISOLATED, (g['node_voxels'][1:] == 1) & (g['node_degree'][1:] == 0))
    assert np.array_equal(kinds == G.END, (g['node_voxels'][1:] == 1) & (g['node_degree'][1:] == 1))
    com = np.array(ndi.center_of_mass(m, node, np.arange(1, g['V'] + 1))).reshape(-1, 3)
    assert np.allclose(g['node_centroid'][1:], com, rtol=0, atol=1e-9)


def test_the_counts_the_issue_names():
    g = G.graph(S.bernoulli((9, 10, 129), 0.1, seed=3))              # seed 0 gives (223, 337, 3, 114)
    loops = int(((g['seg_nodes'][1:, 0] == g['seg_nodes'][1:, 1]) & (g['seg_nodes'][1:, 0] > 0)).sum())
    assert (g['E'], g['V'], int((g['attachments'][1:] == 0).sum()), loops) == (193, 330, 9, 92)


# ------------------------------------------------------------------------------------------------ radius
@pytest.mark.parametrize('sampling', [None, SAMPLING], ids=['unit', 'anisotropic'])
def test_the_fixed_point_mean_radius(sampling):
    mask = S.tubes_and_torus()
    skel = S.skeletonize(mask)[0]
    radius = ndi.distance_transform_edt(mask, sampling=sampling).astype(np.float32)
    g = G.graph(skel, radius, sampling)
    k, D = G.radius_scale(skel.shape, sampling)
    n = skel.size
    assert 2.0 ** k * D * n <= 2.0 ** 62 and k == 62 - math.ceil(math.log2(n)) - math.ceil(math.log2(D))       # the sums fit an int64
    assert g['bad'] == 0 and g['E'] > 3
    for e in range(1, g['E'] + 1):
        r = radius[g['segment_labels'] == e].astype(np.float64)
        assert abs(g['seg_radius_mean'][e] - r.mean()) <= 2.0 ** -(k + 1) + 4 * np.spacing(r.mean())
        assert g['seg_radius_min'][e] == r.min() and g['seg_radius_max'][e] == r.max()
    assert g['seg_radius_mean'][0] == 0 and g['seg_radius_min'].dtype == np.float32
    spoilt = radius.copy()
    b = np.argwhere(g['segment_labels'] > 0)
    spoilt[tuple(b[0])], spoilt[tuple(b[1])], spoilt[tuple(b[2])], spoilt[tuple(b[3])] = np.nan, np.inf, -1.0, np.float32(2 * D)
    assert G.graph(skel, spoilt, sampling)['bad'] == 4


# ------------------------------------------------------------------------------------------------ pruning
@pytest.mark.parametrize('min_length', [2.5, 6, 1e9])
@pytest.mark.parametrize('name', MASKS)
def test_pruning_keeps_the_topology(name, min_length):
    m = _masks()[name]
    before = invariants(m)
    cur = m
    for rounds in (1, 3):
        out, info = G.prune(m, min_length, None, rounds)
        assert out.dtype == np.uint8 and not (out & ~(m != 0)).any()
        assert int((m != 0).sum()) - int(out.sum()) == sum(info['voxels']) and info['rounds'] == len(info['spurs']) <= rounds
        got = invariants(out)
        assert (got[0], got[2]) == (before[0], before[2]), (name, min_length, rounds)
        cur = out
    g0, g1 = _graph(name), G.graph(cur)
    assert int((g1['attachments'][1:] == 0).sum()) >= int((g0['attachments'][1:] == 0).sum())        # cycles are kept (a ring that loses its tail becomes one)


@pytest.mark.parametrize('name', MASKS)
def test_pruning_everything_is_idempotent(name):
    out, info = G.prune(_masks()[name], 1e9, None, 1000)
    assert info['voxels'][-1] == 0 and info['rounds'] < 1000
    again, info2 = G.prune(out, 1e9, None, 5)
    assert np.array_equal(again, out) and info2 == dict(rounds=1, spurs=[0], voxels=[0])
    g = G.graph(out)
    n0, n1 = g['seg_nodes'][:, 0], g['seg_nodes'][:, 1]
    assert not ((n0 > 0) & ((g['node_kind'][n0] == G.END) != (g['node_kind'][n1] == G.END)))[1:].any()      # no spur of any length is left


def test_pruning_that_removes_nothing_and_the_copy():
    m = _masks()['raw p0.3 5x4x65']
    out, info = G.prune(m * 5, 0.0, None, 3)
    assert np.array_equal(out, (m != 0).astype(np.uint8)) and info == dict(rounds=0, spurs=[], voxels=[])
    total = sum(G.prune(_masks()[n], 1e9)[1]['voxels'][0] for n in MASKS)
    assert total > 0                                                 # the five masks do have spurs


# ------------------------------------------------------------------------------------------------ known answers
STEPS = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]         # STEPS[c] is a step of class c


@pytest.mark.parametrize('c', range(7))
def test_a_straight_line_along_every_step_class(c):
    L = 9
    assert G.step_class(*STEPS[c]) == c
    g = G.graph(G.line(L, STEPS[c]), None, SAMPLING)
    l = math.sqrt(sum((d * w) ** 2 for d, w in zip(STEPS[c], SAMPLING)))
    assert (g['E'], g['V']) == (1, 2) and g['seg_voxels'][1] == L - 2 and list(g['node_kind'][1:]) == [G.END, G.END]
    want = np.zeros(7, np.int64)
    want[c] = 2 * (L - 1)
    assert np.array_equal(g['seg_half_steps'][1], want) and g['seg_length'][1] == (L - 1) * l == g['seg_chord'][1]
    assert list(g['seg_nodes'][1]) == [1, 2] and list(g['node_degree']) == [0, 1, 1] and list(g['node_voxels']) == [0, 1, 1]
    mirrored = G.graph(G.line(L, STEPS[c])[::-1, ::-1, ::-1].copy(), None, SAMPLING)
    assert mirrored['seg_length'][1] == g['seg_length'][1]


def test_the_crafted_skeletons():
    ring = G.graph(S.skeletonize(S.torus())[0])
    assert (ring['E'], ring['V']) == (1, 0) and ring['seg_voxels'][1] == 36 and list(ring['seg_ends'][1]) == [-1, -1] and list(ring['seg_nodes'][1]) == [0, 0]
    assert ring['seg_chord'][1] == 0 and ring['seg_half_steps'][1].sum() == 72
    disc = G.graph(S.skeletonize(S.disc_along_z())[0])
    assert (disc['E'], disc['V']) == (1, 2) and disc['seg_voxels'][1] == 136 and list(disc['node_kind'][1:]) == [G.END, G.END]
    assert disc['seg_length'][1] == 137.0 == disc['seg_chord'][1]


def test_small_known_answers():
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1, 1] = 1
    g = G.graph(one)
    assert (g['E'], g['V']) == (0, 1) and list(g['node_kind']) == [0, G.ISOLATED] and list(g['node_centroid'][1]) == [1, 1, 1]
    assert g['seg_half_steps'].shape == (1, 7) and g['seg_length'].shape == (1,)
    two = one.copy()
    two[2, 2, 2] = 1
    g = G.graph(two)
    assert (g['E'], g['V']) == (0, 1) and list(g['node_kind']) == [0, G.OTHER] and g['node_voxels'][1] == 2 and list(g['node_centroid'][1]) == [1.5, 1.5, 1.5]
    empty = G.graph(np.zeros((2, 3, 4), np.uint8))
    assert (empty['E'], empty['V']) == (0, 0) and empty['node_kind'].shape == (1,) and G.summary(empty)['total_length'] == 0.0
    block = G.graph(np.ones((4, 4, 4), np.uint8))
    assert (block['E'], block['V']) == (0, 1) and block['node_voxels'][1] == 64 and list(block['node_centroid'][1]) == [1.5, 1.5, 1.5]
    loop = G.graph(G.ring_with_tail())
    assert (loop['E'], loop['V']) == (2, 2) and sorted(loop['node_kind'][1:]) == [G.END, G.OTHER]
    ring = int(np.argmax(loop['seg_voxels']))
    j = int(np.nonzero(loop['node_kind'] == G.OTHER)[0][0])
    assert list(loop['seg_nodes'][ring]) == [j, j] and loop['seg_voxels'][ring] == 11 and loop['seg_chord'][ring] == 0 and loop['node_degree'][j] == 3
    assert loop['seg_ends'][ring][0] == loop['seg_ends'][ring][1] >= 0
    s = G.summary(loop)
    assert (s['segments'], s['cycles'], s['loops'], s['nodes'], s['end_points'], s['junctions'], s['isolated']) == (2, 0, 1, 2, 1, 1, 0)
    assert s['mean_tortuosity'] == 1.0 and s['mean_radius'] is None                  # the tail alone has a chord
    br = G.graph(G.bridge())
    assert (br['E'], br['V']) == (5, 6) and sorted(br['node_kind'][1:]) == [1, 1, 1, 1, 2, 2] and list(br['seg_voxels'][1:]) == [1] * 5
    mid = int(br['segment_labels'][2, 2, 3])
    assert list(br['node_kind'][br['seg_nodes'][mid]]) == [G.OTHER, G.OTHER] and br['seg_length'][mid] == 2.0 == br['seg_chord'][mid]


def test_the_tee_and_its_spur():
    g = G.graph(G.tee())
    assert (g['E'], g['V']) == (3, 4) and sorted(g['node_kind'][1:]) == [1, 1, 1, 2] and sorted(g['seg_voxels'][1:]) == [2, 4, 4]
    assert sorted(g['seg_length'][1:]) == [3.0, 4 + math.sqrt(2), 4 + math.sqrt(2)]
    out, info = G.prune(G.tee(), 4.5)
    assert np.array_equal(out, G.tee_bar()) and info == dict(rounds=1, spurs=[1], voxels=[3])
    assert np.array_equal(G.prune(G.tee(), 3.0)[0], G.tee())         # not shorter than its own length
    after = G.graph(out)
    assert (after['E'], after['V']) == (1, 2) and after['seg_voxels'][1] == 9     # the junction became a voxel of the bar
    gone, info = G.prune(G.tee(), 1e9, None, 5)                      # with no bound on the length every arm is a spur: the apex alone stays
    assert info['spurs'][0] == 3 and int(gone.sum()) == 1 and info['voxels'][-1] == 0


# ------------------------------------------------------------------------------------------------ the host side of the package
def test_argument_checks_come_before_the_device():
    import van_gan_amd
    from van_gan_amd import postprocess as P
    mask = torch.zeros(4, 5, 6, dtype=torch.uint8)
    calls = (lambda m: P.skeleton_graph(m), lambda m: P.prune_spurs(m, 3.0), lambda m: P.vessel_graph(m))
    for fn in calls:
        with pytest.raises(ValueError, match='on the device'):
            fn(mask)
        with pytest.raises(ValueError, match='on the device|torch tensor'):
            fn(mask.numpy())
        with pytest.raises(ValueError, match=r'\[X,Y,Z\]'):
            fn(mask[0])
        with pytest.raises(ValueError, match='must be'):
            fn(mask.to(torch.float32))
        with pytest.raises(ValueError, match='contiguous'):
            fn(mask.transpose(0, 2))
        with pytest.raises(ValueError, match=r'2\^31'):
            fn(torch.empty(2 ** 11, 2 ** 10, 2 ** 10, dtype=torch.uint8, device='meta'))
    with pytest.raises(ValueError, match='tiles'):
        P.skeleton_graph(torch.empty(2 ** 27, 1, 1, dtype=torch.uint8, device='meta'))
    for fn in (lambda s: P.skeleton_graph(mask, None, s), lambda s: P.prune_spurs(mask, 3.0, s), lambda s: P.vessel_graph(mask, s)):
        with pytest.raises(ValueError, match='sampling'):
            fn((1.0, 2.0))
        with pytest.raises(ValueError, match='sampling'):
            fn((1.0, 0.0, 2.0))
    with pytest.raises(ValueError, match='radius must be'):
        P.skeleton_graph(mask, mask)
    with pytest.raises(ValueError, match='radius has shape'):
        P.skeleton_graph(mask, torch.zeros(4, 5, 7))
    for bad in ('abc', None, True, float('nan'), (1,)):
        with pytest.raises(ValueError, match='min_length'):
            P.prune_spurs(mask, bad)
        with pytest.raises(ValueError, match='min_spur'):
            P.vessel_graph(mask, None, True, bad)
    for bad in (0, -1, 1.5, 'abc', True):
        with pytest.raises(ValueError, match='rounds'):
            P.prune_spurs(mask, 3.0, None, bad)
    with pytest.raises(ValueError, match='SkeletonGraph'):
        P.network_summary(dict())
    for name in ('SkeletonGraph', 'skeleton_graph', 'prune_spurs', 'network_summary', 'vessel_graph'):
        assert getattr(van_gan_amd, name) is getattr(P, name)
    assert callable(van_gan_amd.VanGan.segment_graph)
    assert (P.NODE_ISOLATED, P.NODE_END, P.NODE_OTHER) == (G.ISOLATED, G.END, G.OTHER)


def test_the_entries_refuse_on_the_host():
    from van_gan_amd import _lib, build
    from van_gan_amd._lib import lib, lib_fp16
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vangan_hip.h')).read()
    for name, nargs in (('vg_skelgraph_classify', 8), ('vg_skelgraph_scratch_bytes', 2), ('vg_skelgraph_tables', 27), ('vg_skelgraph_prune', 18)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(lib, name) and hasattr(lib_fp16(), name)
        proto = header[header.index('\nint%s %s(' % ('64_t' if nargs == 2 else '', name)):]
        assert proto[:proto.index(';')].count(',') == nargs - 1
    assert 'vg_skelgraph.hip' in build.SOURCES

    def al16(b):
        return (b + 15) // 16 * 16
    for E, V in ((0, 0), (1, 0), (0, 1), (193, 330), (2 ** 20, 3), (2 ** 30, 2 ** 30)):
        assert lib.vg_skelgraph_scratch_bytes(E, V) == al16(80 * (E + 1) + 36 * (V + 1) + 16) + al16(12 * (E + 1)) == lib_fp16().vg_skelgraph_scratch_bytes(E, V)
    assert lib.vg_skelgraph_scratch_bytes(-1, 0) < 0 and lib.vg_skelgraph_scratch_bytes(0, -1) < 0 and lib.vg_skelgraph_scratch_bytes(2 ** 30 + 1, 0) < 0
    f, big = 1 << 20, 1 << 40                                      # non-NULL, aligned, never dereferenced: every call below is refused on the host
    assert lib.vg_skelgraph_classify(None, 4, 4, 4, f, f, f, None) == -1 and lib.vg_skelgraph_classify(f, 4, 4, 4, f, None, f, None) == -1
    assert lib.vg_skelgraph_classify(f, 4, 0, 4, f, f, f, None) == -1 and lib.vg_skelgraph_classify(f, 2048, 1024, 1024, f, f, f, None) == -1

    def tables(**kw):
        a = dict(skel=f, degree=f, seg=f, node=f, radius=None, X=4, Y=4, Z=4, E=3, V=2, sampling=None, half=f, vox=f, ends=f, nodes=f, length=f, chord=f,
                 rmean=None, rminmax=None, nvox=f, ndeg=f, kind=f, centroid=f, bad=f, scratch=f, nbytes=big)
        a.update(kw)
        return lib.vg_skelgraph_tables(*a.values(), None)
    three = lambda *v: (_lib.C.c_double * 3)(*v)  # noqa: E731
    for kw in (dict(skel=None), dict(node=None), dict(half=None), dict(kind=None), dict(bad=None), dict(scratch=None), dict(X=0), dict(Z=-4), dict(X=2048, Y=1024, Z=1024),
               dict(E=-1), dict(V=-1), dict(E=34), dict(V=34), dict(radius=f), dict(rmean=f), dict(radius=f, rmean=f), dict(half=f + 4), dict(centroid=f + 4),
               dict(seg=f + 2), dict(nvox=f + 1), dict(scratch=f + 8), dict(nbytes=lib.vg_skelgraph_scratch_bytes(3, 2) - 1),
               dict(sampling=three(1.0, 0.0, 1.0)), dict(sampling=three(1.0, float('inf'), 1.0)), dict(sampling=three(float('nan'), 1.0, 1.0))):
        assert tables(**kw) == -1, kw

    def prune(**kw):
        a = dict(skel=f, degree=f, seg=f, node=f, X=4, Y=4, Z=4, E=3, V=2, half=f, nodes=f, kind=f, min_length=2.5, sampling=None, flags=f, out=f, counts=f)
        a.update(kw)
        return lib.vg_skelgraph_prune(*a.values(), None)
    for kw in (dict(skel=None), dict(degree=None), dict(half=None), dict(flags=None), dict(out=None), dict(counts=None), dict(Y=0), dict(E=34), dict(V=-1),
               dict(min_length=float('nan')), dict(half=f + 4), dict(counts=f + 2), dict(sampling=three(-1.0, 1.0, 1.0))):
        assert prune(**kw) == -1, kw
