"""numpy restatement of the vessel graph (van_gan_amd/postprocess.py skeleton_graph, prune_spurs, network_summary;
csrc/vg_skelgraph.hip; the definitions are in include/vangan_hip.h "The vessel graph" and DESIGN.md 3.19): what the GPU suite
(tests/test_gpu_vesselgraph.py) compares with by equality, pinned on the CPU by tests/test_vesselgraph_host.py to a sequential tracer
and to invariants that share no code with it.  numpy and scipy.ndimage.label alone; imports nothing from the package.  Not a test module.

S = {skel != 0}; deg = 26-neighbour count; B = {deg = 2} are the segment voxels, N = S \\ B the node voxels; segments and nodes are the
26-components of B and of N as scipy.ndimage.label numbers them.  Every table has one row per label and a row 0 of zeros."""
import math

import numpy as np
import scipy.ndimage as ndi

FULL = np.ones((3, 3, 3), bool)
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
ISOLATED, END, OTHER = 0, 1, 2


def step_class(dx, dy, dz):
    return 4 * abs(dx) + 2 * abs(dy) + abs(dz) - 1


def degree(m):
    m = np.asarray(m) != 0
    pad = np.pad(m, 1).astype(np.int64)
    X, Y, Z = m.shape
    s = sum(pad[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z] for dx, dy, dz in OFFSETS)
    return np.where(m, s, 0).astype(np.uint8)


def _spacing(sampling):
    if sampling is None:
        return np.ones(3, np.float64)
    return np.asarray((sampling,) * 3 if np.isscalar(sampling) else sampling, np.float64)


def step_lengths(sampling=None):
    """fp64 [7]: l[c] = sqrt((|dx| sx)^2 + (|dy| sy)^2 + (|dz| sz)^2) of class c = 4 |dx| + 2 |dy| + |dz| - 1"""
    s = _spacing(sampling)
    out = np.zeros(7, np.float64)
    for c in range(7):
        a = np.array([(c + 1) >> 2 & 1, (c + 1) >> 1 & 1, (c + 1) & 1], np.float64) * s
        out[c] = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return out


def radius_scale(shape, sampling=None):
    """(k, D): the fixed point of the radius sums is 2^-k; D is the diagonal of the volume, above which no radius is taken"""
    e = np.asarray(shape, np.float64) * _spacing(sampling)
    D = float(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))
    n = int(np.prod([int(v) for v in shape]))
    b = 62 - (n - 1).bit_length()                                    # 62 - ceil(log2 n)
    mant, ex = math.frexp(D)                                         # D = mant 2^ex, 0.5 <= mant < 1
    return b - (ex if mant > 0.5 else ex - 1), D


def length_of(half, sampling=None):
    """(sum over c of half[:, c] l[c]) / 2, left to right"""
    l = step_lengths(sampling)
    half = np.asarray(half)
    acc = half[:, 0].astype(np.float64) * l[0]
    for c in range(1, 7):
        acc = acc + half[:, c].astype(np.float64) * l[c]
    return acc / 2.0


def graph(skel, radius=None, sampling=None):
    """dict of numpy arrays with the fields of van_gan_amd.postprocess.SkeletonGraph, and: attachments [E + 1] (the (B voxel, N
    neighbour) pairs of every segment), bad (the segment voxels whose radius was skipped)"""
    m = np.asarray(skel) != 0
    X, Y, Z = m.shape
    s = _spacing(sampling)
    deg = degree(m)
    B = m & (deg == 2)
    N = m & ~B
    seg, E = ndi.label(B, structure=FULL)
    node, V = ndi.label(N, structure=FULL)
    seg, node = seg.astype(np.int32), node.astype(np.int32)
    segp, nodep = np.pad(seg, 1), np.pad(node, 1)
    bx, by, bz = np.nonzero(B)
    e_of = seg[bx, by, bz].astype(np.int64)
    p_lin = (bx * Y + by) * Z + bz
    half = np.zeros((E + 1, 7), np.int64)
    pe, pp, pq, pn = [], [], [], []
    for dx, dy, dz in OFFSETS:
        c = step_class(dx, dy, dz)
        sq = segp[bx + 1 + dx, by + 1 + dy, bz + 1 + dz]
        nq = nodep[bx + 1 + dx, by + 1 + dy, bz + 1 + dz]
        np.add.at(half[:, c], e_of[sq > 0], 1)
        np.add.at(half[:, c], e_of[nq > 0], 2)
        sel = nq > 0
        pe.append(e_of[sel])
        pp.append(p_lin[sel])
        pq.append((((bx + dx) * Y + (by + dy)) * Z + (bz + dz))[sel])
        pn.append(nq[sel].astype(np.int64))
    pe, pp, pq, pn = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (pe, pp, pq, pn))
    attachments = np.bincount(pe, minlength=E + 1)
    ends = np.zeros((E + 1, 2), np.int64)
    ends[1:] = -1
    nodes = np.zeros((E + 1, 2), np.int32)
    order = np.lexsort((pq, pp, pe))                                 # the pairs by (segment, p, q): the first and the last of every
    pe, pp, pq, pn = pe[order], pp[order], pq[order], pn[order]      # segment are its smallest and its largest pair (p, q)
    has = np.nonzero(attachments)[0]
    lo, hi = np.searchsorted(pe, has, 'left'), np.searchsorted(pe, has, 'right') - 1
    ends[has, 0], ends[has, 1] = pq[lo], pq[hi]
    nodes[has, 0], nodes[has, 1] = pn[lo], pn[hi]
    seg_voxels = np.bincount(seg.ravel(), minlength=E + 1).astype(np.int32)
    seg_voxels[0] = 0
    path = ends[:, 0] >= 0
    path[0] = False
    c0 = np.stack(np.unravel_index(np.where(path, ends[:, 0], 0), m.shape), 1)
    c1 = np.stack(np.unravel_index(np.where(path, ends[:, 1], 0), m.shape), 1)
    d = (c0 - c1).astype(np.float64) * s
    chord = np.where(path, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), 0.0)
    out = dict(segment_labels=seg, node_labels=node, degree=deg, E=E, V=V, seg_voxels=seg_voxels, seg_nodes=nodes, seg_ends=ends, seg_half_steps=half,
               seg_length=length_of(half, sampling), seg_chord=chord, attachments=attachments, shape=m.shape, sampling=tuple(float(v) for v in s),
               seg_radius_mean=None, seg_radius_min=None, seg_radius_max=None, bad=0)
    if radius is not None:
        k, D = radius_scale(m.shape, sampling)
        r = np.asarray(radius, np.float32)[bx, by, bz]
        with np.errstate(invalid='ignore'):
            ok = (r >= 0) & (r.astype(np.float64) <= D)
        out['bad'] = int((~ok).sum())
        r, eo = r[ok], e_of[ok]
        rsum = np.zeros(E + 1, np.int64)
        np.add.at(rsum, eo, np.rint(r.astype(np.float64) * 2.0 ** k).astype(np.int64))
        rmin, rmax = np.full(E + 1, np.inf, np.float32), np.full(E + 1, -np.inf, np.float32)
        np.minimum.at(rmin, eo, r)
        np.maximum.at(rmax, eo, r)
        some = np.isfinite(rmin)
        with np.errstate(invalid='ignore', divide='ignore'):
            out['seg_radius_mean'] = np.where(some, rsum.astype(np.float64) / 2.0 ** k / seg_voxels, 0.0)
        out['seg_radius_min'] = np.where(some, np.abs(rmin), np.float32(0)).astype(np.float32)      # abs: -0 counts as 0
        out['seg_radius_max'] = np.where(some, np.abs(rmax), np.float32(0)).astype(np.float32)
    node_voxels = np.bincount(node.ravel(), minlength=V + 1).astype(np.int32)
    node_voxels[0] = 0
    nx, ny, nz = np.nonzero(N)
    n_of = node[nx, ny, nz]
    top = np.zeros(V + 1, np.int64)
    np.maximum.at(top, n_of, deg[nx, ny, nz].astype(np.int64))      # of a node of one voxel: that voxel's degree
    kind = np.where(node_voxels == 1, np.minimum(top, 2), OTHER).astype(np.uint8)
    kind[0] = 0
    sums = np.zeros((V + 1, 3), np.uint64)
    for a, coord in enumerate((nx, ny, nz)):
        np.add.at(sums[:, a], n_of, coord.astype(np.uint64))
    with np.errstate(invalid='ignore', divide='ignore'):
        centroid = np.where(node_voxels[:, None] > 0, sums.astype(np.float64) / node_voxels[:, None].astype(np.float64), 0.0)
    out.update(node_voxels=node_voxels, node_degree=np.bincount(pn, minlength=V + 1).astype(np.int32), node_kind=kind, node_centroid=centroid)
    return out


def prune_round(skel, min_length, sampling=None):
    """(mask, spurs, voxels deleted) of one pruning round"""
    m = np.asarray(skel) != 0
    g = graph(m, None, sampling)
    n0, n1 = g['seg_nodes'][:, 0], g['seg_nodes'][:, 1]
    kind = g['node_kind']
    flag = (n0 > 0) & ((kind[n0] == END) != (kind[n1] == END)) & (g['seg_length'] < min_length)
    flag[0] = False
    seg = g['segment_labels']
    gone = flag[seg]
    segp = np.pad(seg, 1)
    tx, ty, tz = np.nonzero(m & (seg == 0) & (g['degree'] == 1))
    hit = np.zeros(len(tx), bool)
    for dx, dy, dz in OFFSETS:
        hit |= flag[segp[tx + 1 + dx, ty + 1 + dy, tz + 1 + dz]]
    gone[tx[hit], ty[hit], tz[hit]] = True
    return (m & ~gone).astype(np.uint8), int(flag.sum()), int(gone.sum())


def prune(skel, min_length, sampling=None, rounds=1):
    """(mask, dict(rounds, spurs, voxels)): rounds until one removes nothing, `rounds` at most; min_length <= 0: a copy, no round"""
    cur = (np.asarray(skel) != 0).astype(np.uint8)
    info = dict(rounds=0, spurs=[], voxels=[])
    if min_length <= 0:
        return cur, info
    for _ in range(rounds):
        cur, spurs, voxels = prune_round(cur, min_length, sampling)
        info['rounds'] += 1
        info['spurs'].append(spurs)
        info['voxels'].append(voxels)
        if voxels == 0:
            break
    return cur, info


def summary(g):
    """the dict of van_gan_amd.postprocess.network_summary from the tables of graph()"""
    E = g['E']
    length, chord, vox = g['seg_length'][1:], g['seg_chord'][1:], g['seg_voxels'][1:].astype(np.float64)
    n0, n1 = g['seg_nodes'][1:, 0], g['seg_nodes'][1:, 1]
    kind = g['node_kind'][1:]
    total = float(length.sum())
    volume = float(np.prod([float(v) for v in g['shape']]) * np.prod(g['sampling']))
    curved = chord > 0
    has_r = g['seg_radius_mean'] is not None
    return dict(segments=E, cycles=int((g['seg_ends'][1:, 0] < 0).sum()), loops=int(((n0 == n1) & (n0 > 0)).sum()), nodes=g['V'],
                end_points=int((kind == END).sum()), junctions=int((kind == OTHER).sum()), isolated=int((kind == ISOLATED).sum()),
                total_length=total, length_density=total / volume,
                mean_radius=float((g['seg_radius_mean'][1:] * vox).sum() / vox.sum()) if has_r and vox.sum() > 0 else None,
                mean_tortuosity=float((length[curved] / chord[curved]).mean()) if curved.any() else None)


# ------------------------------------------------------------------------------------------------ masks with known answers
def line(L, step, origin=(0, 0, 0), shape=None):
    """L voxels from origin in steps of `step` (a 26-neighbour offset)"""
    pts = np.asarray(origin)[None, :] + np.arange(L)[:, None] * np.asarray(step)[None, :]
    if shape is None:
        shape = tuple(int(v) + 1 for v in pts.max(0))
    m = np.zeros(shape, np.uint8)
    m[pts[:, 0], pts[:, 1], pts[:, 2]] = 1
    return m


def tee_bar(shape=(3, 13, 7), at=(1, 1, 1)):
    """the bar of tee() alone: five voxels along y, an apex one step up in z, five more voxels along y"""
    m = np.zeros(shape, np.uint8)
    x, y, z = at
    m[x, y:y + 5, z] = m[x, y + 6:y + 11, z] = 1
    m[x, y + 5, z + 1] = 1
    return m


def tee(shape=(3, 13, 7), at=(1, 1, 1)):
    """tee_bar() with a spur of three voxels along z from its apex: 4 nodes (three end points and the apex, a junction of one voxel),
    3 segments -- two arms of length 4 + sqrt(2) and the spur of length 3.  (A spur from a straight bar would leave its first voxel in
    the junction cluster, which pruning never touches.)"""
    m = tee_bar(shape, at)
    x, y, z = at
    m[x, y + 5, z + 2:z + 5] = 1
    return m


def ring_with_tail(shape=(3, 9, 12), at=(1, 1, 1)):
    """a diamond ring in the y-z plane with a straight tail along z from its corner: the ring is a loop, both ends at the junction"""
    m = np.zeros(shape, np.uint8)
    x, y, z = at
    for i in range(4):
        m[x, y + 3 - i, z + i] = m[x, y + 3 + i, z + i] = m[x, y + i, z + 3 + i] = m[x, y + 6 - i, z + 3 + i] = 1
    m[x, y + 3, z + 7:z + 10] = 1
    return m


def bridge(shape=(5, 5, 7), at=(2, 2, 2)):
    """two junctions, `at` and two voxels further along z, joined through the one voxel between them; each has two diagonal arms of two
    voxels that touch nothing else: a one-voxel segment between two nodes of kind 2, four one-voxel segments to four end points"""
    m = np.zeros(shape, np.uint8)
    x, y, z = at
    m[x, y, z:z + 3] = 1
    for k in (1, 2):
        m[x + k, y + k, z - k] = m[x - k, y - k, z - k] = m[x + k, y + k, z + 2 + k] = m[x - k, y - k, z + 2 + k] = 1
    return m
