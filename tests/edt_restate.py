"""numpy restatement of the mask measurements (van_gan_amd/postprocess.py, csrc/vg_edt.hip): what the GPU suite (tests/test_gpu_edt.py)
compares with, pinned to scipy on the CPU by tests/test_edt_host.py.  Not a test module.

edt_sq: the separable squared Euclidean distance transform as three brute-force min-plus passes in int64 -- along Z, then Y, then X,
g(p) = min over p' of (f(p') + (p - p')^2), starting from 0 on the background and INF = 2^31 - 1 elsewhere; an INF source stays INF
(INF plus anything is clipped back to INF), so a volume without background is INF everywhere.  edt_weighted: its fp64 twin with
w_a = sampling_a^2, the cost f + w_a * (p - p')^2 rounded as a product and then a sum, sentinel +inf; the square root at the end.
fill_holes: label the background at connectivity 1, keep the components that miss all six faces."""
import numpy as np
import scipy.ndimage as ndi

INF = 2 ** 31 - 1


def _min_plus(f, axis, w, inf):
    """min over p' of (f(p') + w * (p - p')^2) along axis, one source position at a time"""
    f = np.moveaxis(f, axis, -1)
    L = f.shape[-1]
    p = np.arange(L, dtype=np.int64)
    g = np.full(f.shape, inf, f.dtype)
    for q in range(L):
        step = (p - q) ** 2
        g = np.minimum(g, f[..., q:q + 1] + (step if w is None else w * step.astype(np.float64)))
    return np.moveaxis(np.minimum(g, inf), -1, axis)


def edt_sq(mask):
    """int64 [X,Y,Z]: the squared distance to the nearest background voxel, INF where there is none"""
    f = np.where(np.asarray(mask) != 0, np.int64(INF), np.int64(0))
    for axis in (2, 1, 0):
        f = _min_plus(f, axis, None, np.int64(INF))
    return f


def edt(mask):
    """float32: np.sqrt of the squared distances in float64, rounded once; +inf for INF"""
    sq = edt_sq(mask)
    return np.where(sq == INF, np.inf, np.sqrt(sq.astype(np.float64))).astype(np.float32)


def edt_weighted(mask, sampling):
    """float64 [X,Y,Z]: the distance with voxel spacing sampling = (sx, sy, sz), +inf where there is no background"""
    f = np.where(np.asarray(mask) != 0, np.inf, 0.0)
    for axis in (2, 1, 0):
        s = float(sampling[axis])
        f = _min_plus(f, axis, s * s, np.inf)
    return np.sqrt(f)


def fill_holes(mask):
    """uint8 0 / 1: the mask and the background components (6 neighbours) that touch none of the six faces"""
    m = np.asarray(mask) != 0
    lab, K = ndi.label(~m, structure=ndi.generate_binary_structure(3, 1))
    faces = np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(), lab[:, :, 0].ravel(), lab[:, :, -1].ravel()])
    open_ = np.zeros(K + 1, bool)
    open_[faces] = True
    open_[0] = True                                                  # label 0 is the mask itself, kept by the first term
    return (m | ~open_[lab]).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ masks that break the method
def bernoulli(shape, p, seed=0):
    return (np.random.default_rng(seed + sum((i + 2) * s for i, s in enumerate(shape))).random(shape) < p).astype(np.uint8)


def one_background_corner(shape):
    """One background voxel, at (0, 0, 0): no scan ends early and the largest distances of the shape are reached."""
    m = np.ones(shape, np.uint8)
    m[0, 0, 0] = 0
    return m


def background_plane(shape):
    """Background confined to the plane x = c, and thinned out there: whole rows and columns hold the sentinel until the last pass."""
    m = np.ones(shape, np.uint8)
    c = shape[0] // 2
    m[c] = bernoulli(shape[1:], 0.9, seed=3)
    m[c, shape[1] // 2, shape[2] // 2] = 0
    return m


def tubes(shape, seed=0):
    """The vessel-like label volume of van_gan_amd.synth (tubular blobs), cut to shape."""
    from van_gan_amd.synth import synth_volumes
    X, Y, Z = shape
    _, S = synth_volumes(1, max(X, 8), max(Y, 8), max(Z, 8), seed=1234 + seed)
    return np.ascontiguousarray((S[0, :X, :Y, :Z, 0] > 0).numpy().astype(np.uint8))


def box(shape, lo, hi):
    """A solid box [lo, hi) inside a volume of zeros."""
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def hole_cases():
    """name -> mask: what hole filling has to tell apart."""
    out = {}
    m = box((7, 8, 9), (1, 1, 1), (6, 7, 8))
    m[3, 3, 3] = 0
    out['a closed box with a one-voxel cavity'] = m
    m = box((7, 8, 9), (1, 1, 1), (6, 7, 8))
    m[2, 2, 2] = 0                                                   # the cavity
    m[1, 1, 2] = 0                                                   # reaches it through an edge only
    out['a cavity joined to the outside through an edge'] = m
    m = box((7, 8, 9), (1, 1, 1), (6, 7, 8))
    m[2, 2, 2] = 0
    m[1, 1, 1] = 0                                                   # through a corner only
    out['a cavity joined to the outside through a corner'] = m
    m = box((7, 8, 9), (0, 1, 1), (6, 7, 8))
    m[0:3, 3, 3] = 0                                                 # a pit that opens on the face x = 0
    out['a cavity that touches a face'] = m
    m = box((11, 11, 70), (1, 1, 1), (10, 10, 69))
    m[2:9, 2:9, 2:68] = 0
    m[3:8, 3:8, 3:67] = 1
    m[4:7, 4:7, 4:66] = 0
    m[5, 5, 5:65] = 1
    out['nested shells'] = m
    m = np.zeros((9, 9, 66), np.uint8)
    m[2:7, 2:7, :] = 1
    m[3:6, 3:6, :] = 0                                               # the lumen runs from face to face
    out['a tube open at both ends'] = m
    m = np.zeros((9, 9, 66), np.uint8)
    m[2:7, 2:7, :] = 1
    m[3:6, 3:6, 1:65] = 0                                            # the same tube, capped: the lumen is a hole
    out['a tube closed at both ends'] = m
    return out
