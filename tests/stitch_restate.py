"""Float64 numpy restatement of the whole sliding-window stitch with the blending and flip-averaging modes -- TEST INFRASTRUCTURE ONLY.
Written from the description of the feature, not from the engine's code: symmetric pad, the window walk with
its clamped trailing origins, border crop, optional per-window min-max to [-1,1], flip -> gen -> un-flip, weighted overlap-add, division
by the summed weights, un-pad, 255 * min-max.  In 'count' mode without flips it is the reference's stitch (oracle/stitch_oracle.py, which
accumulates in fp32); tests/test_stitchblend_host.py pins the two together.

Shared helpers of the two stitchblend test files live here too: the probe generator and the small table every kernel test uses."""
import itertools
import math

import numpy as np

AXIS_BIT = {'x': 1, 'y': 2, 'z': 4}


def origins_1d(n, k, s):
    """floor((n-k)/s + 1) + 1 starts, stepping by s, each clamped to n-k (so trailing ones may coincide and then count twice)."""
    count = int(math.floor((n - k) / s + 1)) + 1
    return [min(t * s, n - k) for t in range(count)]


def flip_masks(tta):
    allowed = sum(AXIS_BIT[a] for a in tta)
    return [m for m in range(8) if not m & ~allowed]


def flip(a, mask):
    """Mirror the first three axes of `a` whose bit is set in mask (bit 0 = first axis)."""
    ax = [d for d in range(3) if mask >> d & 1]
    return np.flip(a, ax) if ax else a


def axis_weights(k, sigma_scale):
    i = np.arange(k, dtype=np.float64)
    return np.maximum(np.exp(-0.5 * ((i - (k - 1) / 2.0) / (sigma_scale * k)) ** 2), 1e-12).astype(np.float32).astype(np.float64)


def stitch(gen, img, k, stride=(25, 25, 128), complete=True, padFactor=0.25, border_removal=True, process_img=False, blend='count',
           sigma_scale=0.125, tta=''):
    """gen: callable on a float64 [1,kx,ky,kz,1] array, returning the same shape.  img [X,Y,Z,1].  Returns a dict:
    out (255 * min-max, [X,Y,Z,1] float64), raw (the un-normalised quotient), n_max (largest number of contributions to one voxel of the
    padded volume), gen_absmax (largest |generator output| seen), forwards (generator calls)."""
    v = np.asarray(img, dtype=np.float64)[..., 0]
    ox, oy, oz = v.shape
    sx = sy = sz = 0
    if complete:
        sx, sy = int(padFactor * ox), int(padFactor * oy)
        sz = 0 if stride[2] == 1 else int(padFactor * oz)
        v = np.pad(v, ((sx, sx), (sy, sy), (sz, sz)), 'symmetric')
    dims = v.shape
    p = [int(0.1 * n) for n in k] if (complete and border_removal) else [0, 0, 0]
    if k[2] == dims[2]:
        p[2] = 0
    if blend == 'gaussian':
        wx, wy, wz = (axis_weights(n, sigma_scale) for n in k)
    elif blend == 'count':
        wx, wy, wz = (np.ones(n) for n in k)
    else:
        raise ValueError(blend)
    w = (wx[:, None, None] * wy[None, :, None]) * wz[None, None, :]
    crop = tuple(slice(p[a], k[a] - p[a]) for a in range(3))
    num, den, hits = np.zeros(dims), np.zeros(dims), np.zeros(dims, dtype=np.int64)
    gmax, forwards = 0.0, 0
    for o in itertools.product(*(origins_1d(dims[a], k[a], stride[a]) for a in range(3))):
        box = tuple(slice(o[a] + p[a], o[a] + k[a] - p[a]) for a in range(3))
        arr = v[o[0]:o[0] + k[0], o[1]:o[1] + k[1], o[2]:o[2] + k[2]]
        if process_img:
            arr = 2.0 * (arr - arr.min()) / (arr.max() - arr.min()) - 1.0
        for m in flip_masks(tta):
            y = np.asarray(gen(np.ascontiguousarray(flip(arr, m))[None, ..., None]), dtype=np.float64)[0, ..., 0]
            forwards += 1
            gmax = max(gmax, float(np.abs(y).max()))
            y = flip(y, m)
            num[box] += (w * y)[crop]
            den[box] += w[crop]
            hits[box] += 1
    with np.errstate(invalid='ignore', divide='ignore'):
        raw = (num / den)[sx:sx + ox, sy:sy + oy, sz:sz + oz]
    out = 255.0 * (raw - raw.min()) / (raw.max() - raw.min())
    return dict(out=out[..., None], raw=raw, n_max=int(hits.max()), gen_absmax=gmax, forwards=forwards)


# ---- the probe generator: tanh(0.7 a) + ramp, the ramp asymmetric in every axis (a missing or doubled un-flip shows) ----
RAMP = (0.031, -0.017, 0.011)


def ramp(k):
    i, j, l = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in k), indexing='ij')
    return RAMP[0] * i + RAMP[1] * j + RAMP[2] * l


def probe_gen(a):
    return np.tanh(0.7 * a) + ramp(a.shape[1:4])[None, ..., None]


def equivariant_gen(a):
    return np.tanh(0.7 * a)


# ---- kernel-test fixtures: volume 29x23x17, 11 table rows per window size ----
VOL = (29, 23, 17)


def table(k):
    """11 rows (x0, y0, z0, flip): all 8 flip masks, unaligned origins, the clamped last origin of each axis, one duplicated row."""
    mx, my, mz = (VOL[a] - k[a] for a in range(3))
    rows = [(0, 0, 0, 0), (1, 3, 2, 1), (5, 1, 1, 2), (3, 2, 5, 3), (mx, 0, 1, 4), (2, my, 3, 5), (7, 5, mz, 6), (mx, my, mz, 7),
            (mx, my, mz, 7), (4, 4, 0, 0), (9, 7, 1, 5)]
    rows = [(min(x, mx), min(y, my), min(z, mz), f) for x, y, z, f in rows]          # (8,8,16) leaves z origins 0..1 only
    assert all(0 <= r[a] <= VOL[a] - k[a] for r in rows for a in range(3)) and {r[3] for r in rows} == set(range(8))
    return np.array(rows, dtype=np.int32)
