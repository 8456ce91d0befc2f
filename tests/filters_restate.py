"""numpy restatement of the imaging filters (include/vangan_hip.h "Imaging filters"): what the GPU tests compare against, and what
tests/test_filters_host.py pins to scipy.ndimage.median_filter and to the literal numpy recipe of threshold_outliers."""
import itertools

import numpy as np

F32 = np.float32


def _size3(size):
    return (int(size),) * 3 if np.isscalar(size) else tuple(int(s) for s in size)


def median(x, size=3):
    """The element of rank m // 2 among the m = sx * sy * sz values of the window centred on each voxel; the volume is continued by
    np.pad(mode='symmetric') (-1 reads 0, n reads n - 1: scipy's mode='reflect')."""
    x = np.asarray(x)
    s3 = _size3(size)
    assert x.ndim == 3 and all(s % 2 == 1 for s in s3)
    h = [s // 2 for s in s3]
    p = np.pad(x, [(k, k) for k in h], mode='symmetric')
    views = [p[i:i + x.shape[0], j:j + x.shape[1], k:k + x.shape[2]]
             for i, j, k in itertools.product(range(s3[0]), range(s3[1]), range(s3[2]))]
    return np.sort(np.stack(views, axis=0), axis=0)[len(views) // 2]


def moments64(x):
    """(mean, population standard deviation) in float64, and their float32 roundings."""
    x64 = np.asarray(x, dtype=np.float64)
    m, s = x64.mean(), x64.std()
    return m, s, F32(m), F32(s)


def outlier_limits(x32, m32, s32, thr):
    """(lower, upper, kept): the smallest and the largest value with |(x - m) / s| <= thr, each of the three operations in float32, and how
    many values satisfy it.  Nothing kept: (+inf, -inf, 0)."""
    x32 = np.asarray(x32)
    assert x32.dtype == F32
    with np.errstate(all='ignore'):
        z = np.abs((x32 - F32(m32)) / F32(s32))
        assert z.dtype == F32
        keep = z <= F32(thr)
    kept = int(keep.sum())
    if kept == 0:
        return F32(np.inf), F32(-np.inf), 0
    sel = x32[keep]
    return sel.min(), sel.max(), kept


def threshold_outliers(x32, thr=6):
    """x32 clipped to the limits taken at the float32-rounded float64 moments."""
    x32 = np.asarray(x32)
    _, _, m32, s32 = moments64(x32)
    lo, hi, _ = outlier_limits(x32, m32, s32, thr)
    return np.clip(x32, lo, hi)


def limit_volumes(seed=7, shape=(24, 20, 36)):
    """The three raw volumes of the limits tests: a bulk with a few far outliers, so that the limits are data values well inside the
    threshold and the kept set does not change when a moment moves by an ulp (the tests assert that)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    u16 = np.clip(rng.normal(3000, 200, shape), 0, 65535).astype(np.uint16)
    u16.reshape(-1)[rng.choice(n, 40, replace=False)] = rng.integers(20000, 65535, 40).astype(np.uint16)
    u16.reshape(-1)[rng.choice(n, 5, replace=False)] = 0
    u8 = np.clip(rng.normal(60, 6, shape), 0, 255).astype(np.uint8)
    u8.reshape(-1)[rng.choice(n, 30, replace=False)] = 255
    f32 = rng.standard_normal(shape).astype(F32)
    f32.reshape(-1)[rng.choice(n, 30, replace=False)] *= F32(50)
    out = {'uint16': u16, 'uint8': u8, 'float32': f32}
    for a in out.values():
        a.setflags(write=False)
    return out


def limits_at_neighbours(x32, thr):
    """The limits at the float32-rounded float64 moments and at their eight neighbours (m +- 1 ulp, s +- 1 ulp): nine (lower, upper, kept)."""
    _, _, m32, s32 = moments64(x32)
    ms = (np.nextafter(m32, F32(-np.inf)), m32, np.nextafter(m32, F32(np.inf)))
    ss = (np.nextafter(s32, F32(-np.inf)), s32, np.nextafter(s32, F32(np.inf)))
    return [outlier_limits(x32, m, s, thr) for m in ms for s in ss]


def rescale(c, lo, hi):
    """((c - lo) / (hi - lo) - 0.5) / 0.5 in float32, each operation rounded: vg_clip_rescale's arithmetic after the clip."""
    c, lo, hi = np.asarray(c, F32), F32(lo), F32(hi)
    u = (c - lo) / F32(hi - lo)
    return (u - F32(0.5)) / F32(0.5)
