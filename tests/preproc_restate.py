"""float64 numpy restatement of the raw-volume preprocessing (van_gan_amd/preprocess.py), written from the behaviour it has to have:

    for each z:  s = std(x[..., z]) (ddof 0);  m = mean(x[..., z]);  zs[..., z] = (x - m) / s  if s > 0  else  x - m
    lp, up = percentile(zs, lower), percentile(zs, upper)        # scipy.stats.scoreatpercentile, 'fraction' interpolation
    c = clip(zs, lp, up);  out = ((c - min c) / (max c - min c) - 0.5) / 0.5

The reference computes its slice moments in float32; float64 is the truth both it and the device approximate (the convention of
tests/golden/*_np.npz).  device_order() is the bitwise oracle of the last stage: it takes the device's own fp32 z-scores and applies the
limits as the device does -- formed in float64, rounded once to fp32, used in fp32."""
import math

import numpy as np


def slice_moments(x):
    """[Z, 2] float64: (mean, population standard deviation) of every z-slice."""
    x = np.asarray(x)[..., 0] if np.ndim(x) == 4 else np.asarray(x)
    x64 = x.astype(np.float64)
    return np.stack([x64.mean(axis=(0, 1)), x64.std(axis=(0, 1))], axis=1)


def zscore_slices(x):
    x = np.asarray(x)[..., 0] if np.ndim(x) == 4 else np.asarray(x)
    x64 = x.astype(np.float64)
    out = np.empty_like(x64)
    for z in range(x64.shape[2]):
        sl = x64[..., z]
        s, m = sl.std(), sl.mean()
        out[..., z] = (sl - m) / s if s > 0 else sl - m
    return out


def rank_fraction(n, per):
    """index = per / 100 * (n - 1); (floor, min(floor + 1, n - 1), index - floor)."""
    idx = per / 100.0 * (n - 1)
    lo = int(math.floor(idx))
    return lo, min(lo + 1, n - 1), idx - lo


def percentile(a, per):
    """The score at percentile `per` of all values of a, linear between the two neighbouring order statistics; float64."""
    srt = np.sort(np.asarray(a).ravel())
    lo, hi, f = rank_fraction(srt.size, per)
    if f == 0.0:
        return np.float64(srt[lo])
    idx = per / 100.0 * (srt.size - 1)
    w_lo, w_hi = (lo + 1) - idx, idx - lo                  # both exact; their sum is 1
    return (np.float64(srt[lo]) * w_lo + np.float64(srt[hi]) * w_hi) / (w_lo + w_hi)


def prepare(x, lower=0.05, upper=99.95):
    zs = zscore_slices(x)
    lp, up = percentile(zs, lower), percentile(zs, upper)
    c = np.clip(zs, lp, up)
    out = ((c - c.min()) / (c.max() - c.min()) - 0.5) / 0.5
    return dict(z=zs, lp=lp, up=up, clipped=c, out=out)


def device_order(z32, lower=0.05, upper=99.95):
    """z32: the device's fp32 z-scores on the host.  Returns (lp, up, out) as fp32, bit for bit what the device must produce."""
    z32 = np.asarray(z32)
    assert z32.dtype == np.float32
    srt = np.sort(z32.ravel())
    lims = []
    for per in (lower, upper):
        lo, hi, f = rank_fraction(srt.size, per)
        lims.append(np.float32(np.float64(srt[lo]) * (1.0 - f) + np.float64(srt[hi]) * f))
    lp, up = lims
    c = np.where(z32 < lp, lp, np.where(z32 > up, up, z32)).astype(np.float32)
    out = ((c - lp) / (up - lp) - np.float32(0.5)) / np.float32(0.5)
    assert out.dtype == np.float32
    return lp, up, out


def zscore_bound(x):
    """Per-voxel bound of |z_device - z_float64|: 2^-22 * (|m| + |x - m|) / s with s := 1 on a constant slice -- the four fp32 roundings
    of (x - fl(m)) / fl(s): the mean (2^-24 |m|), the standard deviation (2^-24 |z| relative), the subtraction and the division."""
    x = np.asarray(x)[..., 0] if np.ndim(x) == 4 else np.asarray(x)
    x64 = x.astype(np.float64)
    ms = slice_moments(x)
    m, s = ms[:, 0], np.where(ms[:, 1] > 0, ms[:, 1], 1.0)
    return 2.0 ** -22 * (np.abs(m) + np.abs(x64 - m)) / s
