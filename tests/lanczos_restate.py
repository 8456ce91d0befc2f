"""float64 numpy restatement of the Lanczos-4 volume resize (van_gan_amd/preprocess.py resize_volume), written from the filter's
definition, not from the library's code:

    one axis, L -> T samples, for dx = 0 .. T-1:
        fx = float32((dx + 0.5) * (1 / (T / L)) - 0.5);  sx = floor(fx);  t = fx - sx  (float32)
        taps k = 0 .. 7 read the source at clip(sx - 3 + k, 0, L - 1)
        t < 2^-23:  w = unit tap at k = 3
        else:       c_k = float32((-1)^k sin(y_k) / y_k^2),  y_k = -(t + 3 - k) pi / 4  (float64);  S = c_0 + ... + c_7 in float32;
                    w_k = c_k * float32(1 / S)
    a volume: the axes Y, X, Z in that order, an axis whose length does not change skipped

The coefficients are the float32 ones the device uses (they ARE the filter); the accumulation and the intermediates are float64, the truth
that float32 dot products and float32 intermediates approximate.  abs_resize() runs the same passes with |w| on |x|: the factor of the
rounding-error bound."""
import math

import numpy as np

EPS = 2.0 ** -23


def weights(t):
    """The 8 float32 coefficients of the float32 phase t."""
    t = float(np.float32(t))
    w = np.zeros(8, np.float32)
    if t < EPS:
        w[3] = 1
        return w
    s = np.float32(0)
    for k in range(8):
        y = -(t + 3 - k) * math.pi / 4
        w[k] = np.float32((-1) ** k * math.sin(y) / (y * y))
        s = np.float32(s + w[k])
    inv = np.float32(np.float32(1) / s)
    return (w * inv).astype(np.float32)


def phases(L, T):
    """(sx int64 [T], t float32 [T])."""
    scale = 1.0 / (T / L)
    fx = np.array([np.float32((dx + 0.5) * scale - 0.5) for dx in range(T)], np.float32)
    sx = np.floor(fx)
    return sx.astype(np.int64), (fx - sx).astype(np.float32)


def table(L, T):
    """(first int32 [T] = sx - 3, unclamped; w8 float32 [T, 8])."""
    sx, t = phases(L, T)
    return (sx - 3).astype(np.int32), np.stack([weights(v) for v in t])


def _apply(x, axis, T, mag):
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
    L = x.shape[0]
    first, w8 = table(L, T)
    w = np.abs(w8.astype(np.float64)) if mag else w8.astype(np.float64)
    out = np.zeros((T,) + x.shape[1:], np.float64)
    for k in range(8):
        idx = np.clip(first.astype(np.int64) + k, 0, L - 1)
        out += w[:, k].reshape((T,) + (1,) * (x.ndim - 1)) * x[idx]
    return np.moveaxis(out, 0, axis)


def apply_axis(x, axis, T):
    """One pass along `axis`: the float32 table, float64 accumulation; float64."""
    return _apply(x, axis, T, False)


def _passes(x, target, mag):
    x = np.abs(np.asarray(x, np.float64)) if mag else np.asarray(x, np.float64)
    assert x.ndim == 3 and len(target) == 3
    n = 0
    for axis in (1, 0, 2):
        if x.shape[axis] != target[axis]:
            x = _apply(x, axis, target[axis], mag)                      # float64 throughout: the device's float32 intermediate is an error term
            n += 1
    return x, n


def resize(x, target):
    """[X,Y,Z] -> target: (float64 result, number of passes executed)."""
    return _passes(x, target, False)


def abs_resize(x, target):
    """The same passes with |w| applied to |x| (no rounding between them): A of the bound p * 9 * 2^-24 * A."""
    return _passes(x, target, True)[0]
