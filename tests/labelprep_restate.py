"""float32 numpy restatement of the label-volume preprocessing (van_gan_amd.preprocess.value_mode / prepare_segmentation), written from the
behaviour it has to have:

    s: the label stack as float32 [X,Y,Z]; a non-finite value anywhere refuses the stack ('NaN detected')
    only after a resize:  s[s < 0] = 0;  s[s > 255] = 255
    y = (s - min s) / (max s - min s)                 # float32, each operation rounded; min == max is min_max_norm's ValueError
    m = the most frequent value of y, the smallest among equally frequent ones
    if m == 1:  y = |y - 1|
    z = (y - 0.5) / 0.5;  out = -1 where z < 0, else +1

Everything stays in float32, so the device has to reproduce it bit for bit."""
import numpy as np

F32 = np.float32
MINMAX_ERROR = 'Cannot perform min-max normalization when max and min are equal.'


def mode(a):
    """(value, count) of the most frequent finite value of a: np.unique sorts the distinct values, argmax takes the first maximum, so
    among equally frequent values the smallest wins.  -0.0 and +0.0 compare equal and are one value, reported as +0.0."""
    flat = np.asarray(a).ravel()
    flat = flat[np.isfinite(flat)]
    values, counts = np.unique(flat, return_counts=True)
    i = int(np.argmax(counts))
    return values[i] + values.dtype.type(0), int(counts[i])


def clamp(s):
    s = np.array(s, F32)
    s[s < 0] = 0
    s[s > 255] = 255
    return s


def normalise(s):
    s = np.asarray(s)
    assert s.dtype == F32
    mn, mx = s.min(), s.max()
    if mn == mx:
        raise ValueError(MINMAX_ERROR)
    y = (s - mn) / (mx - mn)
    assert y.dtype == F32
    return y, mn, mx


def label(raw, resized=False):
    """dict(out float32 in {-1, +1}, inverted, mode, count, min, max) of a raw stack [X,Y,Z] or [X,Y,Z,1] (uint8, uint16 or float32);
    resized: the stack is the output of a resize, so it is clamped to [0, 255] first."""
    s = np.asarray(raw)
    s = (s[..., 0] if s.ndim == 4 else s).astype(F32)
    if not np.isfinite(s).all():
        raise ValueError('NaN detected')
    if resized:
        s = clamp(s)
    y, mn, mx = normalise(s)
    m, count = mode(y)
    inverted = bool(m == 1)
    if inverted:
        y = np.abs(y - F32(1))
    z = (y - F32(0.5)) / F32(0.5)
    out = np.where(z < 0, F32(-1), F32(1)).astype(F32)
    assert y.dtype == F32 and z.dtype == F32
    return dict(out=out, inverted=inverted, mode=float(m), count=count, min=float(mn), max=float(mx))


def collision_example():
    """Twelve-plus values whose raw mode is 7 (five times) while three neighbours of the maximum merge with it under the float32
    normalisation: six values become exactly 1.0 and the mode of the normalised array is 1."""
    top = F32(200)
    below = np.nextafter(top, F32(0))
    below2 = np.nextafter(below, F32(0))
    return np.array([-100] * 2 + [top] * 3 + [below] * 3 + [7] * 5 + [below2], F32)
