"""Raw-volume preprocessing on MI355X: the imaging-domain recipe the reference runs before run_mapping (main.py:255-270) --
preprocess_rsom_images (main.py:127-150: z-score every z-slice, clip to two percentiles of the whole volume with
scipy.stats.scoreatpercentile) followed by process_tiff's min_max_norm and (x - 0.5) / 0.5 and its NaN check (preprocessing.py:179-215)
-- and, on request, process_tiff's resize_volume between the two (utils.py:224-255: Lanczos-4) -- and process_tiff's label-domain branch
(preprocessing.py:173-189: prepare_segmentation), without the TIFF I/O -- and the two further preprocessors the
reference's driver brings in for imaging volumes, scipy.ndimage.median_filter and threshold_outliers (main.py:34-36, utils.py:108-133),
as functions of their own and as stages of prepare_imaging.  The arithmetic runs in csrc/vg_preproc.hip, csrc/vg_resample.hip,
csrc/vg_labelprep.hip and csrc/vg_filters.hip (include/vangan_hip.h "Raw-volume preprocessing", "Volume resize", "Label-volume
preprocessing" and "Imaging filters", DESIGN.md sections 3.12 to 3.15); this module owns buffers, ranks, filter tables and checks.

A volume is [X,Y,Z] (or [X,Y,Z,1]) with Z innermost -- process_tiff's layout after its transpose -- as uint8, uint16 or float32, a numpy
array or a torch tensor, on the host or on the device.  torch has no uint16 arithmetic, so a 16-bit stack travels as the int16 tensor of
the same bytes and the kernels read it as what it is."""
from __future__ import annotations

import ctypes as C
import functools
import math
import operator
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check as _check, lib
from .ops import _p, stream

PP_U8, PP_U16, PP_F32 = 0, 1, 2            # VG_PP_U8, VG_PP_U16, VG_PP_F32
MAX_RANKS = 4                              # VG_PP_MAX_RANKS
MODE_LDS_SLOTS = 1024                      # VG_MODE_LDS_SLOTS: the slots of value_mode's per-workgroup combiner
MINMAX_ERROR = 'Cannot perform min-max normalization when max and min are equal.'       # the message of min_max_norm (utils.py:23)
_T_UINT16 = getattr(torch, 'uint16', None)


class RawVolume:
    """A device-resident raw volume: the tensor that owns the bytes, the dtype code the kernels read them as, and (X, Y, Z)."""

    def __init__(self, buf: torch.Tensor, code: int, shape: Tuple[int, int, int]):
        self.buf, self.code, self.shape = buf, code, shape

    @property
    def nxy(self) -> int:
        return self.shape[0] * self.shape[1]

    @property
    def numel(self) -> int:
        return self.nxy * self.shape[2]


def _drop_channel(sizes: tuple) -> tuple:                      # [a, b, c, 1] -> [a, b, c]: the trailing 1 of a volume's shape is tolerated
    return sizes[:3] if len(sizes) == 4 and sizes[3] == 1 else sizes


def _shape3(shape) -> Tuple[int, int, int]:
    shape = _drop_channel(tuple(int(s) for s in shape))
    if len(shape) != 3:
        raise ValueError('a volume is [X,Y,Z] or [X,Y,Z,1], got shape %s' % (shape,))
    if min(shape) < 1:
        raise ValueError('empty volume %s' % (shape,))
    return shape


def _resolve_device(device, given: Optional[torch.device]) -> torch.device:
    if device is None:
        device = given if given is not None and given.type == 'cuda' else 'cuda'
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('the preprocessing runs on the GPU, got device %s' % (dev,))
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def as_raw_volume(raw, device=None) -> RawVolume:
    """Validates (shape and dtype first: a bad argument is rejected before the device is touched), then uploads if needed."""
    if isinstance(raw, RawVolume):
        return raw
    if isinstance(raw, np.ndarray):
        shape = _shape3(raw.shape)
        code = {np.dtype(np.uint8): PP_U8, np.dtype(np.uint16): PP_U16, np.dtype(np.float32): PP_F32}.get(raw.dtype)
        if code is None:
            raise ValueError('a raw volume is uint8, uint16 or float32, got %s' % raw.dtype)
        a = np.ascontiguousarray(raw)
        t = torch.from_numpy(a.view(np.int16) if code == PP_U16 else a)
        given = None
    elif isinstance(raw, torch.Tensor):
        shape = _shape3(raw.shape)
        if raw.dtype == torch.uint8:
            code = PP_U8
        elif raw.dtype == torch.float32:
            code = PP_F32
        elif _T_UINT16 is not None and raw.dtype == _T_UINT16:
            code = PP_U16
        else:
            raise ValueError('a raw volume is uint8, uint16 or float32, got %s' % raw.dtype)
        t = raw.detach().contiguous()
        if code == PP_U16:
            t = t.view(torch.int16)
        given = raw.device
    else:
        raise ValueError('a raw volume is a numpy array or a torch tensor, got %s' % type(raw).__name__)
    return RawVolume(t.to(_resolve_device(device, given)), code, shape)


def _scratch(query: str, *args, dev) -> Tuple[torch.Tensor, int]:
    """(buffer, bytes): the scratch an entry point needs for these sizes, as its query `query` (vg_..._scratch_bytes) tells; allocated as
    that many bytes (torch aligns every allocation to 512 bytes, the entries ask for 16)."""
    nbytes = int(getattr(lib, query)(*args))
    _check(nbytes, query)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _moments_into(v: RawVolume, ms: torch.Tensor) -> None:
    scratch, nbytes = _scratch('vg_slice_moments_scratch_bytes', v.nxy, v.shape[2], dev=v.buf.device)
    _check(lib.vg_slice_moments(_p(v.buf), v.code, v.nxy, v.shape[2], _p(ms), _p(scratch), nbytes, stream()), 'vg_slice_moments')


def _zscore_into(v: RawVolume, ms: torch.Tensor, out: torch.Tensor, counter_ptr: int) -> None:
    _check(lib.vg_zscore_slices(_p(v.buf), v.code, v.nxy, v.shape[2], _p(ms), _p(out), counter_ptr, stream()), 'vg_zscore_slices')


def slice_moments(vol, device=None) -> torch.Tensor:
    """[Z, 2] fp32 on the device: (mean, population standard deviation) of every z-slice, accumulated in fp64 and rounded once."""
    v = as_raw_volume(vol, device)
    with torch.cuda.device(v.buf.device):
        ms = torch.empty(v.shape[2], 2, device=v.buf.device)
        _moments_into(v, ms)
    return ms


def zscore_slices(vol, device=None, return_count: bool = False):
    """fp32 [X,Y,Z] on the device: (x - mean_z) / std_z where std_z > 0, else x - mean_z (z_score_norm, utils.py:68-83, per z-slice).
    return_count: also the one-element int32 device tensor that counts the non-finite values written."""
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        ms = torch.empty(v.shape[2], 2, device=dev)
        out = torch.empty(v.shape, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        _moments_into(v, ms)
        _zscore_into(v, ms, out, _p(counter))
    return (out, counter) if return_count else out


def _dev_f32(x, what='x') -> torch.Tensor:
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError('%s must be an fp32 device tensor' % what)
    return x.contiguous()


def _order_stats_into(x: torch.Tensor, ranks: Sequence[int], out_ptr: int) -> None:
    n, R = x.numel(), len(ranks)
    scratch, nbytes = _scratch('vg_order_stats_scratch_bytes', n, R, dev=x.device)
    rk = (C.c_int64 * R)(*ranks)
    _check(lib.vg_order_stats(_p(x), n, rk, R, out_ptr, _p(scratch), nbytes, stream()), 'vg_order_stats')


def order_stats(x: torch.Tensor, ranks: Sequence[int]) -> torch.Tensor:
    """sorted(x.flatten())[ranks] as an fp32 device tensor, exact, for up to 4 ranks (duplicates allowed); x: fp32 on the device, finite,
    fewer than 2^31 elements.  Enqueue-only: a radix select of 9 launches, no sort and no read-back."""
    ranks = [int(r) for r in ranks]
    x = _dev_f32(x)
    n = x.numel()
    if not 1 <= len(ranks) <= MAX_RANKS:
        raise ValueError('between 1 and %d ranks, got %d' % (MAX_RANKS, len(ranks)))
    if n < 1 or n >= 2 ** 31:
        raise ValueError('order_stats serves 1 <= n < 2^31 elements, got %d' % n)
    for r in ranks:
        if not 0 <= r < n:
            raise ValueError('rank %d outside [0, %d)' % (r, n))
    with torch.cuda.device(x.device):
        out = torch.empty(len(ranks), device=x.device)
        _order_stats_into(x, ranks, _p(out))
    return out


def percentile_rank(n: int, per: float) -> Tuple[int, int, float]:
    """(lower rank, upper rank, fraction) of scipy.stats.scoreatpercentile(a, per) with the default 'fraction' interpolation on n values:
    index = per / 100 * (n - 1) in Python floats, lower = floor(index), upper = min(lower + 1, n - 1), fraction = index - lower (exact);
    the score is a[lower] * (1 - fraction) + a[upper] * fraction."""
    per = float(per)
    if n < 1:
        raise ValueError('percentile of an empty array')
    if not 0.0 <= per <= 100.0:
        raise ValueError('percentile must be in the range [0, 100], got %r' % per)
    idx = per / 100.0 * (n - 1)
    lo = int(math.floor(idx))
    return lo, min(lo + 1, n - 1), idx - lo


def percentiles(x: torch.Tensor, per) -> np.ndarray:
    """scipy.stats.scoreatpercentile(x, per) ('fraction' interpolation) for a scalar or a sequence per, as float64 on the host: the order
    statistics are selected on the device, two percentiles per select, and interpolated in float64 here (a synchronising read)."""
    pers = [float(p) for p in np.atleast_1d(np.asarray(per, dtype=np.float64))]
    x = _dev_f32(x)
    n = x.numel()
    out = []
    for i in range(0, len(pers), 2):
        rf = [percentile_rank(n, p) for p in pers[i:i + 2]]
        a = order_stats(x, [r for lo, hi, _ in rf for r in (lo, hi)]).cpu().numpy().astype(np.float64)
        for j, (_, _, f) in enumerate(rf):
            out.append(a[2 * j] * (1.0 - f) + a[2 * j + 1] * f if f != 0.0 else a[2 * j])
    return np.asarray(out, dtype=np.float64)


def _clip_into(z: torch.Tensor, lower_thresh: float, upper_thresh: float, rescale: bool, limits_ptr: int, out: torch.Tensor) -> None:
    """Percentile clip of the fp32 device volume z (optionally with the rescale to [-1, 1]) into out, which may be z."""
    n = z.numel()
    lo = percentile_rank(n, lower_thresh)
    hi = percentile_rank(n, upper_thresh)
    stats = torch.empty(4, device=z.device)
    _order_stats_into(z, [lo[0], lo[1], hi[0], hi[1]], _p(stats))
    _check(lib.vg_clip_rescale(_p(z), n, _p(stats), lo[2], hi[2], 1 if rescale else 0, limits_ptr, _p(out), stream()), 'vg_clip_rescale')


# The words of a status block (_state_block).  Words 4 and 5 mean one thing in prepare_imaging's block and another in prepare_segmentation's.
W_NONFINITE, W_INVERTED, W_LO, W_HI = 0, 1, 2, 3     # the non-finite counter, the inversion flag of a label volume, the fp32 limits (lp, up)
W_KEPT, W_KEPT_NONFINITE = 4, 5                     # imaging: the kept and the non-finite count of the 'outliers' stage
W_MODE, W_MODE_COUNT, W_MODE_STATUS = 4, 5, 6       # labels: the mode's value (fp32 bits), its count, vg_value_mode's status


def _state_block(dev, words: int = 4) -> torch.Tensor:
    """32-bit words on the device that the kernels fill and one copy reads back, zeroed: prepare_imaging uses 4, and 8 with an 'outliers'
    stage (vg_outlier_limits writes two); prepare_segmentation's words 1 to 7 are written by vg_label_finish."""
    return torch.zeros(words, dtype=torch.int32, device=dev)


def _word(state: torch.Tensor, w: int) -> int:                # the device address of word w
    return _p(state) + 4 * w


def _read_state(state: torch.Tensor, check: bool = True, outliers: bool = False):
    """(words, lp, up): the status block on the host (a synchronising copy) and its two limits; check: raises what both recipes raise.
    outliers: prepare_imaging's block with an 'outliers' stage, whose words 4 and 5 are checked too (never a label block)."""
    host = state.cpu()
    lo, hi = (float(x) for x in host[W_LO:W_HI + 1].view(torch.float32))
    if check:
        if int(host[W_NONFINITE]) != 0 or (outliers and int(host[W_KEPT_NONFINITE]) != 0):
            raise ValueError('NaN detected')
        if outliers and int(host[W_KEPT]) == 0:
            raise ValueError(OUTLIERS_ERROR)
        if lo == hi:
            raise ValueError(MINMAX_ERROR)
    return host, lo, hi


def preprocess_rsom_images(vol, lower_thresh: float = 0.05, upper_thresh: float = 99.95, device=None) -> torch.Tensor:
    """preprocess_rsom_images (main.py:127-150) on the device: the slice-wise z-score clipped to its lower_thresh-th and upper_thresh-th
    percentile; fp32 [X,Y,Z].  Enqueue-only."""
    percentile_rank(1, lower_thresh), percentile_rank(1, upper_thresh)
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        state = _state_block(dev)
        ms = torch.empty(v.shape[2], 2, device=dev)
        z = torch.empty(v.shape, device=dev)
        _moments_into(v, ms)
        _zscore_into(v, ms, z, _word(state, W_NONFINITE))
        _clip_into(z, lower_thresh, upper_thresh, False, _word(state, W_LO), z)
    return z


# ------------------------------------------------------------------------------------------------ Lanczos-4 volume resize
# resize_volume (utils.py:224-255) resamples with cv2.resize(..., interpolation=cv2.INTER_LANCZOS4).  TP, unverifiable here: what follows
# restates OpenCV's float32 single-channel Lanczos-4 resize (the index table of its resize, the coefficients of its interpolateLanczos4)
# from its published source; OpenCV itself was never run against it.  The contract is in include/vangan_hip.h "Volume resize".
LANCZOS_TAPS = 8
MAX_AXIS = 1 << 20                         # vg_resample_axis serves L, T <= 2^20
_FLT_EPSILON = float(np.finfo(np.float32).eps)
_S45 = 0.70710678118654752440084436210485
_CS = ((1.0, 0.0), (-_S45, -_S45), (0.0, 1.0), (_S45, -_S45), (-1.0, 0.0), (_S45, _S45), (0.0, -1.0), (-_S45, _S45))


def lanczos4_weights(t) -> np.ndarray:
    """The 8 float32 coefficients of the phase t in [0, 1) (a float32 value): the unit tap at k = 3 when t < FLT_EPSILON; else, in float64,
    y_k = -(t + 3 - k) pi / 4 and c_k = float32((-1)^k sin(y_k) / y_k^2) with (-1)^k sin(y_k) = cs_k[0] sin(y_0) + cs_k[1] cos(y_0) (y_k is
    y_0 advanced by k eighths of a turn), summed in float32 in tap order and scaled by float32(1 / sum): sinc(u) sinc(u / 4) at
    u = t + 3 - k, normalised.  math.sin / math.cos: one libm whatever the numpy build."""
    t = float(np.float32(t))
    w = np.zeros(LANCZOS_TAPS, np.float32)
    if t < _FLT_EPSILON:
        w[3] = 1.0
        return w
    y0 = -(t + 3.0) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    total = np.float32(0.0)
    for k in range(LANCZOS_TAPS):
        y = -(t + 3.0 - k) * math.pi * 0.25
        w[k] = np.float32((_CS[k][0] * s0 + _CS[k][1] * c0) / (y * y))
        total = np.float32(total + w[k])
    return w * np.float32(np.float32(1.0) / total)


@functools.lru_cache(maxsize=32)
def _lanczos4_table(L: int, T: int):
    scale = 1.0 / (T / L)
    fx = ((np.arange(T, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    t = fx - sx                                                    # float32 - float32
    w8 = np.empty((T, LANCZOS_TAPS), np.float32)
    phases = {}
    for j, tj in enumerate(t.tolist()):                            # the phases of a rational scale repeat: each is evaluated once
        w = phases.get(tj)
        if w is None:
            w = phases[tj] = lanczos4_weights(tj)
        w8[j] = w
    first = sx.astype(np.int32) - np.int32(3)
    first.setflags(write=False), w8.setflags(write=False)
    return first, w8


def lanczos4_table(L: int, T: int) -> Tuple[np.ndarray, np.ndarray]:
    """(first int32 [T], w8 float32 [T, 8]) of one axis resized from L to T samples, on the host (read-only arrays): output dx reads the
    source indices first[dx] + k, k = 0 .. 7, each clamped to [0, L - 1] by the kernel, with the weights w8[dx].  scale = 1 / (T / L) in
    float64, fx = float32((dx + 0.5) scale - 0.5), sx = floor(fx), t = fx - float32(sx) in float32, first = sx - 3, w8[dx] =
    lanczos4_weights(t)."""
    L, T = operator.index(L), operator.index(T)
    if not (1 <= L <= MAX_AXIS and 1 <= T <= MAX_AXIS):
        raise ValueError('an axis is resized from 1 <= L <= 2^20 to 1 <= T <= 2^20 samples, got L = %d, T = %d' % (L, T))
    return _lanczos4_table(L, T)


def _target3(target_size) -> Tuple[int, int, int]:
    """Three integers >= 1 (a trailing 1 is tolerated, as in a volume's shape)."""
    try:
        tgt = _drop_channel(tuple(operator.index(s) for s in target_size))
    except TypeError:
        raise ValueError('target_size is three integers, got %r' % (target_size,)) from None
    if len(tgt) != 3 or min(tgt) < 1 or max(tgt) > MAX_AXIS:
        raise ValueError('target_size is three integers in [1, 2^20], got %r' % (target_size,))
    return tgt


def _upload_table(first, w8, T: int, dev: torch.device) -> torch.Tensor:
    """first [T] and w8 [T, 8] as one int32 device buffer of 9 T words (one upload of 36 T bytes): first, then the bits of w8."""
    first, w8 = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(w8, np.float32)
    if first.shape != (T,) or w8.shape != (T, LANCZOS_TAPS):
        raise ValueError('a table is (first int32 [T], w8 float32 [T, 8])')
    return torch.from_numpy(np.concatenate([first, w8.ravel().view(np.int32)])).to(dev)


@functools.lru_cache(maxsize=32)
def _device_table(L: int, T: int, dev: torch.device) -> torch.Tensor:
    """The uploaded lanczos4_table(L, T), kept per device: a later resize between the same lengths neither rebuilds nor uploads it, so the
    call only enqueues.  Read-only on the device; at most 32 tables of 36 T bytes are held."""
    first, w8 = lanczos4_table(L, T)
    return _upload_table(first, w8, T, dev)


def resample_axis(x: torch.Tensor, T: int, table=None) -> torch.Tensor:
    """One pass of the resize: x fp32 [outer, L, inner] on the device -> [outer, T, inner], resampled along its middle axis with
    lanczos4_table(L, T), or with table = (first int32 [T], w8 float32 [T, 8]) given as host arrays.  Enqueue-only; x is not modified."""
    T = operator.index(T)
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        raise ValueError('x must be a contiguous fp32 device tensor [outer, L, inner]')
    outer, L, inner = x.shape
    with torch.cuda.device(x.device):
        tab = _device_table(L, T, x.device) if table is None else _upload_table(table[0], table[1], T, x.device)
        out = torch.empty(outer, T, inner, device=x.device)
        _check(lib.vg_resample_axis(_p(x), outer, L, inner, T, _p(tab), _p(tab) + 4 * T, _p(out), stream()), 'vg_resample_axis')
    return out


def _resize_f32(x: torch.Tensor, tgt: Tuple[int, int, int]) -> torch.Tensor:
    """x: fp32 [X,Y,Z] on the device, contiguous.  The passes Y, X, Z; an axis that already has its length is skipped."""
    for axis in (1, 0, 2):
        s = x.shape
        if s[axis] != tgt[axis]:
            outer, inner = math.prod(s[:axis]), math.prod(s[axis + 1:])
            x = resample_axis(x.view(outer, s[axis], inner), tgt[axis]).view(s[:axis] + (tgt[axis],) + s[axis + 1:])
    return x


def _to_f32(v: RawVolume, counter_ptr: int) -> torch.Tensor:
    """The conversion to fp32: the z-score kernel with a table of zeros computes x - 0 (and counts the non-finite values)."""
    ms = torch.zeros(v.shape[2], 2, device=v.buf.device)
    z = torch.empty(v.shape, device=v.buf.device)
    _zscore_into(v, ms, z, counter_ptr)
    return z


def resize_volume(vol, target_size, device=None) -> torch.Tensor:
    """resize_volume (utils.py:224-255) on the device: vol [X,Y,Z] (whatever as_raw_volume takes; uint8 / uint16 stacks are converted to
    fp32 first) -> fp32 [T0,T1,T2], Lanczos-4 as cv2.resize(..., INTER_LANCZOS4) computes it on float32 (TP: restated, never run against
    OpenCV).  The reference resizes every z-slice in 2-D (OpenCV: columns, then rows), then every x-slab; as 1-D passes with fp32
    intermediates that is Y, then X, then Z, and Z alone when X and Y already match.  An axis whose length equals its target is skipped
    (OpenCV <= 4.5 applies the exact unit tap there; newer versions differ from it by at most one ulp: the one known ambiguity).  The
    reference works only for target_size[0] == target_size[1] -- its slice assignment needs that; here axis a simply goes to
    target_size[a].  Enqueue-only; arguments are validated before the device is touched.  When no pass is needed the fp32 volume itself is
    returned (for an fp32 device tensor: the same storage)."""
    tgt = _target3(target_size)
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        x = v.buf.view(v.shape) if v.code == PP_F32 else _to_f32(v, _word(_state_block(dev), W_NONFINITE))
        return _resize_f32(x, tgt)


def _minmax_rescale(x: torch.Tensor, limits_ptr: int) -> None:
    """min_max_norm and (x - 0.5) / 0.5 in place: vg_minmax finds the extremes, and the clip pass with (min, max) as its limits (fractions 0)
    clips nothing and applies ((x - min) / (max - min) - 0.5) / 0.5; it also files (min, max) at limits_ptr."""
    n = x.numel()
    mm = torch.zeros(1, 4, device=x.device)
    _check(lib.vg_minmax(_p(x), 1, n, _p(mm), stream()), 'vg_minmax')
    stats = torch.stack((mm[0, 0], mm[0, 1], mm[0, 1], mm[0, 1]))
    _check(lib.vg_clip_rescale(_p(x), n, _p(stats), 0.0, 0.0, 1, limits_ptr, _p(x), stream()), 'vg_clip_rescale')


# ------------------------------------------------------------------------------------------------ imaging filters
# scipy.ndimage.median_filter (main.py:36) and threshold_outliers (utils.py:108-133, main.py:34): csrc/vg_filters.hip, include/vangan_hip.h
# "Imaging filters", DESIGN.md section 3.15.
STAGES = ('median', 'outliers', 'rsom')
OUTLIERS_ERROR = 'threshold_outliers: no voxel lies within the threshold'


def _median_size3(size) -> Tuple[int, int, int]:
    """(sx, sy, sz), each 1 or 3, from an int (the same along every axis) or a 3-tuple: what vg_median3 serves."""
    try:
        s3 = (operator.index(size),) * 3
    except TypeError:
        try:
            s3 = tuple(operator.index(s) for s in size)
        except TypeError:
            raise ValueError('a median size is an int or three ints, got %r' % (size,)) from None
    if len(s3) != 3 or any(s not in (1, 3) for s in s3):
        raise ValueError('the median filter serves sizes of 1 or 3 along each of three axes, got %r' % (size,))
    return s3


def _outlier_threshold(threshold) -> float:
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('the outlier threshold is a number, got %r' % (threshold,)) from None
    if not (math.isfinite(thr) and thr > 0.0 and math.isfinite(float(np.float32(thr))) and float(np.float32(thr)) > 0.0):
        raise ValueError('the outlier threshold must be finite and > 0, got %r' % (threshold,))
    return thr


def _median_into(v: RawVolume, size3: Tuple[int, int, int], counter_ptr: int) -> torch.Tensor:
    X, Y, Z = v.shape
    out = torch.empty(v.shape, device=v.buf.device)
    _check(lib.vg_median3(_p(v.buf), v.code, X, Y, Z, size3[0], size3[1], size3[2], _p(out), counter_ptr, stream()), 'vg_median3')
    return out


def _volume_moments_into(v: RawVolume, ms: torch.Tensor) -> None:
    scratch, nbytes = _scratch('vg_volume_moments_scratch_bytes', v.numel, dev=v.buf.device)
    _check(lib.vg_volume_moments(_p(v.buf), v.code, v.numel, _p(ms), _p(scratch), nbytes, stream()), 'vg_volume_moments')


def _outlier_limits_into(v: RawVolume, threshold: float, stats: torch.Tensor, counts_ptr: int) -> None:
    """stats (4 fp32 on the device) = (lo, lo, hi, hi) of v; counts_ptr names (kept, non-finite): the second word is added to."""
    ms = torch.empty(2, device=v.buf.device)
    _volume_moments_into(v, ms)
    _check(lib.vg_outlier_limits(_p(v.buf), v.code, v.numel, _p(ms), threshold, _p(stats), counts_ptr, stream()), 'vg_outlier_limits')


def _outliers_into(v: RawVolume, threshold: float, rescale: bool, state: torch.Tensor) -> torch.Tensor:
    """threshold_outliers of v as a new fp32 tensor (optionally with the rescale to [-1, 1]); state: the 8-word block of prepare_imaging."""
    stats = torch.empty(4, device=v.buf.device)
    _outlier_limits_into(v, threshold, stats, _word(state, W_KEPT))
    if v.code == PP_F32:
        x, out = v.buf.view(v.shape), torch.empty(v.shape, device=v.buf.device)
    else:
        x = out = _to_f32(v, _word(state, W_NONFINITE))
    _check(lib.vg_clip_rescale(_p(x), v.numel, _p(stats), 0.0, 0.0, 1 if rescale else 0, _word(state, W_LO), _p(out), stream()), 'vg_clip_rescale')
    return out


def median_filter(vol, size=3, device=None, return_count: bool = False):
    """scipy.ndimage.median_filter(vol, size=size) with its default mode='reflect', on the device: fp32 [X,Y,Z], exact (a median is one of
    the values).  size: an int or (sx, sy, sz), each 1 or 3 -- 3 is the 3-D median, (3, 3, 1) the median of every z-slice; anything else
    raises ValueError before the device is touched.  return_count: also the one-element int32 device tensor that counts the non-finite
    voxels of vol; where a window holds a NaN the value is unspecified.  Enqueue-only."""
    size3 = _median_size3(size)
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        out = _median_into(v, size3, _p(counter))
    return (out, counter) if return_count else out


def volume_moments(vol, device=None) -> torch.Tensor:
    """[2] fp32 on the device: (mean, population standard deviation) of the whole volume, accumulated in fp64 and rounded once."""
    v = as_raw_volume(vol, device)
    with torch.cuda.device(v.buf.device):
        ms = torch.empty(2, device=v.buf.device)
        _volume_moments_into(v, ms)
    return ms


def outlier_limits(vol, threshold=6, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(limits, counts) on the device: limits = (lower, upper) fp32, the smallest and the largest value x of vol with
    |(x - mean) / std| <= threshold in fp32 (the selection of threshold_outliers, utils.py:119-128); counts = (kept, non-finite) int32,
    kept saturating at 2^32 - 1 (read it as unsigned).  No kept voxel (a constant volume, a NaN in it): limits = (+inf, -inf).
    Enqueue-only."""
    thr = _outlier_threshold(threshold)
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        stats = torch.empty(4, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        _outlier_limits_into(v, thr, stats, _p(counts))
    return stats[1:3], counts


def threshold_outliers(vol, threshold=6, device=None) -> torch.Tensor:
    """threshold_outliers (utils.py:108-133) on the device: vol clipped to outlier_limits(vol, threshold); fp32 [X,Y,Z].  Moments, limits,
    then the clip pass with those limits and no rescale.  threshold must be finite and > 0.  Enqueue-only."""
    thr = _outlier_threshold(threshold)
    v = as_raw_volume(vol, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        return _outliers_into(v, thr, False, _state_block(dev, 8))


def _stages(preprocess) -> Tuple[str, ...]:
    if preprocess is None:
        return ()
    names = (preprocess,) if isinstance(preprocess, str) else preprocess
    try:
        names = tuple(names)
    except TypeError:
        names = (names,)
    if not names or any(not isinstance(s, str) or s not in STAGES for s in names) or len(set(names)) != len(names):
        raise ValueError("preprocess must be None, 'rsom', 'median', 'outliers' or a sequence of these, each at most once, got %r" % (preprocess,))
    return names


def prepare_imaging(raw, preprocess='rsom', lower_thresh: float = 0.05, upper_thresh: float = 99.95, check: bool = True,
                    device=None, target_size=None, median_size=3, outlier_threshold=6) -> torch.Tensor:
    """Raw imaging volume -> what stitch_subvolumes and DataPipeline take: fp32 [X,Y,Z,1] in [-1, 1] on the device.
    preprocess='rsom': z-score per z-slice, clip to the two percentiles, min-max, (x - 0.5) / 0.5 (main.py:127-150 and
    preprocessing.py:179-185).  preprocess=None: min-max and (x - 0.5) / 0.5 alone (process_tiff without a preprocess_fn).
    preprocess='median': median_filter(size=median_size) first; 'outliers': threshold_outliers(threshold=outlier_threshold) first.  A
    sequence of these names, each at most once -- ('median', 'rsom'), ('outliers', 'median') -- applies the stages left to right, as one
    composes them inside the reference's preprocess_fn; a stage that follows another reads the fp32 result of the one before it.  When the
    last stage is a clip whose limits are on the device ('rsom', 'outliers') and there is no resize, the clip and the rescale are one
    launch; otherwise a min / max pass and the rescale follow.
    check=True reads one small block back and raises ValueError('NaN detected') when a non-finite value was met (preprocessing.py:191-215
    prints that and skips the file), ValueError('threshold_outliers: no voxel lies within the threshold') when the 'outliers' stage kept
    nothing (numpy raises there too), and min_max_norm's ValueError when the two limits coincide.  check=False reads nothing back: the
    call only enqueues, and the launches it makes do not depend on the data.
    target_size=(T0, T1, T2): process_tiff's resize=True (preprocessing.py:170-185) -- the preprocessed volume (clipped, not yet rescaled)
    goes through resize_volume before min_max_norm, and the result is [T0,T1,T2,1].  Lanczos-4 overshoots, so the extremes are taken from
    the resized volume by a min / max pass.  The non-finite count is that of the values before the resize.  None: no resize, today's
    launches; a target equal to the volume's shape gives the same bits as None."""
    stages = _stages(preprocess)
    percentile_rank(1, lower_thresh), percentile_rank(1, upper_thresh)
    size3 = _median_size3(median_size)
    thr = _outlier_threshold(outlier_threshold)
    tgt = None if target_size is None else _target3(target_size)
    v = as_raw_volume(raw, device)
    dev = v.buf.device
    with torch.cuda.device(dev):
        outliers = 'outliers' in stages
        state = _state_block(dev, 8) if outliers else _state_block(dev)
        fused = bool(stages) and stages[-1] in ('rsom', 'outliers') and tgt is None
        out = None
        for i, stage in enumerate(stages):
            rescale = fused and i == len(stages) - 1
            if stage == 'median':
                out = _median_into(v, size3, _word(state, W_NONFINITE))
            elif stage == 'outliers':
                out = _outliers_into(v, thr, rescale, state)
            else:
                ms = torch.empty(v.shape[2], 2, device=dev)
                out = torch.empty(v.shape, device=dev)
                _moments_into(v, ms)
                _zscore_into(v, ms, out, _word(state, W_NONFINITE))
                _clip_into(out, lower_thresh, upper_thresh, rescale, _word(state, W_LO), out)
            v = RawVolume(out, PP_F32, v.shape)
        if not stages:
            out = _to_f32(v, _word(state, W_NONFINITE))
        if tgt is not None:
            out = _resize_f32(out, tgt)                 # `out` itself when no axis changes: ours, so the rescale below may run in place
        if not fused:
            _minmax_rescale(out, _word(state, W_LO))
        if check:
            _read_state(state, outliers=outliers)
    return out[..., None]


# ------------------------------------------------------------------------------------------------ label volumes
def _value_mode_into(x: torch.Tensor, mm_ptr, result: torch.Tensor) -> None:
    """result (4 int32 words on the device) = vg_value_mode of x, of its min-max normalisation when mm_ptr names a vg_minmax row."""
    n = x.numel()
    scratch, nbytes = _scratch('vg_value_mode_scratch_bytes', n, dev=x.device)
    _check(lib.vg_value_mode(_p(x), n, mm_ptr, _p(result), _p(scratch), nbytes, stream()), 'vg_value_mode')


def _mode_count_ok(n: int, what: str) -> None:
    if n < 1 or n >= 2 ** 31:
        raise ValueError('%s serves 1 <= n < 2^31 elements, got %d' % (what, n))


def value_mode(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(value, count): the most frequent value of x as a one-element fp32 device tensor and how often it occurs as a one-element int32
    device tensor -- scipy.stats.mode(x, axis=None): among equally frequent values the smallest; -0.0 and +0.0 are one value.  Exact.
    x: fp32 on the device, fewer than 2^31 elements; non-finite values are not counted (all non-finite: a NaN with count 0).
    Enqueue-only: four launches, no sort and no read-back; the hash table it counts in takes 16 to 32 bytes of scratch per element."""
    x = _dev_f32(x)
    _mode_count_ok(x.numel(), 'value_mode')
    with torch.cuda.device(x.device):
        result = torch.empty(4, dtype=torch.int32, device=x.device)
        _value_mode_into(x, None, result)
    return result[0:1].view(torch.float32), result[1:2]


@functools.lru_cache(maxsize=8)
def _label_clamp_stats(dev: torch.device) -> torch.Tensor:
    """(0, 0, 255, 255) on the device, kept per device: vg_clip_rescale's order statistics for the clamp of a resized label stack."""
    return torch.tensor([0.0, 0.0, 255.0, 255.0], dtype=torch.float32).to(dev)


def prepare_segmentation(raw, check: bool = True, device=None, target_size=None, return_info: bool = False):
    """Raw label volume -> what DataPipeline takes as a segmentation volume: fp32 [X,Y,Z,1] in {-1, +1} on the device -- process_tiff's
    partition 'S' branch (preprocessing.py:173-189): min_max_norm; when the most frequent value of the normalised stack is 1 (the
    background is the bright level) the stack is inverted, |y - 1|; (y - 0.5) / 0.5; negative -> -1, else +1.  Every step in fp32 as numpy
    rounds it; the mode is exact (value_mode's table, counting the normalised values: the normalisation can merge neighbouring values).
    raw: whatever as_raw_volume takes.  target_size=(T0, T1, T2): process_tiff's resize=True -- resize_volume, then the clamp to [0, 255]
    the reference applies to a resized label stack, then the above; a target equal to the volume's shape is skipped, clamp included.
    check=True reads one small block back and raises ValueError('NaN detected') when the raw volume holds a non-finite value,
    min_max_norm's ValueError when the two limits coincide, and RuntimeError on a non-zero status word of the mode.  check=False reads
    nothing back: the call only enqueues, and the launches it makes do not depend on the data.  return_info=True: (out, dict(inverted,
    mode, count, min, max)) -- the mode of the normalised stack and its count, the limits of the stack; this needs the read-back.
    Temporary device memory: the fp32 volume and the mode's table of 16 to 32 bytes per voxel (1 GiB at 512x512x140)."""
    tgt = None if target_size is None else _target3(target_size)
    v = as_raw_volume(raw, device)
    if tgt == tuple(v.shape):
        tgt = None
    _mode_count_ok(math.prod(v.shape if tgt is None else tgt), 'prepare_segmentation')
    dev = v.buf.device
    with torch.cuda.device(dev):
        state = _state_block(dev, 8)                                # [0] non-finite counter, [1..7] written by vg_label_finish
        x = _to_f32(v, _word(state, W_NONFINITE))                   # ours: everything below runs in place
        if tgt is not None:
            x = _resize_f32(x, tgt)
            n = x.numel()
            _check(lib.vg_clip_rescale(_p(x), n, _p(_label_clamp_stats(dev)), 0.0, 0.0, 0, _word(state, W_LO), _p(x), stream()), 'vg_clip_rescale')
        n = x.numel()
        mm = torch.zeros(1, 4, device=dev)
        _check(lib.vg_minmax(_p(x), 1, n, _p(mm), stream()), 'vg_minmax')
        result = torch.empty(4, dtype=torch.int32, device=dev)
        _value_mode_into(x, _p(mm), result)
        _check(lib.vg_label_finish(_p(x), n, _p(mm), _p(result), _p(x), _p(state), stream()), 'vg_label_finish')
        info = None
        if check or return_info:
            host, lo, hi = _read_state(state, check)
            if check and int(host[W_MODE_STATUS]) != 0:
                raise RuntimeError('vg_value_mode reported status %d' % int(host[W_MODE_STATUS]))
            info = dict(inverted=bool(int(host[W_INVERTED])), mode=float(host[W_MODE:W_MODE + 1].view(torch.float32)[0]),
                        count=int(host[W_MODE_COUNT]), min=lo, max=hi)
    out = x[..., None]
    return (out, info) if return_info else out
