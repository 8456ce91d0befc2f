"""Raw-volume preprocessing on MI355X: the imaging-domain recipe the reference runs before run_mapping (main.py:255-270) --
preprocess_rsom_images (main.py:127-150: z-score every z-slice, clip to two percentiles of the whole volume with
scipy.stats.scoreatpercentile) followed by process_tiff's min_max_norm and (x - 0.5) / 0.5 and its NaN check (preprocessing.py:179-215)
-- without the TIFF I/O, the resize and the label-domain branch.  The arithmetic runs in csrc/vg_preproc.hip
(include/vangan_hip.h "Raw-volume preprocessing"); this module owns buffers, ranks and checks.

A volume is [X,Y,Z] (or [X,Y,Z,1]) with Z innermost -- process_tiff's layout after its transpose -- as uint8, uint16 or float32, a numpy
array or a torch tensor, on the host or on the device.  torch has no uint16 arithmetic, so a 16-bit stack travels as the int16 tensor of
the same bytes and the kernels read it as what it is."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check as _check, lib
from .ops import _p, stream

PP_U8, PP_U16, PP_F32 = 0, 1, 2            # VG_PP_U8, VG_PP_U16, VG_PP_F32
MAX_RANKS = 4                              # VG_PP_MAX_RANKS
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


def _shape3(shape) -> Tuple[int, int, int]:
    shape = tuple(int(s) for s in shape)
    if len(shape) == 4 and shape[3] == 1:
        shape = shape[:3]
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


def _moments_into(v: RawVolume, ms: torch.Tensor) -> None:
    X, Y, Z = v.shape
    nbytes = int(lib.vg_slice_moments_scratch_bytes(v.nxy, Z))
    _check(nbytes, 'vg_slice_moments_scratch_bytes')
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=v.buf.device)
    _check(lib.vg_slice_moments(_p(v.buf), v.code, v.nxy, Z, _p(ms), _p(scratch), nbytes, stream()), 'vg_slice_moments')


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
    nbytes = int(lib.vg_order_stats_scratch_bytes(n, R))
    _check(nbytes, 'vg_order_stats_scratch_bytes')
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=x.device)
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


def _state_block(dev) -> torch.Tensor:
    """Four 32-bit words read back in one copy: [0] the non-finite counter, [2], [3] the fp32 limits (lp, up)."""
    return torch.zeros(4, dtype=torch.int32, device=dev)


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
        _zscore_into(v, ms, z, _p(state))
        _clip_into(z, lower_thresh, upper_thresh, False, _p(state) + 8, z)
    return z


def prepare_imaging(raw, preprocess: Optional[str] = 'rsom', lower_thresh: float = 0.05, upper_thresh: float = 99.95, check: bool = True,
                    device=None) -> torch.Tensor:
    """Raw imaging volume -> what stitch_subvolumes and DataPipeline take: fp32 [X,Y,Z,1] in [-1, 1] on the device.
    preprocess='rsom': z-score per z-slice, clip to the two percentiles, min-max, (x - 0.5) / 0.5 (main.py:127-150 and
    preprocessing.py:179-185).  preprocess=None: min-max and (x - 0.5) / 0.5 alone (process_tiff without a preprocess_fn).
    check=True reads one small block back and raises ValueError('NaN detected') when a non-finite value was met (preprocessing.py:191-215
    prints that and skips the file) and min_max_norm's ValueError when the two limits coincide.  check=False reads nothing back: the call
    only enqueues, and the launches it makes do not depend on the data."""
    if preprocess not in ('rsom', None):
        raise ValueError("preprocess must be 'rsom' or None, got %r" % (preprocess,))
    percentile_rank(1, lower_thresh), percentile_rank(1, upper_thresh)
    v = as_raw_volume(raw, device)
    dev = v.buf.device
    n = v.numel
    with torch.cuda.device(dev):
        state = _state_block(dev)
        ms = torch.empty(v.shape[2], 2, device=dev) if preprocess else torch.zeros(v.shape[2], 2, device=dev)
        z = torch.empty(v.shape, device=dev)
        if preprocess:
            _moments_into(v, ms)
            _zscore_into(v, ms, z, _p(state))
            _clip_into(z, lower_thresh, upper_thresh, True, _p(state) + 8, z)
            out = z
        else:
            _zscore_into(v, ms, z, _p(state))            # mean 0, std 0: x - 0, the conversion to fp32 (and the non-finite count)
            mm = torch.zeros(1, 4, device=dev)
            _check(lib.vg_minmax(_p(z), 1, n, _p(mm), stream()), 'vg_minmax')
            # the clip pass with (min, max) as its limits (fractions 0) clips nothing and applies ((x - min) / (max - min) - 0.5) / 0.5 in
            # place; it also files (min, max) beside the counter
            stats = torch.stack((mm[0, 0], mm[0, 1], mm[0, 1], mm[0, 1]))
            _check(lib.vg_clip_rescale(_p(z), n, _p(stats), 0.0, 0.0, 1, _p(state) + 8, _p(z), stream()), 'vg_clip_rescale')
            out = z
        if check:
            host = state.cpu()
            if int(host[0]) != 0:
                raise ValueError('NaN detected')
            lims = host[2:].view(torch.float32)
            if float(lims[0]) == float(lims[1]):
                raise ValueError(MINMAX_ERROR)
    return out[..., None]

